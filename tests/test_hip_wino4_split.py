"""GPU tests of wino4_plain_split_kernel (ctrlhair_amd/csrc/conv_wino4_split.h; option sean.wino4_split): the ResBlock 3x3 convs
(/root/reference/sean_codes/models/networks/architecture.py:82-91) as Winograd F(4x4,3x3) with the 36 positions, not the 32 GEMM rows,
split between the two waves of a tile group.  Same operations on the same values in the same order as wino4_plain_kernel
(tests/test_wino4_split_model.py is the argument): images and intermediate activations must be IDENTICAL with the option on and off.

Every case runs the ngf = 16 generator with procedural weights, sean.wino = 2, sean.wino4_force = 1 (these calls have fewer tasks than CUs)
and sean.wino4v = 0 (no layer leaves for the pre-transformed-input route)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NGF = 16
BASE = {'sean.wino4_force': 1, 'sean.wino4v': 0}


def _gen(sd, mb, ms, split):
    from ctrlhair_amd.sean.generator import SeanGenerator
    opts = dict(BASE)
    opts.update({'sean.wino': 2, 'sean.wino4_split': split})
    return SeanGenerator(0, f16x3=0, options=opts).load_state_dict(sd, max_batch=mb, max_size=ms)


def _tap_shapes(B, S):
    """Outputs of the F(4x4,3x3) convs (conv_0: '<block>.dx', conv_1: '<block>') and of the 1x1 shortcut conv_1 adds ('<block>.xs')."""
    from ctrlhair_amd.sean import arch
    out = {}
    for b in arch.blocks(NGF):
        r = S // b.res_div
        if r % 32:
            continue
        out[b.name + '.dx'] = (B, b.fmid, r, r)
        out[b.name] = (B, b.fout, r, r)
        if b.learned_shortcut:
            out[b.name + '.xs'] = (B, b.fout, r, r)
    return out


def _run(gen, labels, codes, noise, taps=None):
    dev = gen.device
    bufs = {n: torch.zeros(s, dtype=torch.float32, device=dev) for n, s in (taps or {}).items()}
    for n, t in bufs.items():
        gen.handle.sean_set_tap(n, t.data_ptr())
    out = gen.generate(torch.from_numpy(labels).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(noise).to(dev))
    torch.cuda.synchronize()
    for n in bufs:
        gen.handle.sean_set_tap(n, None)
    return out.cpu().numpy(), {n: t.cpu().numpy() for n, t in bufs.items()}


@pytest.fixture(scope='module')
def sd():
    from ctrlhair_amd import procedural as P
    return P.sean_state_dict(0, NGF)


def _labels(B, S):
    from ctrlhair_amd import procedural as P
    return {'blocky': P.blocky_labels(B, S, grid=8), 'face': np.stack([P.face_like_labels(S, 40 + b) for b in range(B)])}


def _compare(sd, B, S, names):
    from ctrlhair_amd import procedural as P
    on, off = _gen(sd, B, S, 1), _gen(sd, B, S, 0)
    codes, noise = P.style_codes(B, seed=71), P.noise_planes(B, S, NGF, seed=72)
    shapes = _tap_shapes(B, S)
    first = None
    for name in names:
        lab = _labels(B, S)[name]
        a, ta = _run(on, lab, codes, noise, shapes)
        b, tb = _run(off, lab, codes, noise, shapes)
        assert np.isfinite(a).all()
        for n in shapes:
            assert np.abs(tb[n]).max() > 0, n
            assert np.array_equal(ta[n], tb[n]), f'{name} {n}: max |split - plain| = {np.abs(ta[n] - tb[n]).max():.3e}'
        assert np.array_equal(a, b), f'{name}: max |split - plain| = {np.abs(a - b).max():.3e}'
        if first is None:
            first = (lab, a)
    again, _ = _run(on, first[0], codes, noise)            # the same call once more, after calls with other labels
    assert np.array_equal(again, first[1]), 'repeated call differs'
    one, _ = _run(on, first[0][B - 1:], codes[B - 1:], noise[B - 1:])       # ragged batch on the same handle
    ref, _ = _run(off, first[0][B - 1:], codes[B - 1:], noise[B - 1:])
    assert np.array_equal(one, ref)
    on.handle.close()
    off.handle.close()
    return shapes


def test_split_equals_plain_s128(hip_lib, sd):
    """S = 128, B = 3: up_1 at 32 pixels (128 -> 64, 64 -> 64), up_2 at 64 (64 -> 32, 32 -> 32), up_3 at 128 (32 -> 16, 16 -> 16): Cout = 16
    leaves the second row half of the one row tile wholly masked, Cin = 16 is the minimum of four k-steps (the epilogue's exchange right
    behind the ring's first lap), conv_1 adds the 1x1 shortcut's output as its residual; 3 ... 48 tasks."""
    shapes = _compare(sd, 3, 128, ('face', 'blocky'))
    assert {'up_1', 'up_1.dx', 'up_2', 'up_3', 'up_3.dx', 'up_3.xs'} <= set(shapes) and shapes['up_3'] == (3, 16, 128, 128)


def test_split_equals_plain_s512(hip_lib, sd):
    """S = 512, B = 2: 512 tasks at up_3 -- more than CUs, so a block runs several tasks and the exchange reuses a ring stage across task
    boundaries -- and G_middle at 32 pixels: 256 -> 256 (eight row tiles), G_middle_0 reading its residual through the x2 up-sampling
    (res_up = 1), G_middle_1 at the same size."""
    shapes = _compare(sd, 2, 512, ('face',))
    assert shapes['G_middle_0'] == (2, 256, 32, 32) and shapes['up_3'] == (2, 16, 512, 512)


def test_split_against_the_oracle(hip_lib, sd):
    """The split kernel against the reference the sean.wino = 2 leg of tests/test_hip_wino.py is held to -- the oracle's forward pass on
    the same inputs -- at that test's bound of 1e-3."""
    from ctrlhair_amd import procedural as P
    from oracle import sean_oracle as O
    B, S = 1, 128
    g = _gen(sd, B, S, 1)
    codes, noise = P.style_codes(B, seed=71), P.noise_planes(B, S, NGF, seed=72)
    lab = _labels(B, S)['face']
    out, _ = _run(g, lab, codes, noise)
    ref = O.generator_forward(O.to_torch(sd), lab, codes, noise, NGF).numpy()
    d = float(np.abs(out - ref).max())
    print(f'ngf16 S={S}: max |F(4x4) split - oracle| = {d:.3e}')
    assert np.isfinite(out).all() and d <= 1e-3
    g.handle.close()


def test_zencoder_reflection_conv(hip_lib, sd):
    """The Zencoder's 256 -> 512 conv (architecture.py:174; reflection padding + tanh) on the split kernel's reflection instantiation, at
    the smallest size the F(4x4,3x3) kernel takes it: S = 64, a 32 x 32 feature map = ONE spatial tile, so every block sits at the left
    AND the right image edge (the left replacement lives in the jh = 0 waves, the right one in jh = 1).  The feature map must be
    identical; the codes are region means accumulated with float atomics (equal up to their summation order: 1e-6, as
    tests/test_hip_zencoder.py asks of two evaluations of the same map)."""
    from ctrlhair_amd import procedural as P
    B, S = 2, 64
    lab, img = P.blocky_labels(B, S, grid=8, seed=9), P.synthetic_images(B, S, seed=10)
    got = {}
    for split in (1, 0):
        g = _gen(sd, B, S, split)
        feat = torch.zeros(B, 512, S // 2, S // 2, device=g.device)
        g.handle.sean_set_tap('zenc.feat', feat.data_ptr())
        codes = g.encode(torch.from_numpy(img).to(g.device), torch.from_numpy(lab).to(g.device))
        torch.cuda.synchronize()
        g.handle.sean_set_tap('zenc.feat', None)
        got[split] = (feat.cpu().numpy(), codes.cpu().numpy())
        g.handle.close()
    assert np.isfinite(got[1][0]).all() and np.abs(got[1][0]).max() > 0
    assert np.array_equal(got[1][0], got[0][0]), f'max |split - plain| = {np.abs(got[1][0] - got[0][0]).max():.3e}'
    assert np.abs(got[1][1] - got[0][1]).max() <= 1e-6


def test_option_must_precede_finalize(hip_lib, sd):
    g = _gen(sd, 1, 64, 0)
    with pytest.raises(RuntimeError):
        g.handle.set_option('sean.wino4_split', 1)
    g.handle.close()
