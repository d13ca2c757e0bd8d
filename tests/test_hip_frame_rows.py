"""GPU tests of the frame rows (option sean.frame, on top of sean.edge; ctrlhair_amd/csrc/ace_sparse.h): a pixel of the two outermost rings
of a level of 128 pixels and more whose window reaches outside the image along exactly one axis, and whose in-image 5x5 window is uniformly
A < 19, gets gamma / beta from a per-code table row (+ the style-LUT column / row sums of the taps inside) in the interior pass instead of
from the boundary conv.  Both SPADE convs and the style convs zero-pad (normalization.py:105-106,240-247): a tap outside adds nothing, a
hidden position outside is zero.  All cases run through SeanGenerator on the exact-f32 path, as tests/test_hip_interior_groups.py does."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _gen(sd, mb, ms, extra=None):
    from ctrlhair_amd.sean.generator import SeanGenerator
    return SeanGenerator(0, f16x3=0, options=dict(extra or {})).load_state_dict(sd, max_batch=mb, max_size=ms)


def _run(gen, labels, codes, noise):
    dev = gen.device
    out = gen.generate(torch.from_numpy(labels).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(noise).to(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _ring(B, S, width, inner=13, ring=4):
    lab = np.full((B, S, S), ring, np.uint8)
    lab[:, width:S - width, width:S - width] = inner
    return lab


def _label_sets(B, S):
    from ctrlhair_amd import procedural as P
    sets = {}
    sets['one_region'] = np.full((B, S, S), 13, np.uint8)      # every frame pixel but the 2 x 2 corners is a frame-row pixel
    sets['blocky'] = P.blocky_labels(B, S, grid=8)
    sets['ring3'] = _ring(B, S, 3)                             # frame codes with A = the ring's label on the outermost ring only: the next ring sees the
                                                               # inner label, its quads stay boundary quads and the conv writes all four of their pixels
    sets['ring4'] = _ring(B, S, 4)                             # both rings of the frame take codes of the ring's label: whole quads leave the conv
    sets['ring1'] = _ring(B, S, 1)                             # the in-image window of a frame pixel is never uniform: none may be taken
    noclass = P.blocky_labels(B, S, grid=4, seed=77).copy()    # (as tests/test_hip_interior_groups.py: 255 and 19 touch the frame)
    noclass[:, : S // 2, : S // 2] = 255
    noclass[:, S // 2:, S // 2:] = 19
    sets['noclass'] = noclass
    band = np.full((B, S, S), 7, np.uint8)                     # a 2-pixel band of 255 INSIDE the image: to a test on the patch value its
    band[:, :, S // 2:S // 2 + 2] = 255                        # neighbours look like (outside, outside, A, A, A) -- they are boundary pixels
    sets['band255'] = band
    return sets


@pytest.mark.parametrize('ngf,S,B', [(64, 128, 2), (24, 160, 3)])
def test_frame_rows_equal_the_boundary_conv(hip_lib, ngf, S, B):
    """sean.frame = 1 against the boundary-conv evaluation of the same library (sean.frame = 0) at 1e-5 and against the direct evaluation
    (sean.wino = 0) at 2e-4 -- the bounds of tests/test_hip_wino.py::test_straight_edge_pixels_equal_the_boundary_conv for edge rows -- and a
    repeated call gives the same bits.  ngf 24, S 160, B 3: a ragged 128-pixel tile, partial classification tiles, an odd batch."""
    from ctrlhair_amd import procedural as P
    sd = P.sean_state_dict(0, ngf, calibrated=ngf in (16, 64))
    on, off, direct = _gen(sd, B, S, {'sean.frame': 1}), _gen(sd, B, S, {'sean.frame': 0}), _gen(sd, B, S, {'sean.wino': 0})
    codes, noise = P.style_codes(B, seed=51), P.noise_planes(B, S, ngf, seed=52)
    for name, lab in _label_sets(B, S).items():
        a, b, c = _run(on, lab, codes, noise), _run(off, lab, codes, noise), _run(direct, lab, codes, noise)
        d, dd = float(np.abs(a - b).max()), float(np.abs(a - c).max())
        print(f'ngf{ngf} S={S} {name}: max |frame rows - boundary conv| = {d:.3e}, |frame rows - direct| = {dd:.3e}')
        assert np.isfinite(a).all() and d <= 1e-5 and dd <= 2e-4, (name, d, dd)
        assert np.array_equal(a, _run(on, lab, codes, noise)), (name, 'repeated call differs')
    for g in (on, off, direct):
        g.handle.close()


def test_the_reduction_applies(hip_lib):
    """On a single region the 128-pixel level goes from 252 frame quads per sample (four 64-quad chunks) to the 4 corner quads (one chunk):
    the SPADE convs must execute strictly fewer FLOPs with sean.frame = 1, whatever the dense levels below add."""
    from ctrlhair_amd import procedural as P
    ngf, S, B = 64, 128, 2
    sd = P.sean_state_dict(0, ngf)
    codes, noise = P.style_codes(B, seed=51), P.noise_planes(B, S, ngf, seed=52)
    lab = np.full((B, S, S), 13, np.uint8)
    ex = {}
    for frame in (1, 0):
        g = _gen(sd, B, S, {'sean.frame': frame})
        g.handle.profile_enable(True)
        _run(g, lab, codes, noise)
        g.handle.profile_enable(False)
        ex[frame] = g.handle.profile_read(1)['flops_executed']
        g.handle.profile_read(-1)
        g.handle.close()
    print(f'SPADE conv FLOPs executed on one region: {ex[0]:.3e} -> {ex[1]:.3e}')
    assert ex[1] < ex[0]


@pytest.mark.parametrize('name', ['one_region', 'blocky'])
def test_frame_rows_against_the_oracle(hip_lib, name):
    """ngf 64, S 128, first sample, defaults (sean.frame = 1) against the PyTorch oracle at the project's 1e-3."""
    from ctrlhair_amd import procedural as P
    from oracle import sean_oracle as O
    ngf, S = 64, 128
    sd = P.sean_state_dict(0, ngf)
    lab = _label_sets(1, S)[name][:1]
    codes, noise = P.style_codes(1, seed=51), P.noise_planes(1, S, ngf, seed=52)
    gen = _gen(sd, 1, S, {'sean.frame': 1})
    got = _run(gen, lab, codes, noise)
    ref = O.generator_forward(O.to_torch(sd), lab, codes, noise, ngf).numpy()
    d = float(np.abs(got - ref).max())
    print(f'sean.frame=1 ngf={ngf} S={S} {name}: max |hip - oracle| = {d:.3e}')
    assert d <= 1e-3
    gen.handle.close()
