"""CPU tests of tests/stage_local.py: the operand model against torch's bf16 and the f16 split of tests/sh16_emul.py, the restated row exponents,
a "model device" (a torch-f32 forward that rounds its operands by the model and sums every conv in a second association) that must pass every
bound on f16, bf16 and f16x3, and planted faults in that model device: each must fail exactly the stage it is planted in, with the stage and the
pixel kind named, and no later stage (locality).  The model device gives only its convs a second association; its ACE stages are the f32
evaluation of the reference's own code plus one rounding, so on the wide stages "passes every bound" checks the checker, not a second evaluation
of them.  No GPU, no library."""
import numpy as np
import pytest
import torch

from tests import sh16_emul as E
from tests import stage_local as SL
from tests import stage_parity as SP

NGF, S, MAPS = 16, 128, ('face', 'offgrid', 'noclass')          # shape P of tests/test_hip_stage_local.py


# ---- operand model ---------------------------------------------------------------------------------------------------------------
def _values(n=200_000):
    """Seeded f32 values over 40 binades, with exact bf16 ties (both parities of the kept bit), values next to ties, zeros and signs."""
    rng = np.random.default_rng(11)
    x = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(np.float32)
    u = x.view(np.uint32).copy()
    u[: n // 4] = (u[: n // 4] & np.uint32(0xFFFF0000)) | np.uint32(0x8000)               # exact ties
    u[n // 4: n // 4 + 1000] = (u[n // 4: n // 4 + 1000] & np.uint32(0xFFFF0000)) | np.uint32(0x7FFF)
    u[n // 4 + 1000: n // 4 + 2000] = (u[n // 4 + 1000: n // 4 + 2000] & np.uint32(0xFFFF0000)) | np.uint32(0x8001)
    x = u.view(np.float32).copy()
    x[-4:] = (0.0, -0.0, 1.0, -1.0)
    return x


def test_round_operand_bf16_is_torch_bfloat16():
    x = _values()
    ties = (x.view(np.uint32) & np.uint32(0xFFFF)) == 0x8000
    assert len(x) >= 100_000 and ties.sum() >= 10_000
    want = torch.from_numpy(x).to(torch.bfloat16).to(torch.float32).numpy()
    got = SL.round_operand(x, 'bf16')
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    kept = (x.view(np.uint32)[ties] >> 16) & 1
    assert kept.min() == 0 and kept.max() == 1                  # ties to even were exercised in both directions
    assert SL.is_representable(got, 'bf16').all() and not SL.is_representable(x[~ties][:1000], 'bf16').all()


def test_round_operand_f16_is_the_hi_term_of_the_split():
    rng = np.random.default_rng(12)
    for mag in (1e-3, 0.07, 1.0, 37.0):
        w = (rng.standard_normal((64, 144)) * mag).astype(np.float32)
        s = E.row_scale(w)
        hi, lo = E.split(w, s)
        assert np.array_equal(SL.round_operand(w, 'f16', s).astype(np.float64) * s, hi)
        assert np.array_equal(SL.round_operand(w, 'f16x3', s).astype(np.float64) * s, hi + lo)
        assert SL.is_representable(SL.round_operand(w, 'f16', s), 'f16').all()
        assert not SL.is_representable(SL.round_operand(w, 'f16x3', s), 'f16').all()
    assert SL.round_operand(np.float32([1e9, -1e9]), 'f16').tolist() == [E.SH16_MAX, -E.SH16_MAX]          # saturation (MODE.FP16_OVFL)


def test_truncation_is_toward_zero_and_representable():
    x = _values(20_000)
    for fmt in ('f16', 'bf16'):
        t = SL.truncate_operand(x, fmt)
        assert SL.is_representable(t, fmt).all() and (np.abs(t) <= np.abs(x)).all() and (np.sign(t) * np.sign(x) >= 0).all()
        assert (np.abs(x - t) < np.abs(x) * 2.0 ** (1 - SL.SIG_BITS[fmt]) + 1e-45).all() and (t != SL.round_operand(x, fmt)).any()


def test_row_exponents_put_the_row_maximum_in_the_window():
    rng = np.random.default_rng(13)
    w = (rng.standard_normal((96, 40, 3, 3)) * np.exp2(rng.integers(-30, 10, (96, 1, 1, 1)))).astype(np.float32)
    w[5] = 0
    w[6] = np.float32(2.0 ** -3)                                 # a power of two: the lower end of the window
    k = SL.row_exponents(w)
    mx = np.abs(w.reshape(96, -1)).max(axis=1).astype(np.float64) * np.exp2(k.astype(np.float64))
    live = np.arange(96) != 5
    assert k[5] == 0 and (mx[live] >= 2.0 ** 14).all() and (mx[live] < 2.0 ** 15).all() and mx[6] == 2.0 ** 14
    assert all(E.row_scale(w[r]) == 2.0 ** k[r] for r in range(96) if r != 5)
    # shared exponents of a fused conv_1 / conv_s pair: one D for every row, no row above its own optimum
    k1, ks = rng.integers(10, 20, 32), rng.integers(8, 22, 32)
    n1, ns, D = SL.shared_exponents(k1, ks)
    assert (n1 - ns == D).all() and (n1 <= k1).all() and (ns <= ks).all() and ((n1 == k1) | (ns == ks)).all()


def test_spectral_weights_follow_the_loader_not_the_float64_oracle():
    """w / (float) sigma in f32: the float64 oracle's quotient, rounded to f32 afterwards, differs in some elements, and a few bf16 roundings flip."""
    from ctrlhair_amd import procedural as P
    from oracle import sean_oracle as O
    sd = P.sean_state_dict(0, NGF)
    mine = SL.spectral_f32(sd, 'up_0.conv_0')
    sd64 = O._cast_sd(O.to_torch(sd), torch.float64)
    theirs = O.spectral_weight(sd64, 'up_0.conv_0').numpy()
    assert mine.dtype == np.float32 and np.abs(mine - theirs).max() <= 2.0 ** -23 * np.abs(theirs).max()
    print(f'up_0.conv_0: {(mine != theirs.astype(np.float32)).mean():.3f} of the f32 quotients differ from the rounded f64 quotient')


def test_the_oracle_float64_conv_is_the_dense_conv():
    """oracle.sean_oracle._conv3x3 (float64, 64 input channels or more: nine shifted matrix products) against F.conv2d, with and without a bias;
    below 64 channels and in f32 it IS F.conv2d."""
    import torch.nn.functional as F
    from oracle import sean_oracle as O
    g = torch.Generator().manual_seed(5)
    for C, K, h, w_ in ((64, 24, 9, 13), (512, 48, 8, 8), (128, 6, 5, 7)):
        x, w, b = (torch.randn(s, generator=g, dtype=torch.float64) for s in ((2, C, h, w_), (K, C, 3, 3), (K,)))
        for bias in (b, None):
            want = F.conv2d(x, w, bias, padding=1)
            assert float((O._conv3x3(x, w, bias) - want).abs().max()) <= 1e-14 * float(want.abs().max())
    x, w, b = (torch.randn(s, generator=g) for s in ((2, 128, 6, 6), (8, 128, 3, 3), (8,)))
    assert torch.equal(O._conv3x3(x, w, b), F.conv2d(x, w, b, padding=1))
    assert torch.equal(O._conv3x3(x[:, :19].double(), w[:, :19].double(), None), F.conv2d(x[:, :19].double(), w[:, :19].double(), None, padding=1))


# ---- the model device ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def shape():
    from ctrlhair_amd import procedural as P
    sd = P.sean_state_dict(0, NGF)
    labels = SP.label_batch(S, MAPS)
    codes, noise = P.style_codes(len(MAPS), seed=71), P.noise_planes(len(MAPS), S, NGF, seed=72)
    shared, locs = {}, {}

    def local(fmt):
        if fmt not in locs:
            locs[fmt] = SL.Local(sd, labels, codes, noise, NGF, fmt, MAPS, shared=shared)
        return locs[fmt]
    return dict(sd=sd, local=local)


@pytest.mark.parametrize('fmt', SL.FORMATS)
def test_the_model_device_passes_every_bound(shape, fmt):
    loc = shape['local'](fmt)
    res = loc.check(SL.model_device(loc, shape['sd']))
    res.merge(loc.check(SL.model_device(loc, shape['sd'], folded=True), folded=True))
    res.merge(loc.check(SL.model_device(loc, shape['sd'], samples=[0]), samples=[0]))
    print(f'model device, {fmt}: worst E / bound = {res.worst[0]:.3f} at {res.worst[1]}, sample {res.worst[2]}; {res.table()}')
    assert res.failure is None, str(res.failure)
    assert set(res.by_type) == {'fc', '.hs', '.xs', '.h0', '.dx', '.h1', 'block', 'image'} and set(res.by_kind) == set(SP.KIND_NAMES)
    if fmt != 'f16x3':
        taps = SL.model_device(loc, shape['sd'], samples=[1])
        assert all(SL.is_representable(t.numpy(), fmt).all() for s, t in taps.items() if s[-3:] in ('.hs', '.h0', '.h1'))


# (fault, where, format, the one stage that must fail, sample): the sample is offgrid, whose 128-pixel level has every pixel kind
FAULTS = [
    ('trunc', 'up_2.conv_0', 'bf16', 'up_2.dx'),
    ('trunc', 'up_0.conv_s', 'f16', 'up_0.xs'),
    ('swap', 'up_3.conv_1', 'bf16', 'up_3'),
    ('swap', 'up_3.conv_0', 'f16', 'up_3.dx'),
    ('gamma', 'up_3.ace_1', 'bf16', 'up_3.h1'),
    ('gamma', 'up_3.ace_s', 'f16', 'up_3.hs'),
    ('noise', 'up_2.ace_0', 'f16', 'up_2.h0'),
    ('noise', 'up_3.ace_1', 'bf16', 'up_3.h1'),
    ('lo', 'up_1.h0', 'f16', 'up_1.dx'),
    ('lo', 'up_3.h0', 'f16', 'up_3.dx'),
]


@pytest.mark.parametrize('fault,where,fmt,stage', FAULTS)
def test_a_planted_fault_fails_its_own_stage_and_no_other(shape, fault, where, fmt, stage):
    loc = shape['local'](fmt)
    taps = SL.model_device(loc, shape['sd'], samples=[1], faults={fault: where})
    res = loc.check(taps, samples=[1])
    print(f'{fault} at {where}, {fmt}: {res.failure}')
    assert res.failure is not None and res.failed_stages == [stage], (res.failed_stages, str(res.failure))
    f = res.failure
    assert f.stage == stage and f.sample == 1 and f.map == 'offgrid' and f.kind in SP.KIND_NAMES and f.E > f.bound
    if fault == 'swap':
        assert f.y < 64 + 1                                       # the first 64 output rows
    if fault == 'gamma':
        assert f.x == S - 1 and f.kind in ('frame', 'boundary-conv')
        assert all(v <= f.bound for k, v in f.by_kind.items() if k in ('interior', 'straight-edge'))
    if fault == 'lo':                                            # planted alone, the same fault is not an f16 operand
        assert not SL.is_representable(taps[where].numpy(), 'f16').all()
        clean = SL.model_device(loc, shape['sd'], samples=[1])
        assert SL.is_representable(clean[where].numpy(), 'f16').all()
