"""GPU tests of the per-chunk level plan (ctrlhair_amd/csrc/sean_model.cpp Runner::plan_aces, LevelPlan, Runner::prepare): what a chunk
classifies, lists and launches for a resolution level is decided from (B, S) and the options of THIS call alone, so nothing of an earlier
call on the same handle may show in a later one.  Every assertion is torch.equal against a fresh handle of the same geometry that makes
only that call.  ngf = 16.

Sizes: S = 256, 128 and 64 put two, one and zero gather-route levels above the F(4x4) and dense levels (128 and 256 are the smallest sizes
that do); B = max_batch + 1 runs in two chunks, the second of one sample."""
import pytest
import torch

pytestmark = pytest.mark.gpu
NGF = 16
# name -> (sean.f16x3, options, max_batch)
HANDLES = {'run_ahead': (0, {}, 2),
           'prologue_grouped_luts': (0, {'sean.ahead': 0}, 4),
           'direct_sparse': (0, {'sean.ahead': 0, 'sean.wino': 0}, 3),
           'f16x3': (1, {}, 2)}
MAX_SIZE = 256


def _gen(f16x3, options, mb):
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.sean.generator import SeanGenerator
    return SeanGenerator(0, f16x3=f16x3, options=options).load_state_dict(P.sean_state_dict(0, NGF), max_batch=mb, max_size=MAX_SIZE)


def _run(gen, B, S):
    from ctrlhair_amd import procedural as P
    dev = gen.device
    out = gen.generate(torch.from_numpy(P.blocky_labels(B, S, grid=8, seed=11 + S)).to(dev), torch.from_numpy(P.style_codes(B, seed=22 + S)).to(dev),
                       torch.from_numpy(P.noise_planes(B, S, NGF, seed=33 + S)).to(dev))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out


def _fresh(f16x3, options, mb, B, S):
    g = _gen(f16x3, options, mb)
    try:
        return _run(g, B, S)
    finally:
        g.handle.close()


@pytest.mark.parametrize('name', list(HANDLES))
def test_one_handle_many_sizes(hip_lib, name):
    f16x3, options, mb = HANDLES[name]
    calls = [(mb, 256), (1, 128), (mb + 1, 64), (mb, 256)]
    ref = {c: _fresh(f16x3, options, mb, *c) for c in set(calls)}
    g = _gen(f16x3, options, mb)
    try:
        for i, c in enumerate(calls):
            out = _run(g, *c)
            assert torch.equal(out, ref[c]), f'{name}: call {i} (B, S) = {c}: max |reused - fresh| = {float((out - ref[c]).abs().max()):.3e}'
    finally:
        g.handle.close()


def test_live_options_are_read_per_call(hip_lib):
    """sean.sparse 1 -> 0 -> 1, then sean.hidden_wq 1 -> 0, between calls at (3, 256) on one exact-f32 handle beyond the run-ahead sizes"""
    base, mb, call = {'sean.ahead': 0}, 3, (3, 256)
    ref = {key: _fresh(0, dict(base, **dict(key)), mb, *call) for key in ((), (('sean.sparse', 0),), (('sean.hidden_wq', 0),))}
    g = _gen(0, base, mb)
    try:
        for step, (opt, val, key) in enumerate([(None, 0, ()), ('sean.sparse', 0, (('sean.sparse', 0),)), ('sean.sparse', 1, ()),
                                                ('sean.hidden_wq', 0, (('sean.hidden_wq', 0),))]):
            if opt:
                g.handle.set_option(opt, val)
            out = _run(g, *call)
            assert torch.equal(out, ref[key]), f'step {step} ({opt} = {val}): max |live - fresh| = {float((out - ref[key]).abs().max()):.3e}'
    finally:
        g.handle.close()
