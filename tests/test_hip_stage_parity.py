"""GPU tests: every tapped stage of the SEAN generator against the float64 oracle at the levels of 128 pixels and more, where the four-pixel
interior pass, the straight-edge and frame table rows, the boundary-quad gather conv (hidden-activation planes and pre-gathered patches), the
F(4x4,3x3) plain / split / V routes and the pointwise shortcut conv run.  Metric, bound and checker: tests/stage_parity.py --

    E(x) = max |x[b] - ref64[b]| / rms(ref64[b]) <= 4 * (E32(stage, b) + e4 * uses_f4)

with E32 the PyTorch f32 oracle's own E against the float64 run and e4 the f32 model of one F(4x4,3x3) conv at the widest F(4x4) layer of the
shape; nothing measured from the library enters the bound.  The assertion message names the first stage over its bound, the sample's label map,
the (c, y, x) of the worst element and its pixel kind (interior / straight-edge / frame / boundary-conv).

Shapes: A = ngf 64, S 128, the nine label maps of stage_parity.MAP_NAMES in one batch (levels 4 .. 128; 128 and 64 channels at the top level);
B = ngf 24, S 160, maps face / offgrid / noclass, uncalibrated weights (levels 5 .. 160: a second, partly filled 128-pixel block column, only the top
level on the 32 grid); C = ngf 16, S 256, offgrid alone (a styled 128-pixel level -- the style-LUT column / row sums of the table rows -- and a
256-pixel level of two full block columns).
Paths: exact-f32 defaults, sean.batch_invariant = 1 (uses_f4 = 1), sean.wino = 1, sean.wino = 0, f16x3 defaults, f16x3 with sean.dbg 64
(uses_f4 = 0).  Each path runs twice: with every tap, and with the block outputs alone (a tap on '<block>.xs' keeps the 1x1 shortcut conv from being
folded into conv_1; the second run takes the folded route).  On the exact-f32 default path the same samples also go two at a time through a
max_batch 2 handle and one at a time through a max_batch 1 handle (GEMV LUT route, tiny-level split-K, full run-ahead, the task-count rule).

Measured worst E(hip) / bound per path and shape (MI355X; 1.0 = at the bound):
    path                      A       B       C
    f32 (defaults)            0.312   0.101   0.065
    sean.batch_invariant = 1  0.429   0.206   0.309
    sean.wino = 1             0.640   0.758   0.379
    sean.wino = 0             0.678   0.758   0.416
    f16x3                     0.634   0.522   0.344
    f16x3, sean.dbg 64        0.634   0.522   0.388
    f32, max_batch 2          0.050   0.101   -
    f32, max_batch 1          0.050   0.101   -
(shape A in one call of nine takes F(4x4,3x3) from 32 pixels on; two samples or one at a time stay below its task-count rule: F(2x2,3x3), hence 0.05.)
(e4 at the widest layer that can take F(4x4,3x3), stage_parity.f4_channels: 512 channels for A, 48 for B -- only its 160-pixel level is on the
32 grid --, 256 for C.)
No stage of any path exceeded its bound (the closest: 0.76 of it), so none needed investigation.  As a check of the check, a frame-row beta off by 1e-4
(planted by hand in ace_edge_table, not kept) fails shape A at up_3.xs (f32: E 2.7e-4 > 2.3e-4) and up_3.hs (sean.wino = 1: 8.6e-5 > 2.5e-5) and
shape C at up_2.xs, each time on a frame pixel with the other kinds below 1e-5; the paths without frame rows (sean.wino = 0, f16x3) still pass.
Measured time of the module on an MI355X host (the oracle on 16 CPU threads): 54 s in one process -- shape A 33 s (oracle pair 12 s, first test 14 s with it, f16x3 handles 5 s each,
the others 1 to 2 s), shape B 12 s, shape C 8 s.
"""
import time

import pytest
import torch

from tests import stage_parity as SP

pytestmark = pytest.mark.gpu

SHAPES = {
    'A': dict(ngf=64, S=128, maps=SP.MAP_NAMES, calibrated=True),
    'B': dict(ngf=24, S=160, maps=('face', 'offgrid', 'noclass'), calibrated=False),
    'C': dict(ngf=16, S=256, maps=('offgrid',), calibrated=True),
}
# path: (sean.f16x3, options before ch_finalize, options after it, uses_f4)
PATHS = {
    'f32': (0, {}, {}, 1),
    'batch_invariant': (0, {'sean.batch_invariant': 1}, {}, 1),
    'wino1': (0, {'sean.wino': 1}, {}, 0),
    'wino0': (0, {'sean.wino': 0}, {}, 0),
    'f16x3': (1, {}, {}, 0),
    'f16x3ws': (1, {}, {'sean.dbg': 64}, 0),
}
_shapes = {}
DEVICE = 0                   # the handles, the inputs and the references all live here


@pytest.fixture(scope='module', autouse=True)
def _free_references():
    yield
    _shapes.clear()          # the references live on the device
    torch.cuda.empty_cache()


def _shape(name):
    """Inputs, the oracle pair (run once per module) and the Reference of a shape, on the device."""
    if name not in _shapes:
        from ctrlhair_amd import procedural as P
        cfg = SHAPES[name]
        ngf, S, maps = cfg['ngf'], cfg['S'], cfg['maps']
        t0 = time.time()
        sd = P.sean_state_dict(0, ngf, calibrated=cfg['calibrated'])
        labels = SP.label_batch(S, maps)
        codes, noise = P.style_codes(len(maps), seed=71), P.noise_planes(len(maps), S, ngf, seed=72)
        t64, t32 = SP.oracle_pair(sd, labels, codes, noise, ngf)
        ref = SP.Reference(t64, t32, labels, maps, device=torch.device('cuda', DEVICE))
        del t64, t32
        e4 = SP.e4(SP.f4_channels(ngf, S))
        print(f'shape {name}: oracle pair and reference in {time.time() - t0:.1f} s; e4({SP.f4_channels(ngf, S)}) = {e4:.2e}; '
              f'E32 up to {max(float(v.max()) for v in ref.E32.values()):.2e}')
        _shapes[name] = dict(cfg, sd=sd, labels=labels, codes=codes, noise=noise, ref=ref, e4=e4)
    return _shapes[name]


def _gen(sh, path, max_batch):
    from ctrlhair_amd.sean.generator import SeanGenerator
    f16x3, before, after, _ = PATHS[path]
    gen = SeanGenerator(DEVICE, f16x3=f16x3, options=before).load_state_dict(sh['sd'], max_batch=max_batch, max_size=sh['S'])
    for k, v in after.items():
        gen.handle.set_option(k, v)
    return gen


def _render(gen, sh, samples, stages):
    """One generate() call on the samples `samples` with taps on `stages`: {stage: device tensor}, the image under SP.IMAGE."""
    dev, ref = gen.device, sh['ref']
    idx = list(samples)
    bufs = {s: torch.full((len(idx),) + tuple(ref.ref[s].shape[1:]), float('nan'), dtype=torch.float32, device=dev) for s in stages if s != SP.IMAGE}
    for s, t in bufs.items():
        gen.handle.sean_set_tap(s, t.data_ptr())
    try:
        img = gen.generate(torch.from_numpy(sh['labels'][idx]).to(dev), torch.from_numpy(sh['codes'][idx]).to(dev), torch.from_numpy(sh['noise'][idx]).to(dev))
        torch.cuda.synchronize()
    finally:
        for s in bufs:
            gen.handle.sean_set_tap(s, None)
    bufs[SP.IMAGE] = img
    return bufs


def _check(gen, sh, path, groups, tag):
    """Both runs (all taps; block outputs alone) of every group of samples against the bound of the path; the worst E / bound is printed."""
    from ctrlhair_amd.sean import arch
    ref = sh['ref']
    e4_term = sh['e4'] * PATHS[path][3]
    outputs = [b.name for b in arch.blocks(sh['ngf'])] + [SP.IMAGE]
    worst = (0.0, '', -1)
    for stages in (ref.stages, outputs):
        for g in groups:
            got = _render(gen, sh, g, stages)
            failure, w = ref.check(got, e4_term, samples=g, stages=stages)
            assert failure is None, f'{tag} ({"all taps" if stages is ref.stages else "block outputs only"}): {failure}'
            worst = max(worst, w)
    print(f'{tag}: worst E / bound = {worst[0]:.3f} at {worst[1]}, sample {worst[2]} ({ref.map_names[worst[2]]})')


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_every_stage_against_the_float64_oracle(hip_lib, shape, path):
    sh = _shape(shape)
    n = len(sh['maps'])
    gen = _gen(sh, path, n)
    try:
        _check(gen, sh, path, [range(n)], f'shape {shape}, {path}')
    finally:
        gen.handle.close()


@pytest.mark.parametrize('max_batch', [2, 1])
@pytest.mark.parametrize('shape', ['A', 'B'])
def test_call_size(hip_lib, shape, max_batch):
    """The exact-f32 default path through a max_batch 2 handle two samples at a time and through a max_batch 1 handle one at a time: same bounds."""
    sh = _shape(shape)
    n = len(sh['maps'])
    gen = _gen(sh, 'f32', max_batch)
    try:
        _check(gen, sh, 'f32', [range(i, min(i + max_batch, n)) for i in range(0, n, max_batch)], f'shape {shape}, f32, max_batch {max_batch}')
    finally:
        gen.handle.close()


@pytest.mark.parametrize('path', ['f32', 'wino1'])
@pytest.mark.parametrize('shape', ['A', 'B'])
def test_the_sparse_routes_ran(hip_lib, shape, path):
    """The default path must have taken the routes this module is about: launches of the interior pass (profile kind 3) and of the SPADE boundary
    conv (kind 1), and fewer executed FLOPs than the dense evaluation -- a silent fall-back to dense must not pass as covered.  Likewise
    sean.wino = 1: its bound has no F(4x4) term, so it is the path on which the table rows and the interior pass are checked several times closer."""
    sh = _shape(shape)
    n = len(sh['maps'])
    gen = _gen(sh, path, n)
    try:
        gen.handle.profile_enable(True)
        _render(gen, sh, range(n), [SP.IMAGE])
        gen.handle.profile_enable(False)
        interior, conv, everything = gen.handle.profile_read(3), gen.handle.profile_read(1), gen.handle.profile_read(-1)
    finally:
        gen.handle.close()
    print(f'shape {shape}, {path}: interior launches {interior["launches"]}, SPADE conv launches {conv["launches"]}, FLOPs executed '
          f'{everything["flops_executed"]:.3e} of {everything["flops"]:.3e} dense')
    assert interior['launches'] > 0 and conv['launches'] > 0
    assert conv['flops_executed'] < conv['flops'] and everything['flops_executed'] < everything['flops']
