"""GPU tests: every tapped stage of the single-term f16 (sean.f16x3 = 2) and bf16 (= 3) SEAN generator paths, and of f16x3 (= 1) as the control,
against a float64 reference of THAT STAGE ALONE, computed from the device's own taps of the stage's inputs (tests/stage_local.py).  The taps
'.hs' / '.h0' / '.h1' are the decoded stored operand planes, so a conv stage sums exact products of known f16 / bf16 numbers in f32 and is held
to an f32-class bound on every path; an ACE stage is held to the local effect of its format:

    tight ('fc', '.xs', '.dx', '<block>', 'image'):   E <= 4 * E32_local
    wide  ('.hs', '.h0', '.h1'):                      E <= 4 * (E32_local + Eq_local) + u * peak,   u = 2^-11 (f16), 2^-8 (bf16), 0 (f16x3)

with E(x) = max |x[b] - ref[b]| / rms(ref[b]); nothing measured from the library enters a bound, and a fault in stage s fails stage s and no later
one.  The assertion message names the first stage over its bound, the sample's label map, the (c, y, x) of the worst element and its pixel kind.

Shapes: P = ngf 16, S 128, maps face / offgrid / noclass in one call of three (levels 4 .. 128: the 8x8x8, 16x16x2 and 32x16 tiles, each with a
partial batch tile); Q = ngf 24, S 160, maps offgrid / band255, uncalibrated weights (24 and 48 channels: no multiple of the 16-channel k-chunk;
partial tiles at every level; a second, partly filled 128-pixel block column).
P6 and Q4 are P and Q with six / four samples in the call (P6 adds band255 / ring3 / one_region, Q4 face / noclass): see the fused accumulator below.
Paths: f16, bf16 and f16x3 with default options, and each again with sean.dbg 64 ('+ws').  With default options P and Q stay below the 512 tiles
from which an ACE takes the wave-specialised kernel (conv_sh16.h sh16_ace_uses_ws): every ACE runs dense (measured: 0 interior launches, executed =
dense FLOPs).  sean.dbg 64 forces that kernel, so the '+ws' paths are where the tile lists, the compacting kernel and the single / bf16 legs of the
interior pass run at these sizes (6 interior launches; 2.89e10 of 4.19e10 dense FLOPs on P, 3.59e10 of 6.68e10 on Q).  The bit also asks
dispatch_sh16_plain for the wave-specialised PLAIN kernel, but at P and Q every ResBlock conv is a split-K candidate (mtiles_hint_small), which vetoes
it: of the wave-specialised kernels only the ACE one and its compacting form are reached here, not the plain one.
Per path, on P and Q: one run with every tap, one with every tap but the '.xs' ones, sample 0 of P alone through a max_batch 1 handle; every '.hs' /
'.h0' / '.h1' tap of f16 and bf16 must hold numbers of 11 / 8 significant bits (what the conv reads); on the '+ws' paths the sparse routes must have run.
The fused conv_1 + shortcut accumulator: the library adds conv_s into conv_1's accumulator only where no '.xs' tap is set AND the level has 32 pixels
or more AND ceil(Cout / 64) * ceil(B r^2 / 512) >= 192 (can_fuse_1x1).  P and Q never get there (at most 96 / 100, at up_3), so their run without
the '.xs' taps is the unfused sum once more -- asserted: 18 conv launches.  P6 and Q4 reach 192 / 200 at up_3; there the route is asserted (17 conv
launches) and the tight stages of the run without '.xs' taps go against their bounds on f16, bf16 and f16x3.

Measured worst E(hip) / bound per path, shape and stage type, and per pixel kind of the stage's level (MI355X; 1.0 = at the bound; both runs):
    path       shape           fc      .hs     .xs     .h0     .dx     .h1     block   image   interior  str-edge  frame   bnd-conv
    f16        P               0.353   0.438   0.176   0.568   0.288   0.445   0.214   0.154   0.408     0.445     0.247   0.568
    bf16       P               0.353   0.459   0.293   0.452   0.549   0.435   0.472   0.169   0.447     0.472     0.308   0.549
    f16x3      P               0.353   0.445   0.195   0.421   0.505   0.713   0.404   0.190   0.713     0.713     0.462   0.595
    f16+ws     P               0.353   0.438   0.176   0.568   0.262   0.445   0.214   0.164   0.408     0.445     0.247   0.568
    bf16+ws    P               0.353   0.459   0.293   0.452   0.606   0.435   0.472   0.138   0.452     0.476     0.355   0.606
    f16x3+ws   P               0.353   0.445   0.180   0.407   0.506   0.609   0.404   0.180   0.506     0.399     0.440   0.609
    f16        Q               0.241   0.336   0.169   0.511   0.289   0.428   0.326   0.197   0.511     0.428     0.314   0.499
    bf16       Q               0.241   0.366   0.312   0.549   0.536   0.406   0.893   0.190   0.893     0.464     0.476   0.678
    f16x3      Q               0.241   0.690   0.244   0.682   0.523   0.879   0.546   0.259   0.879     0.736     0.611   0.864
    f16+ws     Q               0.241   0.374   0.169   0.511   0.298   0.447   0.326   0.201   0.511     0.447     0.314   0.499
    bf16+ws    Q               0.241   0.500   0.312   0.533   0.552   0.444   0.893   0.189   0.893     0.464     0.498   0.678
    f16x3+ws   Q               0.241   0.631   0.209   0.655   0.523   0.822   0.546   0.171   0.546     0.500     0.605   0.822
    f16        P, max_batch 1  0.287   0.438   0.113   0.568   0.217   0.380   0.198   0.112   0.385     0.230     0.247   0.568
    bf16       P, max_batch 1  0.287   0.459   0.198   0.442   0.549   0.435   0.437   0.110   0.447     0.432     0.308   0.549
    f16x3      P, max_batch 1  0.287   0.445   0.195   0.360   0.505   0.582   0.404   0.113   0.582     0.443     0.279   0.540
    f16+ws     P, max_batch 1  0.287   0.438   0.112   0.568   0.212   0.380   0.198   0.099   0.385     0.249     0.247   0.568
    bf16+ws    P, max_batch 1  0.287   0.459   0.192   0.442   0.606   0.435   0.370   0.090   0.452     0.476     0.355   0.606
    f16x3+ws   P, max_batch 1  0.287   0.445   0.180   0.360   0.503   0.554   0.404   0.095   0.408     0.285     0.284   0.554
Fused accumulator, tight stages of the run without '.xs' taps (17 conv launches each):   fc      .dx     block   image
    f16 / bf16 / f16x3   P6    0.353 / 0.353 / 0.353   0.306 / 0.489 / 0.559   0.224 / 0.400 / 0.418   0.181 / 0.163 / 0.190
    f16 / bf16 / f16x3   Q4    0.241 / 0.241 / 0.241   0.343 / 0.700 / 0.573   0.236 / 0.388 / 0.413   0.223 / 0.198 / 0.201
No pixel kind sits apart from the others on any path.  The ratios above 0.8, both on Q (uncalibrated weights) and both a matter of association, not of
the format: bf16 'up_1' (0.893, run with every tap: xs_dev + conv_1 over 96 channels x 9 taps at 40 pixels) and f16x3 'up_3.h1' (0.822 .. 0.879: the
SPADE conv over 128 channels x 9 taps).  E32_local is PyTorch's blocked f32 conv; a strictly sequential f32 chain of the same exact bf16 products
over 96 channels x 9 taps has E = 1.10 x (4 E32) on N(0, 1) data, of 128 x 9 f16x3 operand pairs 1.37 x, while the lo x lo products f16x3 drops
account for 0.05 x -- the matrix cores' chains of 16-product steps lie between PyTorch's and the sequential one.
The f16 tap defect was real: with a decode that adds the lo plane whenever the path is not bf16 (the library before this module came), every element of every
'.hs' / '.h0' / '.h1' tap of f16 failed is_representable on both shapes -- every writer of that path, not only the interior pass, leaves a lo plane behind
that the single-term conv never reads -- and every tight stage behind an ACE failed: '.xs' at 333 x, '.dx' at 246 x, '<block>' at 279 x its bound
(head_0.dx: E 9.3e-4 against 4.1e-6), bf16 and f16x3 passing; with sh16_decode reading the hi plane alone on the single-term paths, the table above.
Measured time of the module on an MI355X host (references on 16 CPU threads): 75 s in one process -- the first test of each (shape, format) builds the
weights and evaluates that format's float64 and f32 modulation of all 18 ACEs (3.8 to 9.0 s; f16 comes first and also pays the unrounded float64
one that the formats share), every other test 0.3 to 2.9 s.
"""
import time

import numpy as np
import pytest
import torch

from tests import stage_local as SL
from tests import stage_parity as SP

pytestmark = pytest.mark.gpu

SHAPES = {
    'P': dict(ngf=16, S=128, maps=('face', 'offgrid', 'noclass'), calibrated=True),
    'Q': dict(ngf=24, S=160, maps=('offgrid', 'band255'), calibrated=False),
    # the same two with more samples in the call: enough 512-pixel tiles at the top level for the library to add conv_s into conv_1's accumulator
    'P6': dict(ngf=16, S=128, maps=('face', 'offgrid', 'noclass', 'band255', 'ring3', 'one_region'), calibrated=True),
    'Q4': dict(ngf=24, S=160, maps=('offgrid', 'band255', 'face', 'noclass'), calibrated=False),
}
MAIN, FOLD = ('P', 'Q'), ('P6', 'Q4')
# path: (format of stage_local, sean.f16x3, options set after ch_finalize).  With default options shapes P and Q stay below the 512 tiles from which
# an ACE takes the wave-specialised kernel (conv_sh16.h sh16_ace_uses_ws), and with it the tile lists, the compacting kernel and the interior pass:
# every ACE runs dense.  sean.dbg 64 forces the wave-specialised kernel -- in dispatch_sh16_ace, which is what the '+ws' paths are for, and also in
# dispatch_sh16_plain, where it changes nothing at P and Q: every ResBlock conv there is a split-K candidate (mtiles_hint_small), which vetoes it.
PATHS = {'f16': ('f16', 2, {}), 'bf16': ('bf16', 3, {}), 'f16x3': ('f16x3', 1, {}),
         'f16+ws': ('f16', 2, {'sean.dbg': 64}), 'bf16+ws': ('bf16', 3, {'sean.dbg': 64}), 'f16x3+ws': ('f16x3', 1, {'sean.dbg': 64})}
SINGLE = [p for p in PATHS if PATHS[p][0] != 'f16x3']
_shapes = {}
DEVICE = 0


@pytest.fixture(scope='module', autouse=True)
def _free_references():
    yield
    _shapes.clear()
    torch.cuda.empty_cache()


def _shape(name):
    if name not in _shapes:
        from ctrlhair_amd import procedural as P
        cfg = SHAPES[name]
        ngf, S, maps = cfg['ngf'], cfg['S'], cfg['maps']
        _shapes[name] = dict(cfg, sd=P.sean_state_dict(0, ngf, calibrated=cfg['calibrated']), labels=SP.label_batch(S, maps),
                             codes=P.style_codes(len(maps), seed=71), noise=P.noise_planes(len(maps), S, ngf, seed=72), shared={}, local={})
    return _shapes[name]


def _local(sh, path):
    """The local references of a shape and path (built once per module; the modulation of every ACE is evaluated at its first check)."""
    fmt = PATHS[path][0]
    if fmt not in sh['local']:
        sh['local'][fmt] = SL.Local(sh['sd'], sh['labels'], sh['codes'], sh['noise'], sh['ngf'], fmt, sh['maps'], shared=sh['shared'])
    return sh['local'][fmt]


def _gen(sh, path, max_batch):
    from ctrlhair_amd.sean.generator import SeanGenerator
    gen = SeanGenerator(DEVICE, f16x3=PATHS[path][1]).load_state_dict(sh['sd'], max_batch=max_batch, max_size=sh['S'])
    for k, v in PATHS[path][2].items():
        gen.handle.set_option(k, v)
    return gen


def _render(gen, sh, loc, samples, folded):
    """One generate() call on the samples with a tap on every stage (but the '.xs' ones when folded): {stage: CPU tensor}, the image under IMAGE."""
    from ctrlhair_amd.sean import arch
    dev, idx = gen.device, list(samples)
    shapes = {'fc': (16 * sh['ngf'], sh['S'] // 32)}
    for b in arch.blocks(sh['ngf']):
        r = sh['S'] // b.res_div
        shapes.update({b.name + '.hs': (b.fin, r), b.name + '.xs': (b.fout, r), b.name + '.h0': (b.fin, r), b.name + '.dx': (b.fmid, r),
                       b.name + '.h1': (b.fmid, r), b.name: (b.fout, r)})
    stages = [s for s, _, typ in loc.stages if s != SL.IMAGE and not (folded and typ == '.xs')]
    bufs = {s: torch.full((len(idx), shapes[s][0], shapes[s][1], shapes[s][1]), float('nan'), dtype=torch.float32, device=dev) for s in stages}
    for s, t in bufs.items():
        gen.handle.sean_set_tap(s, t.data_ptr())
    try:
        img = gen.generate(torch.from_numpy(sh['labels'][idx]).to(dev), torch.from_numpy(sh['codes'][idx]).to(dev), torch.from_numpy(sh['noise'][idx]).to(dev))
        torch.cuda.synchronize()
    finally:
        for s in bufs:
            gen.handle.sean_set_tap(s, None)
    out = {s: t.cpu() for s, t in bufs.items()}
    out[SL.IMAGE] = img.cpu()
    return out


def _report(tag, res):
    print(f'{tag}: worst E / bound = {res.worst[0]:.3f} at {res.worst[1]}, sample {res.worst[2]}; {res.table()}')


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('shape', MAIN)
def test_every_stage_against_its_local_float64_reference(hip_lib, shape, path):
    sh = _shape(shape)
    loc, n = _local(sh, path), len(sh['maps'])
    t0 = time.time()
    gen = _gen(sh, path, n)
    try:
        res = SL.Result()
        for folded in (False, True):
            r = loc.check(_render(gen, sh, loc, range(n), folded), folded=folded)
            _report(f'shape {shape}, {path}, {"every tap but .xs" if folded else "every tap"}', r)
            res.merge(r)
    finally:
        gen.handle.close()
    print(f'shape {shape}, {path}: {time.time() - t0:.1f} s')
    assert res.failure is None, f'shape {shape}, {path}: {res.failure}; stages over their bound: {res.failed_stages}'


@pytest.mark.parametrize('path', list(PATHS))
def test_one_sample_through_a_max_batch_1_handle(hip_lib, path):
    sh = _shape('P')
    loc = _local(sh, path)
    gen = _gen(sh, path, 1)
    try:
        res = loc.check(_render(gen, sh, loc, [0], False), samples=[0])
        res.merge(loc.check(_render(gen, sh, loc, [0], True), samples=[0], folded=True))
    finally:
        gen.handle.close()
    _report(f'shape P, {path}, sample 0 alone (max_batch 1)', res)
    assert res.failure is None, f'shape P, {path}, max_batch 1: {res.failure}; stages over their bound: {res.failed_stages}'


@pytest.mark.parametrize('path', SINGLE)
@pytest.mark.parametrize('shape', MAIN)
def test_the_tapped_operands_are_what_the_conv_reads(hip_lib, shape, path):
    """Every '.hs' / '.h0' / '.h1' tap of a single-term path holds numbers of 11 (f16) / 8 (bf16) significant bits: the decoded hi plane alone.  (A
    decode that adds the lo plane shows hi + lo on f16 -- every ACE kernel but the single-term interior pass writes a lo plane, and where that pass
    does not, the plane holds whatever it held before -- which is not the operand of the conv that follows: measured, every element.)"""
    sh = _shape(shape)
    loc, n = _local(sh, path), len(sh['maps'])
    gen = _gen(sh, path, n)
    try:
        taps = _render(gen, sh, loc, range(n), False)
    finally:
        gen.handle.close()
    bad = {}
    for s, _, typ in loc.stages:
        if typ in ('.hs', '.h0', '.h1'):
            ok = SL.is_representable(taps[s].numpy(), PATHS[path][0])
            if not ok.all():
                b, c, y, x = np.argwhere(~ok)[0]
                kinds = loc.kinds(int(b), ok.shape[-1])
                per = ', '.join(f'{SP.KIND_NAMES[k]} {(~ok)[b][:, kinds == k].mean():.3f}' for k in range(4) if (kinds == k).any())
                bad[s] = (f'{(~ok).mean():.3f} of the elements, first at sample {b} (c, y, x) = ({c}, {y}, {x}), a {SP.KIND_NAMES[kinds[y, x]]} pixel; '
                          f'share of that sample per kind: {per}')
    assert not bad, f'shape {shape}, {path}: taps that are no {PATHS[path][0]} operands: {bad}'


def fused_blocks(ngf, S, B):
    """The learned-shortcut blocks whose conv_s the library adds into conv_1's accumulator when no '.xs' tap is set (sean_model.cpp can_fuse_1x1,
    restated): a level of 32 pixels or more with at least 192 (64-row tile, 512-pixel tile) pairs -- below that conv_1 is a split-K candidate."""
    from ctrlhair_amd.sean import arch
    return [b.name for b in arch.blocks(ngf) if b.learned_shortcut and S // b.res_div >= 32 and
            ((b.fout + 63) // 64) * ((B * (S // b.res_div) ** 2 + 511) // 512) >= 192]


def _conv_launches(gen, sh):
    """Launches of ResBlock convs (profile kind 0) of one call on every sample with no tap set: 14, plus one per conv_s that runs on its own."""
    dev = gen.device
    gen.handle.profile_enable(True)
    gen.generate(torch.from_numpy(sh['labels']).to(dev), torch.from_numpy(sh['codes']).to(dev), torch.from_numpy(sh['noise']).to(dev))
    torch.cuda.synchronize()
    gen.handle.profile_enable(False)
    n = gen.handle.profile_read(0)['launches']
    gen.handle.profile_read(-1)
    return n


@pytest.mark.parametrize('path', ['f16', 'bf16', 'f16x3'])
@pytest.mark.parametrize('shape', FOLD)
def test_the_fused_shortcut_accumulator(hip_lib, shape, path):
    """Shapes P6 / Q4: with no '.xs' tap the top block (up_3: 16 / 24 output channels, conv_s over 32 / 48 channels, conv_1 over 16 / 24 -- at Q4
    one and a half k-chunks) runs conv_1 and conv_s on one accumulator (conv_sh16_kernel<..., FUSE>, TERMS 1 / 2 / 3).  The route is asserted, not
    assumed: one conv launch fewer than the 18 of the unfused forward, and the restated rule names the block.  Then every tight stage of the run
    with every tap but the '.xs' ones goes against its bound (the block as conv_s(hs_dev) + conv_1(h1_dev) + bias); the ACE stages of these
    batches add no kernel to those of P and Q and are left to them."""
    sh = _shape(shape)
    loc, n = _local(sh, path), len(sh['maps'])
    fused = fused_blocks(sh['ngf'], sh['S'], n)
    assert fused == ['up_3'], fused
    gen = _gen(sh, path, n)
    try:
        launches = _conv_launches(gen, sh)
        res = loc.check(_render(gen, sh, loc, range(n), True), folded=True, only=SL.TIGHT)
    finally:
        gen.handle.close()
    _report(f'shape {shape}, {path}, every tap but .xs, tight stages ({launches} conv launches)', res)
    assert launches == 18 - len(fused), launches
    assert res.failure is None, f'shape {shape}, {path}: {res.failure}; stages over their bound: {res.failed_stages}'


@pytest.mark.parametrize('path', [p for p in PATHS if p.endswith('+ws')])
@pytest.mark.parametrize('shape', MAIN)
def test_the_sparse_routes_ran(hip_lib, shape, path):
    """On the '+ws' paths the interior pass (profile kind 3) and the SPADE boundary conv (kind 1) launched, and fewer FLOPs were executed than the
    dense evaluation has: a silent fall-back to dense must not pass as covered.  (With default options both shapes are below the library's 512-tile
    rule and run every ACE dense -- 0 interior launches, executed = dense FLOPs, measured -- which is why the '+ws' paths exist.)"""
    sh = _shape(shape)
    loc, n = _local(sh, path), len(sh['maps'])
    gen = _gen(sh, path, n)
    try:
        gen.handle.profile_enable(True)
        dev = gen.device
        gen.generate(torch.from_numpy(sh['labels']).to(dev), torch.from_numpy(sh['codes']).to(dev), torch.from_numpy(sh['noise']).to(dev))
        torch.cuda.synchronize()
        gen.handle.profile_enable(False)
        interior, conv, plain = gen.handle.profile_read(3), gen.handle.profile_read(1), gen.handle.profile_read(0)
        everything = gen.handle.profile_read(-1)
    finally:
        gen.handle.close()
    print(f'shape {shape}, {path}: interior launches {interior["launches"]}, SPADE conv launches {conv["launches"]}, FLOPs executed '
          f'{everything["flops_executed"]:.3e} of {everything["flops"]:.3e} dense')
    assert interior['launches'] > 0 and conv['launches'] > 0
    assert fused_blocks(sh['ngf'], sh['S'], n) == [] and plain['launches'] == 18          # P and Q: no conv_s is folded (see FOLD)
    assert conv['flops_executed'] < conv['flops'] and everything['flops_executed'] < everything['flops']
