"""CPU tests of tests/stage_parity.py: the label maps give every pixel kind of the 128-pixel routes, the oracle's dtype argument, the
F(4x4,3x3) rounding model, and the power of the checker -- a planted error of 1e-4 of a stage's rms, which the image-level 1e-3 cannot
see, fails at its stage with its pixel kind.  No GPU, no library."""
import numpy as np
import pytest
import torch

from tests import stage_parity as SP

S = 128


@pytest.fixture(scope='module')
def kinds():
    """{map: (kind, code)} at the 128-pixel level."""
    return {n: SP.pixel_kinds(SP.label_map(n, S)) for n in SP.MAP_NAMES}


# ---- label maps ------------------------------------------------------------------------------------------------------------------
def test_pixel_kinds_follow_the_definition():
    """The vectorised classification against a pixel-by-pixel restatement of ace_sparse.h on crops that hold every kind (a crop is an image of its
    own: its frame is the crop's)."""
    def slow(lab):
        H, W = lab.shape
        L = lab.astype(int)
        out = np.full((H, W), SP.CONV)
        for y in range(H):
            for x in range(W):
                A = L[y, x]
                ys, xs = range(max(y - 2, 0), min(y + 3, H)), range(max(x - 2, 0), min(x + 3, W))
                w = L[np.ix_(ys, xs)]
                cut_y, cut_x = len(ys) < 5, len(xs) < 5
                if A < 19 and (w == A).all():
                    out[y, x] = SP.INTERIOR if not (cut_y or cut_x) else (SP.FRAME if cut_y != cut_x else SP.CONV)
                elif not (cut_y or cut_x) and w.max() < 19:
                    for v in (w, w.T):
                        l = v[0]
                        if (v == l).all() and l[0] != l[4] and all(l[j] in (l[0], l[4]) for j in range(5)) \
                                and all(not (l[j] == l[4] and l[j + 1] == l[0]) for j in range(4)):
                            out[y, x] = SP.EDGE
        return out
    for name, ys, xs in (('offgrid', slice(0, 44), slice(20, 70)), ('noclass', slice(50, 80), slice(40, 90)), ('face', slice(84, 128), slice(30, 100)),
                         ('band255', slice(0, 12), slice(56, 72))):
        lab = SP.label_map(name, S)[ys, xs]
        assert np.array_equal(SP.pixel_kinds(lab)[0], slow(lab)), name


def test_codes_decode_to_their_window(kinds):
    """Every straight-edge / frame code of `offgrid` and `noclass`, taken apart as ace_code_decode does, gives back the window's five lines."""
    for name in ('offgrid', 'noclass', 'ring4'):
        lab = SP.label_map(name, S).astype(int)
        kind, code = kinds[name]
        for y, x in np.argwhere(code >= 0)[::7]:
            frame, o, A, B, s = SP.decode(int(code[y, x]))
            assert frame == (kind[y, x] == SP.FRAME)
            for i in range(5):
                yy, xx = (y, x - 2 + i) if o == 0 else (y - 2 + i, x)
                inside = 0 <= yy < S and 0 <= xx < S
                want = ((A if i >= s else None) if s <= 2 else (A if i < s else None)) if frame else (A if i < s else B)
                assert (lab[yy, xx] if inside else None) == want, (name, y, x, i)


def test_every_kind_is_well_represented(kinds):
    assert len(SP.MAP_NAMES) <= 9
    total = {k: sum(int((kd == k).sum()) for kd, _ in kinds.values()) for k in range(4)}
    print({SP.KIND_NAMES[k]: v for k, v in total.items()})
    assert all(v >= 256 for v in total.values()), total


def test_straight_edges_in_both_orientations_with_every_split(kinds):
    seen = set()
    for kd, code in kinds.values():
        for c in np.unique(code[kd == SP.EDGE]):
            _, o, _, _, s = SP.decode(int(c))
            seen.add((o, s))
    assert seen == {(o, s) for o in (0, 1) for s in (1, 2, 3, 4)}, seen


def test_frame_pixels_on_all_four_borders_at_both_distances(kinds):
    seen = set()
    for kd, code in kinds.values():
        for c in np.unique(code[kd == SP.FRAME]):
            _, o, _, _, s = SP.decode(int(c))
            seen.add((o, s))          # (0, 2) / (0, 1): left border at distance 0 / 1; (0, 3) / (0, 4): right; o = 1: top / bottom
    assert seen == {(o, s) for o in (0, 1) for s in (1, 2, 3, 4)}, seen
    kd = kinds['one_region'][0]
    assert (kd[2:-2, 0] == SP.FRAME).all() and (kd[2:-2, 1] == SP.FRAME).all() and (kd[-1, 2:-2] == SP.FRAME).all() and (kd[:2, :2] == SP.CONV).all()


def test_diag_has_no_interior_and_one_region_few_quads(kinds):
    assert not (kinds['diag'][0] == SP.INTERIOR).any()
    assert SP.boundary_quads(kinds['one_region'][0]) <= 64          # one chunk of 64 per sample: the pre-gathered patches engage


def test_a_no_class_label_touches_the_frame_and_a_straight_border():
    lab = SP.label_map('noclass', S)
    big = lab >= 19
    assert big[0, :].any() and big[:, 0].any() and big[-1, :].any()
    # a straight border: ten rows along which the label left of one column is < 19 and >= 19 right of it (or the reverse), five columns deep
    found = False
    for x in range(5, S - 5):
        for y in range(0, S - 10):
            l, r = lab[y:y + 10, x - 5:x], lab[y:y + 10, x:x + 5]
            if (l == l[0, 0]).all() and (r == r[0, 0]).all() and (l[0, 0] >= 19) != (r[0, 0] >= 19):
                found = True
    assert found


def test_offgrid_borders():
    for S_ in (128, 160, 256):
        lab = SP.offgrid_labels(S_)
        assert len(np.unique(lab)) >= 4
        cx = set((np.nonzero(lab[0, 1:] != lab[0, :-1])[0] + 1).tolist()) | set((np.nonzero(lab[S_ // 2, 1:] != lab[S_ // 2, :-1])[0] + 1).tolist())
        cy = set((np.nonzero(lab[1:, 0] != lab[:-1, 0])[0] + 1).tolist()) | set((np.nonzero(lab[1:, S_ // 2] != lab[:-1, S_ // 2])[0] + 1).tolist())
        for cuts in (cx, cy):
            assert {31, 33, 63, 65} <= cuts and {c % 4 for c in cuts} == {1, 2, 3}, cuts
        assert lab[1, 1] != lab[2, 2] and lab[1, 1] != lab[1, 2] and lab[1, 1] != lab[2, 1]      # a rectangle corner at (2, 2)


# ---- oracle dtype ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small():
    """ngf 16, S 128, four maps: the oracle pair, the inputs and a Reference (the top level runs the same ops as at ngf 64 on fewer channels)."""
    from ctrlhair_amd import procedural as P
    ngf, names = 16, ('one_region', 'offgrid', 'noclass', 'face')
    sd = P.sean_state_dict(0, ngf)
    labels = SP.label_batch(S, names)
    codes, noise = P.style_codes(len(names), seed=61), P.noise_planes(len(names), S, ngf, seed=62)
    t64, t32 = SP.oracle_pair(sd, labels, codes, noise, ngf)
    return dict(ngf=ngf, names=names, sd=sd, labels=labels, codes=codes, noise=noise, t64=t64, t32=t32, ref=SP.Reference(t64, t32, labels, names))


def test_default_dtype_is_the_f32_oracle_bit_for_bit(small):
    from oracle import sean_oracle as O
    taps = {}
    img = O.generator_forward(O.to_torch(small['sd']), small['labels'], small['codes'], small['noise'], small['ngf'], taps=taps)
    assert img.dtype == torch.float32 and torch.equal(img, small['t32'][SP.IMAGE])
    assert all(t.dtype == torch.float32 and torch.equal(t, small['t32'][n]) for n, t in taps.items())
    assert O.one_hot(torch.from_numpy(small['labels'])).dtype == torch.float32


def test_float64_run_is_double_throughout_and_close(small):
    assert all(t.dtype == torch.float64 for t in small['t64'].values())
    ref = small['ref']
    worst = max(float(ref.E32[s].max()) for s in ref.stages)
    print(f'max E32 over the stages: {worst:.2e}')
    assert 0 < worst <= 1e-4                      # an f32 evaluation of the same network: not equal, and not another network
    # a weights cache shared by the two dtypes serves each its own
    from oracle import sean_oracle as O
    def run(wc, dtype):
        return O.generator_forward(O.to_torch(small['sd']), small['labels'][:1], small['codes'][:1], small['noise'][:1], small['ngf'],
                                   weights_cache=wc, dtype=dtype)
    wc = {}
    a, b, a2 = run(wc, torch.float32), run(wc, torch.float64), run(wc, torch.float32)
    assert torch.equal(a, run({}, torch.float32)) and torch.equal(a, a2) and torch.equal(b, run({}, torch.float64))


def test_zencoder_dtype():
    from ctrlhair_amd import procedural as P
    from oracle import sean_oracle as O
    sd = O.to_torch(P.sean_state_dict(0, 16))
    img, lab = P.synthetic_images(1, 64), P.blocky_labels(1, 64, grid=8)
    a, b = O.zencoder_forward(sd, img, lab), O.zencoder_forward(sd, img, lab, dtype=torch.float64)
    assert a.dtype == torch.float32 and b.dtype == torch.float64 and float((a.double() - b).abs().max()) <= 1e-5


# ---- F(4x4,3x3) model ------------------------------------------------------------------------------------------------------------
def test_f4_model_is_exact_in_float64():
    rng = np.random.default_rng(3)
    x, w = rng.standard_normal((12, 16, 24)), rng.standard_normal((5, 12, 3, 3))
    assert np.abs(SP.wino4_model(x, w, np.float64) - SP.direct_model(x, w, np.float64)).max() <= 1e-12


def test_f4_model_error_in_float32():
    """e4(C) and the sequential direct f32 sum's E on the same data (printed); the F(4x4) conv stays a small multiple of the direct one."""
    for C in (64, 128, 512):
        w4, direct = SP.e4(C, with_direct=True)
        print(f'C = {C}: e4 = {w4:.2e}, sequential direct f32 sum {direct:.2e}')
        assert direct < w4 < 30 * direct and w4 < 2e-4


def test_f4_channels_follow_the_library_conditions():
    """Only levels on the 32 grid take F(4x4,3x3): ngf 24, S 160 has the 160-pixel level alone (up_3: 48 and 24 channels), not up_1's 192 at 40
    pixels; ngf 64, S 128 has up_1 at 32 pixels (512); ngf 16, S 128 the styled SPADE convs at 32 / 64 pixels (128 hidden + 19 one-hot planes) above
    the ResBlock's 128; nothing below 32 pixels."""
    assert SP.f4_channels(24, 160) == 48 and SP.f4_channels(64, 128) == 512 and SP.f4_channels(16, 256) == 256
    assert SP.f4_channels(16, 128) == 147 and SP.f4_channels(64, 16) == 0


# ---- power of the check ----------------------------------------------------------------------------------------------------------
def _image_from(small, stage, value):
    from oracle import sean_oracle as O
    return O.generator_forward(O.to_torch(small['sd']), small['labels'], small['codes'], small['noise'], small['ngf'], replace={stage: value})


def test_clean_f32_taps_pass(small):
    failure, worst = small['ref'].check(small['t32'])
    assert failure is None and worst[0] <= 1.0 / SP.K_BOUND + 1e-12, (str(failure), worst)


@pytest.mark.parametrize('stage,kind', [('up_3.h1', SP.FRAME), ('up_3.h0', SP.EDGE)])
def test_a_shift_of_1e_4_rms_on_one_pixel_kind_fails_at_its_stage(small, stage, kind):
    """The f32 oracle's taps with the pixels of one kind of one stage shifted by 1e-4 x rms (bound without the F(4x4) term: the paths sean.wino = 1 / 0
    and f16x3, which share the interior pass, the table rows and the classification with the default path).  The image the oracle makes from the
    shifted stage stays within 1e-3 of the clean one: no image-level test sees it.
    WITH the F(4x4) term -- the exact-f32 default and sean.batch_invariant = 1 -- the bound of this shape is about 4 e4(147) = 1e-4 above that, and the
    same 1e-4 shift reaches 0.74 / 0.80 of it (printed below, so that the limit is on record); there a shift of 1.5 times that bound must fail."""
    ref = small['ref']
    got = dict(small['t32'])
    t = got[stage].clone()
    hit = []
    for b, name in enumerate(small['names']):
        m = torch.from_numpy(ref.kinds(b, S) == kind)
        if m.any():
            hit.append(b)
            t[b][:, m] += 1e-4 * float(ref.rms[stage][b])
    got[stage] = t
    failure, _ = ref.check(got)
    assert failure is not None and failure.stage == stage and failure.sample == hit[0] and failure.kind == SP.KIND_NAMES[kind], str(failure)
    assert failure.map == small['names'][hit[0]] and failure.E > failure.bound
    others = [v for k, v in failure.by_kind.items() if k != SP.KIND_NAMES[kind]]
    assert failure.by_kind[SP.KIND_NAMES[kind]] > failure.bound and all(v <= failure.bound for v in others), str(failure)
    d = float((_image_from(small, stage, t) - small['t32'][SP.IMAGE]).abs().max())
    print(f'{stage}, {SP.KIND_NAMES[kind]} pixels + 1e-4 rms: {failure}; image moves by {d:.2e}')
    assert d <= 1e-3
    # the same with the F(4x4) term in the bound
    e4_term = SP.e4(SP.f4_channels(small['ngf'], S))
    _, worst = ref.check(got, e4_term)
    bound4 = ref.bound(stage, e4_term)
    print(f'with e4 = {e4_term:.2e}: bound {float(bound4[hit[0]]):.2e}, the 1e-4 shift reaches {worst[0]:.2f} of it')
    t4 = small['t32'][stage].clone()
    for b in hit:
        t4[b][:, torch.from_numpy(ref.kinds(b, S) == kind)] += 1.5 * float(bound4[b]) * float(ref.rms[stage][b])
    f4, _ = ref.check(dict(small['t32'], **{stage: t4}), e4_term)
    assert f4 is not None and f4.stage == stage and f4.sample == hit[0] and f4.kind == SP.KIND_NAMES[kind], str(f4)


def test_a_transposed_noise_ring_fails_at_its_stage(small):
    """up_3.ace_1's noise plane read as [H][W] instead of [W][H] on the outermost ring only: fails at up_3.h1 on a frame pixel (one_region: the
    ring is frame pixels but for the corners), nowhere before.  (Unlike the two shifts this error is no small one -- the image moves by 1.8e-1 on the
    ring -- so no claim about the image-level 1e-3 is made for it; what is checked is that the checker places it.)"""
    from ctrlhair_amd.sean import arch
    from oracle import sean_oracle as O
    ngf = small['ngf']
    sizes = arch.noise_plane_sizes(S, ngf)
    off = sum(r * r for r in sizes[:-1])
    noise = small['noise'].copy()
    plane = noise[:, off:].reshape(-1, S, S)
    ring = np.ones((S, S), bool)
    ring[1:-1, 1:-1] = False
    plane[:, ring] = plane.transpose(0, 2, 1)[:, ring]
    taps = {}
    img = O.generator_forward(O.to_torch(small['sd']), small['labels'], small['codes'], noise, ngf, taps=taps)
    taps[SP.IMAGE] = img
    failure, _ = small['ref'].check(taps)
    d = float((img - small['t32'][SP.IMAGE]).abs().max())
    print(f'transposed noise ring: {failure}; image moves by {d:.2e}')
    assert failure is not None and failure.stage == 'up_3.h1' and failure.sample == 0 and failure.kind == 'frame', str(failure)
    assert all(v <= failure.bound for k, v in failure.by_kind.items() if k in ('interior', 'straight-edge'))
