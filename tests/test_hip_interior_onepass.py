"""GPU tests of the code table of the four-pixel interior pass (ace_interior_f32_tile4_kernel, ctrlhair_amd/csrc/ace_sparse.hip; option
sean.int_onepass).  A block of 128 x 8 pixels hashes its distinct straight-edge codes into 128 key slots and compacts them to ranks; with
at most 64 codes it runs steps of 32 channels over 64 table rows, with 65 ... 128 codes steps of 16 channels over 128 rows -- one round
either way -- and beyond 128 codes further rounds at the narrow width.  sean.int_onepass = 0 keeps 64 slots and rounds beyond them.  The
table rows are built with 16-byte loads over four channels.  None of this changes an operation of
    out = act((bn_a x + nv nz + bn_d) (1 + gamma) + beta)          (normalization.py:111-112,182; architecture.py:95)
or of the row sums E[code] + P6[t = 0] + P6[t = 1] + P6[t = 2], so every variant must give the same bits.  All cases run through
SeanGenerator on the exact-f32 path; the codes per block are counted on the host from the definition in ace_sparse.h and asserted, so a
case cannot pass without the path it is named for."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _run(gen, labels, codes, noise, **opts):
    for k, v in opts.items():
        gen.handle.set_option('sean.' + k, v)
    dev = gen.device
    out = gen.generate(torch.from_numpy(labels).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(noise).to(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope='module')
def gens(hip_lib):
    """One generator per (ngf, batch, size, sean.edge), shared by the cases of this module (the live options may be set at any time)."""
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.sean.generator import SeanGenerator
    made = {}

    def get(ngf, B, S, edge=1):
        key = (ngf, B, S, edge)
        if key not in made:
            sd = P.sean_state_dict(0, ngf, calibrated=ngf in (16, 64))
            made[key] = SeanGenerator(0, f16x3=0, options={'sean.edge': edge}).load_state_dict(sd, max_batch=B, max_size=S)
        return made[key]
    yield get
    for g in made.values():
        g.handle.close()


def _pair_codes(lab):
    """Straight-edge code of every pixel of one label map [H][W] (-1: none), as tests/test_hip_interior_groups.py::_edge_codes defines it
    (ace_sparse.h / ace_edge_code), vectorised: the 5x5 window lies inside the image and is five uniform columns (orientation 0) or rows
    (1) A^s B^(5-s), s = 1..4, A != B, both < 19; code = ((orientation * 19 + A) * 19 + B) * 4 + (s - 1).  Columns are tried first."""
    H, W = lab.shape
    out = np.full((H, W), -1, np.int32)
    for o in (1, 0):                                           # (orientation 0 written last: it wins)
        L = lab.astype(np.int32) if o == 0 else lab.astype(np.int32).T
        h, w = L.shape
        # un[y][x]: the five labels L[y-2 .. y+2][x] are equal (y in 2 .. h-3)
        un = np.zeros((h, w), bool)
        un[2:h - 2] = np.all([L[2 + d:h - 2 + d] == L[2:h - 2] for d in (-2, -1, 1, 2)], axis=0)
        c = np.full((h, w), -1, np.int32)
        l = [L[2:h - 2, j:w - 4 + j] for j in range(5)]        # the five line labels of the window centred at (y, x), x in 2 .. w-3
        ok = np.all([un[2:h - 2, j:w - 4 + j] for j in range(5)], axis=0)
        A, Bl = l[0], l[4]
        ok &= (A < 19) & (Bl < 19) & (A != Bl)
        r1 = l[1] == A
        r2 = r1 & (l[2] == A)
        r3 = r2 & (l[3] == A)
        s = 1 + r1.astype(np.int32) + r2 + r3
        for j in (1, 2, 3):
            ok &= l[j] == np.where(j < s, A, Bl)
        c[2:h - 2, 2:w - 2] = np.where(ok, ((o * 19 + A) * 19 + Bl) * 4 + (s - 1), -1)
        c = c if o == 0 else c.T
        out = np.where(c >= 0, c, out)
    return out


def _frame_codes(lab, pair):
    """Frame code (ace_sparse.h, round 9) of every pixel without a pair code: within 2 of exactly one image border, label A < 19, the in-image
    part of its 5x5 window uniformly A; code = 2888 + (o * 19 + A) * 4 + (s - 1), s = lines outside before the window (left / top) or
    5 - lines outside after it."""
    H, W = lab.shape
    out = np.full((H, W), -1, np.int32)
    for y in range(H):
        for x in (range(W) if (y < 2 or y >= H - 2) else list(range(2)) + list(range(W - 2, W))):
            cl, cr, rt, rb = max(2 - x, 0), max(x + 3 - W, 0), max(2 - y, 0), max(y + 3 - H, 0)
            A = int(lab[y, x])
            if pair[y, x] >= 0 or A >= 19 or ((cl + cr) != 0) == ((rt + rb) != 0):
                continue
            if (lab[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3] == A).all():
                o = 0 if (cl + cr) else 1
                lead, trail = (rt, rb) if o else (cl, cr)
                out[y, x] = 2888 + (o * 19 + A) * 4 + ((lead if lead else 5 - trail) - 1)
    return out


def _codes_per_tile(labels):
    """Distinct codes per block of 128 x 8 pixels over all samples: {tile width: (pair codes only, with frame codes)} as lists."""
    per = {}
    for lab in labels:
        H, W = lab.shape
        pair = _pair_codes(lab)
        both = np.where(pair >= 0, pair, _frame_codes(lab, pair))
        for ty in range(0, H, 8):
            for tx in range(0, W, 128):
                p, a = pair[ty:ty + 8, tx:tx + 128], both[ty:ty + 8, tx:tx + 128]
                n = per.setdefault(min(128, W - tx), ([], []))
                n[0].append(len(np.unique(p[p >= 0])))
                n[1].append(len(np.unique(a[a >= 0])))
    return per


def _many_pairs_stripes(B, S):
    """Vertical stripes of 3 pixels whose ordered label pairs (left, right) never repeat along x (tests/test_hip_interior_groups.py): two
    codes per stripe border and no code twice."""
    seq, used = [0], set()
    while len(seq) * 3 < S:
        a = seq[-1]
        nxt = next(b for k in range(1, 19) for b in [(a + k * 7) % 19] if (a, b) not in used)
        used.add((a, nxt))
        seq.append(nxt)
    row = np.repeat(np.asarray(seq, np.uint8), 3)[:S]
    lab = np.empty((B, S, S), np.uint8)
    for b in range(B):
        lab[b] = ((row.astype(np.int32) + 5 * b) % 19).astype(np.uint8)[None, :]
    return lab


def _random_cells(B, S):
    """Cells of 5 x 8 pixels (width x height) with labels from default_rng(5): four codes per vertical border and four per cell centre
    column -- well above 128 per block."""
    g = np.random.default_rng(5).integers(0, 19, size=(B, (S + 7) // 8, (S + 4) // 5)).astype(np.uint8)
    return np.repeat(np.repeat(g, 8, axis=1), 5, axis=2)[:, :S, :S].copy()


def _labels(name, B, S):
    from ctrlhair_amd import procedural as P
    if name == 'blocky16':
        return P.blocky_labels(B, S, grid=16)
    if name == 'stripes3':
        return _many_pairs_stripes(B, S)
    if name == 'cells5x8':
        return _random_cells(B, S)
    if name == 'blocky8':
        return P.blocky_labels(B, S, grid=8)
    if name == 'face':
        return np.stack([P.face_like_labels(S, 40 + b) for b in range(B)])
    if name == 'one_region':
        return np.full((B, S, S), 13, np.uint8)
    if name == 'blocky20':
        return P.blocky_labels(B, S, grid=20)
    raise KeyError(name)


def _census(name, lab):
    per = _codes_per_tile(lab)
    for w, (p, a) in sorted(per.items()):
        print(f'{name}: tiles of {w} x 8 pixels: pair codes {min(p)}..{max(p)} (mean {np.mean(p):.1f}), with frame codes {min(a)}..{max(a)}')
    return per


# what the host count of a label set must show (pair codes, as the definition of tests/test_hip_interior_groups.py counts them)
def _expect_narrow_one_round(per):
    p, a = per[128]
    assert min(p) > 64 and max(p) <= 128 and max(a) <= 128, (min(p), max(p), max(a))


def _expect_rounds_at_narrow_width(per):
    assert max(per[128][0]) > 128, max(per[128][0])


def _expect_unchanged_path(per):
    assert max(per[128][1]) <= 64, max(per[128][1])


def _expect_ragged(per):
    p, r = per[128][0], per[32][0]
    assert min(p) > 64 and max(p) <= 128 and max(per[128][1]) <= 128, (min(p), max(p), max(per[128][1]))
    assert 0 < min(r) and max(r) <= 64, (min(r), max(r))


CASES = [('blocky16', 64, 128, 2, _expect_narrow_one_round), ('stripes3', 64, 128, 2, _expect_narrow_one_round),
         ('cells5x8', 64, 128, 2, _expect_rounds_at_narrow_width), ('blocky8', 64, 128, 2, _expect_unchanged_path),
         ('face', 64, 128, 2, _expect_unchanged_path), ('one_region', 64, 128, 2, _expect_unchanged_path),
         ('blocky20', 24, 160, 2, _expect_ragged)]


@pytest.mark.parametrize('name,ngf,S,B,expect', CASES, ids=[c[0] for c in CASES])
def test_code_table_variants_are_bit_identical(gens, name, ngf, S, B, expect):
    """sean.int_onepass = 0 against 1, sean.int_groups = 1 / 2 / 0 at int_onepass = 1, and a repeated call: np.array_equal.  (The key table is
    filled through atomics, so slot order and ranks may differ from run to run -- the values read may not.)  ngf = 24, S = 160: 48 / 24
    channels -- partial steps of 32 and of 16 channels -- and a ragged tile of 32 x 8 pixels beside the 128-wide one."""
    from ctrlhair_amd import procedural as P
    lab = _labels(name, B, S)
    expect(_census(name, lab))
    codes, noise = P.style_codes(B, seed=31), P.noise_planes(B, S, ngf, seed=32)
    gen = gens(ngf, B, S)
    try:
        ref = _run(gen, lab, codes, noise, int_onepass=0, int_groups=0)
        assert np.isfinite(ref).all()
        for g in (1, 2, 0):
            got = _run(gen, lab, codes, noise, int_onepass=1, int_groups=g)
            assert np.array_equal(ref, got), (name, 'int_groups', g, float(np.abs(ref - got).max()))
        assert np.array_equal(ref, _run(gen, lab, codes, noise, int_onepass=1, int_groups=0)), (name, 'repeated call differs')
    finally:
        gen.handle.set_option('sean.int_onepass', 1)
        gen.handle.set_option('sean.int_groups', 0)


@pytest.mark.parametrize('name', ['blocky16', 'cells5x8'])
def test_table_rows_against_the_boundary_conv(gens, name):
    """int_onepass = 1 (one round at the narrow width / rounds at the narrow width) against sean.edge = 0, where the same pixels go through the
    boundary conv: <= 1e-5, the bound of tests/test_hip_interior_groups.py::test_second_round_of_the_code_table."""
    from ctrlhair_amd import procedural as P
    ngf, S, B = 64, 128, 2
    lab = _labels(name, B, S)
    codes, noise = P.style_codes(B, seed=31), P.noise_planes(B, S, ngf, seed=32)
    got = _run(gens(ngf, B, S), lab, codes, noise, int_onepass=1, int_groups=0)
    off = _run(gens(ngf, B, S, edge=0), lab, codes, noise)
    d = float(np.abs(got - off).max())
    print(f'{name}: max |table rows - boundary conv| = {d:.3e}')
    assert d <= 1e-5


def test_narrow_width_against_the_oracle(gens):
    """16 x 16-block labels at S = 128, one sample (every block above 64 codes: the narrow width) against the PyTorch oracle at the project's 1e-3."""
    from ctrlhair_amd import procedural as P
    from oracle import sean_oracle as O
    ngf, S = 64, 128
    lab = _labels('blocky16', 1, S)
    _expect_narrow_one_round(_census('blocky16 (B = 1)', lab))
    sd = P.sean_state_dict(0, ngf)
    codes, noise = P.style_codes(1, seed=31), P.noise_planes(1, S, ngf, seed=32)
    got = _run(gens(ngf, 1, S), lab, codes, noise, int_onepass=1, int_groups=0)
    ref = O.generator_forward(O.to_torch(sd), lab, codes, noise, ngf).numpy()
    d = float(np.abs(got - ref).max())
    print(f'int_onepass=1 ngf={ngf} S={S} blocky16: max |hip - oracle| = {d:.3e}')
    assert d <= 1e-3
