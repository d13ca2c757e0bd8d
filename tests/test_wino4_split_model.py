"""CPU restatement of the position-split F(4x4,3x3) kernel (ctrlhair_amd/csrc/conv_wino4_split.h) in numpy float32, operation by
operation, against the un-split sequence of wino4_in1d / wino4_out1d (conv_wino4.h) written out the same way: the two must agree bit
for bit, which is the argument why wino4_plain_split_kernel reproduces wino4_plain_kernel's outputs exactly.  Also the fragment order of
the split kernel's weight image (wino4_split_frag).  SEAN ResBlock convs: /root/reference/sean_codes/models/networks/architecture.py:82-91."""
from fractions import Fraction

import numpy as np

F = np.float32


def _round_f32(exact, near):
    """The float32 nearest to the rational `exact`, given a float32 `near` at most one ulp away (no ties: see fma)."""
    cands = [np.nextafter(near, F(-np.inf)), near, np.nextafter(near, F(np.inf))]
    return min(cands, key=lambda c: abs(Fraction(float(c)) - exact))


def fma(a, b, c):
    """One fused multiply-add in float32, rounded once.  The product of two float32 is exact in float64; if adding c to it in float64 is
    exact as well (TwoSum says so) the conversion to float32 is the single rounding.  Otherwise the float64 sum is already rounded and a
    second rounding could go the other way at a float32 tie: decide in rational arithmetic (the exact value is then no tie itself -- a
    float32 tie has 25 significant bits and would have been exact in float64)."""
    a, b, c = np.float64(F(a)), np.float64(F(b)), np.float64(F(c))
    p = a * b
    s = p + c
    bb = s - p
    if (p - (s - bb)) + (c - bb) == 0 or not np.isfinite(s):
        return F(s)
    return _round_f32(Fraction(float(p)) + Fraction(float(c)), F(s))


def in1d(d):
    """wino4_in1d (conv_wino4.h): B^T d, the six outputs."""
    d0, d1, d2, d3, d4, d5 = d
    a, b = fma(-4, d2, d4), fma(-4, d1, d3)
    c, t = F(d4 - d2), F(d3 - d1)
    return [fma(4, d0, fma(-5, d2, d4)), F(a + b), F(a - b), fma(2, t, c), fma(-2, t, c), fma(4, d1, fma(-5, d3, d5))]


def in1d_half(jh, d):
    """wino4_in1d_half<JH> (conv_wino4_split.h): the three outputs of wave half jh, which never touch d5 (jh = 0) / d0 (jh = 1)."""
    if jh == 0:
        d0, d1, d2, d3, d4 = d[:5]
        a, b = fma(-4, d2, d4), fma(-4, d1, d3)
        return [fma(4, d0, fma(-5, d2, d4)), F(a + b), F(a - b)]
    d1, d2, d3, d4, d5 = d[1:]
    c, t = F(d4 - d2), F(d3 - d1)
    return [fma(2, t, c), fma(-2, t, c), fma(4, d1, fma(-5, d3, d5))]


def out1d(m):
    """wino4_out1d (conv_wino4.h): A^T m."""
    m0, m1, m2, m3, m4, m5 = m
    s1, d1, s2, d2 = F(m1 + m2), F(m1 - m2), F(m3 + m4), F(m3 - m4)
    return [F(F(m0 + s1) + s2), fma(2, d2, d1), fma(4, s2, s1), F(fma(8, d2, d1) + m5)]


def out1d_part(jh, m):
    """wino4_out1d_part<JH>: what each wave forms of the second pass from its three columns."""
    a, b, c = m
    if jh == 0:
        s1 = F(b + c)
        return [F(a + s1), s1, F(b - c)]
    return [F(a + b), F(a - b), c]


def out1d_join(left, right):
    """wino4_out1d_join: the last operation of each output, on the two waves' triples."""
    (m0s1, s1, d1), (s2, d2, m5) = left, right
    return [F(m0s1 + s2), fma(2, d2, d1), fma(4, s2, s1), F(fma(8, d2, d1) + m5)]


def input_transform(d):
    """V = B^T d B as the kernels do it: row pass along each patch row, column pass over the rows.  [6][6] -> V[i][j]."""
    rows = [in1d(d[r]) for r in range(6)]
    V = np.empty((6, 6), F)
    for j in range(6):
        V[:, j] = in1d([rows[r][j] for r in range(6)])
    return V


def input_transform_split(jh, d):
    """The wave half's 18 positions: six half row transforms, three full column transforms.  -> V[i][jj], j = 3 jh + jj."""
    rows = [in1d_half(jh, d[r]) for r in range(6)]
    V = np.empty((6, 3), F)
    for jj in range(3):
        V[:, jj] = in1d([rows[r][jj] for r in range(6)])
    return V


def output_transform(M):
    """Y = A^T M A as wino4_plain_epilogue: first pass over i per column j, second pass over j per output row."""
    t = np.empty((4, 6), F)
    for j in range(6):
        t[:, j] = out1d(M[:, j])
    return np.array([out1d(t[r]) for r in range(4)], F)


def output_transform_split(M):
    """The split epilogue: each wave half runs the first pass on its three columns and forms its triples; one of them joins the two."""
    part = []
    for jh in range(2):
        t = np.empty((4, 3), F)
        for jj in range(3):
            t[:, jj] = out1d(M[:, 3 * jh + jj])
        part.append([out1d_part(jh, t[r]) for r in range(4)])
    return np.array([out1d_join(part[0][r], part[1][r]) for r in range(4)], F)


def _patches(rng, n):
    """Random 6 x 6 float32 arrays: O(1) values, mixed magnitudes (2^-20 .. 2^20 per entry), signed zeros and exact small integers."""
    out = [rng.standard_normal((6, 6)).astype(F) for _ in range(n)]
    out += [(rng.standard_normal((6, 6)) * np.exp2(rng.integers(-20, 21, (6, 6)))).astype(F) for _ in range(n)]
    out += [rng.integers(-3, 4, (6, 6)).astype(F) * F(-1.0) for _ in range(n // 4)]
    out += [(rng.standard_normal((6, 6)) * (rng.random((6, 6)) < 0.3)).astype(F) for _ in range(n // 4)]
    return out


def test_fma_helper_is_a_float32_fma():
    """The helper against rational arithmetic, on the transforms' constants and on a case where rounding twice goes wrong."""
    rng = np.random.default_rng(0)
    cases = [(F(4), F(1 + 2.0 ** -23), F(2.0 ** -60))]     # 4 x is exact; + 2^-60 is lost in float64 but cannot be a float32 tie either way
    cases += [(F(5), F(1 + 2.0 ** -22), F(2.0 ** -60))]      # 5 x = 5 + 2.5 ulp lies on a float32 tie; + 2^-60 breaks it upwards, but not in float64
    for _ in range(3000):
        cases.append((F(rng.choice([-5, -4, -2, 2, 4, 8])), F(rng.standard_normal() * 2.0 ** int(rng.integers(-20, 21))),
                      F(rng.standard_normal() * 2.0 ** int(rng.integers(-20, 21)))))
    for a, x, y in cases:
        exact = Fraction(float(a)) * Fraction(float(x)) + Fraction(float(y))
        lo = F(float(exact))
        cands = [np.nextafter(lo, F(-np.inf)), lo, np.nextafter(lo, F(np.inf))]
        dist = sorted((abs(Fraction(float(c)) - exact), float(c)) for c in cands)
        # (a tie has 25 significant bits: float(exact) is exact and its conversion rounds half to even)
        want = dist[0][1] if dist[0][0] < dist[1][0] else float(lo)
        assert float(fma(a, x, y)) == want, (a, x, y)
    x, y = F(1 + 2.0 ** -22), F(2.0 ** -60)
    assert fma(5, x, y) == F(5 + 12 * 2.0 ** -23) and F(np.float64(5) * np.float64(x) + np.float64(y)) == F(5 + 8 * 2.0 ** -23)


def test_half_row_transforms_are_the_same_expressions():
    rng = np.random.default_rng(1)
    for d in _patches(rng, 40):
        for r in range(6):
            full = in1d(d[r])
            assert np.array_equal(np.array(in1d_half(0, d[r]), F), np.array(full[:3], F))
            assert np.array_equal(np.array(in1d_half(1, d[r]), F), np.array(full[3:], F))
    # the halo columns: r0 .. r2 do not read d5, r3 .. r5 do not read d0
    d = rng.standard_normal(6).astype(F)
    e = d.copy()
    e[5] = F(1e30)
    assert in1d_half(0, d) == in1d_half(0, e)
    e = d.copy()
    e[0] = F(1e30)
    assert in1d_half(1, d) == in1d_half(1, e)


def test_split_input_transform_equals_the_unsplit_one():
    rng = np.random.default_rng(2)
    for d in _patches(rng, 60):
        V = input_transform(d)
        for jh in range(2):
            assert np.array_equal(input_transform_split(jh, d), V[:, 3 * jh:3 * jh + 3]), jh


def test_split_output_transform_equals_the_unsplit_one():
    rng = np.random.default_rng(3)
    for M in _patches(rng, 100):
        a, b = output_transform(M), output_transform_split(M)
        assert np.array_equal(a, b) and np.array_equal(np.signbit(a), np.signbit(b))


def test_whole_tile_through_both_evaluations():
    """Patch -> V -> M = sum over channels of U .* V (the MFMA's f32 fma chain, channel by channel) -> Y, split against un-split."""
    rng = np.random.default_rng(4)
    C = 8
    for scale in (1.0, 1e-3, 300.0):
        d = (rng.standard_normal((C, 6, 6)) * scale).astype(F)
        U = rng.standard_normal((C, 6, 6)).astype(F)
        M = np.zeros((6, 6), F)
        Ms = np.zeros((6, 6), F)
        for c in range(C):
            V = input_transform(d[c])
            Vs = np.concatenate([input_transform_split(0, d[c]), input_transform_split(1, d[c])], axis=1)
            for i in range(6):
                for j in range(6):
                    M[i, j] = fma(U[c, i, j], V[i, j], M[i, j])
                    Ms[i, j] = fma(U[c, i, j], Vs[i, j], Ms[i, j])
        assert np.array_equal(output_transform(M), output_transform_split(Ms))


def split_frag(m, i, j):
    """wino4_split_frag (conv_wino4.h)."""
    return (j // 3) * 36 + 2 * (3 * i + j % 3) + m


def test_fragment_order_of_the_split_weight_image():
    """Every (row half, position) exactly once; the 36 fragments of wave half jh = j // 3 fill the nine consecutive 16-byte units
    9 jh .. 9 jh + 8; a unit holds two positions x two row halves, in the order of the four MFMAs of a group."""
    seen = {}
    for m in range(2):
        for i in range(6):
            for j in range(6):
                a = split_frag(m, i, j)
                assert a not in seen
                seen[a] = (m, i, j)
    assert sorted(seen) == list(range(72))
    for jh in range(2):
        units = sorted({a >> 2 for a, (m, i, j) in seen.items() if j // 3 == jh})
        assert units == list(range(9 * jh, 9 * jh + 9))
        assert sum(1 for a, (m, i, j) in seen.items() if j // 3 == jh) == 36
    for u in range(18):
        frs = [seen[4 * u + e] for e in range(4)]
        q = [3 * i + j % 3 for m, i, j in frs]
        assert [m for m, _, _ in frs] == [0, 1, 0, 1] and q[0] == q[1] and q[2] == q[3] == q[0] + 1 and q[0] == 2 * (u % 9)
