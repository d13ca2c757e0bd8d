"""CPU: the exact Delaunay checker (tests/delaunay_oracle.py) on the host mesher's meshes, and warping.build_points_batch."""
import numpy as np
import pytest

from tests import delaunay_oracle as D
from tests.warp_cases import cases

COUNTS = (1402, 1398, 1414, 1412)        # build_mesh on the four fixture pairs; all 196 frame nodes are on the hull


@pytest.mark.parametrize('i', range(4))
def test_checker_accepts_the_host_meshes(i):
    c = cases()[i]
    h, unique = D.check(c['V'], c['F'], want_unique=True)
    tied, strict = D.tied_edges(c['V'], c['F'])
    print(f'case {i}: {len(c["F"])} triangles, h = {h}, {len(unique)} unique triangles, {len(tied)} tied interior edges')
    assert h == 196 and len(c['F']) == COUNTS[i]
    assert 400 <= len(tied) <= 419
    assert 0 < len(unique) < len(c['F'])


def _strict_convex_edge(V, F):
    P = D.to_grid(V)
    for u, v, w, x in D.tied_edges(V, F)[1]:
        if D.orient(P[u], P[x], P[w]) > 0 and D.orient(P[x], P[v], P[w]) > 0:
            return u, v, w, x
    raise AssertionError('no strictly convex non-tied quad')


def test_checker_rejects_a_flipped_diagonal_a_hole_and_a_duplicate():
    c = cases()[0]
    V, F = c['V'], c['F']
    u, v, w, x = _strict_convex_edge(V, F)
    rows = {tuple(r) for r in F.tolist()}
    canon = lambda t: tuple(int(a) for a in D.canonical(np.array([t]))[0])
    rows -= {canon((u, v, w)), canon((v, u, x))}
    rows |= {canon((u, x, w)), canon((x, v, w))}
    flipped = D.canonical(np.array(sorted(rows)))
    assert len(flipped) == len(F)
    with pytest.raises(D.MeshError, match='locally Delaunay'):
        D.check(V, flipped)
    with pytest.raises(D.MeshError):
        D.check(V, np.delete(F, len(F) // 2, axis=0))
    with pytest.raises(D.MeshError, match='lexicographic'):
        D.check(V, np.insert(F, 7, F[7], axis=0))


def test_build_points_batch_equals_build_mesh_bit_for_bit():
    from ctrlhair_amd import warping as W
    cs = cases()
    V, counts, targets = W.build_points_batch(np.stack([c['hair_lm'] for c in cs]), np.stack([c['face_lm'] for c in cs]))
    assert V.dtype == np.float32 and counts.tolist() == [len(c['V']) for c in cs]
    o = 0
    for c, n in zip(cs, counts):
        assert np.array_equal(V[o:o + n].view(np.int32), c['V'].view(np.int32))
        o += n
    assert np.array_equal(targets.view(np.int32), np.stack([c['bc'] for c in cs]).view(np.int32))
    one = W.build_points_batch(cs[2]['hair_lm'][None], cs[2]['face_lm'][None])[0]
    assert np.array_equal(one.view(np.int32), cs[2]['V'].view(np.int32))


def test_build_points_batch_refuses_duplicates_and_points_outside_the_domain():
    from ctrlhair_amd import warping as W
    cs = cases()
    hl = np.stack([c['hair_lm'] for c in cs]).astype(np.float64)
    fl = np.stack([c['face_lm'] for c in cs])
    dup = hl.copy()
    dup[2, W.CHOSEN_LANDMARKS[5]] = dup[2, W.CHOSEN_LANDMARKS[9]]
    with pytest.raises(ValueError, match='pair 2.*duplicate'):
        W.build_points_batch(dup, fl)
    out = hl.copy()
    out[1, W.CHOSEN_LANDMARKS[0]] = (-0.25, 0.5)             # x = -48 px on the canvas
    with pytest.raises(ValueError, match='pair 1.*domain'):
        W.build_points_batch(out, fl)
    off = hl.copy()
    off[3, W.CHOSEN_LANDMARKS[0]] = ((2.0 + 2.0 ** -21 - 80) / 512, 0.5)     # 2 + 2^-21 px: a float32, not on the 2^-20 grid
    with pytest.raises(ValueError, match='pair 3.*domain'):
        W.build_points_batch(off, fl)
