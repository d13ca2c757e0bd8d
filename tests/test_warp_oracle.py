"""CPU-only: the host oracle of the mask warp (tests/warp_oracle.py) held to properties that pin ARAP independently of any
implementation (libigl itself cannot be built here: Eigen is not available), and the host mesher of ctrlhair_amd/warping.py."""
import numpy as np
import pytest

from tests import warp_oracle as O
from tests.warp_cases import HARD_DU_PX, boundary_band, cases, oracle


def _rigid(P, angle, shift):
    c, s = np.cos(angle), np.sin(angle)
    return (np.asarray(P, np.float64) - 336.0) @ np.array([[c, s], [-s, c]]) + 336.0 + np.asarray(shift)


def test_rigid_constraints_give_the_rigid_motion_and_zero_energy():
    c = cases()[0]
    V = c['V'].astype(np.float64)
    bc = _rigid(V[c['b']], 0.2, (7.0, -4.0))
    U, E = O.arap(V, c['F'], c['b'], bc, return_energy=True)
    err = np.abs(U - _rigid(V, 0.2, (7.0, -4.0))).max()
    print(f'rigid: max |U - rigid(V)| = {err:.3e} px, final energy {E[-1]:.3e}')
    assert err < 1e-8 and E[-1] < 1e-12


def test_identity_constraints_keep_the_mesh():
    c = cases()[1]
    V = c['V'].astype(np.float64)
    U = O.arap(V, c['F'], c['b'], V[c['b']])
    assert np.abs(U - V).max() < 1e-9


@pytest.mark.parametrize('i', range(4))
def test_energy_never_increases(i):
    c = cases()[i]
    _, E = O.arap(c['V'], c['F'], c['b'], c['bc'], return_energy=True)
    print(f'case {i}: energy {E[0]:.6g} -> {E[-1]:.6g}')
    assert (np.diff(E) <= 1e-12 * E[0]).all()


@pytest.mark.parametrize('i', range(4))
def test_build_mesh_is_a_valid_triangulation(i):
    from ctrlhair_amd import warping as W
    c = cases()[i]
    V, F, b = c['V'], c['F'], c['b']
    nodes, targets = W.build_nodes(c['hair_lm'], c['face_lm'])
    assert nodes.shape == (273, 2) and targets.shape == (273, 2)
    assert np.array_equal(V[:273], nodes.astype(np.float32)) and np.array_equal(b, np.arange(273))
    assert np.array_equal(nodes[77:], np.round(targets[77:], 4))          # the frame is constrained to itself
    assert nodes[77:].min() == 0 and nodes[77:].max() == 671
    P = V[F].astype(np.float64)
    a, d = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    area2 = a[:, 0] * d[:, 1] - a[:, 1] * d[:, 0]
    assert (area2 > 0).all()
    assert np.array_equal(np.unique(F), np.arange(len(V)))                # every node is used
    assert abs(area2.sum() / 2 - 671.0 ** 2) < 1e-3                       # the triangles tile the canvas
    ang = []
    for k in range(3):
        e1, e2 = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
        ang.append(np.degrees(np.arccos((e1 * e2).sum(1) / np.linalg.norm(e1, axis=1) / np.linalg.norm(e2, axis=1))))
    print(f'case {i}: {len(V)} vertices ({len(V) - 273} free), {len(F)} triangles, minimum angle {np.min(ang):.2f} deg')
    V2, F2, _ = W.build_mesh(nodes)
    assert np.array_equal(V, V2) and np.array_equal(F, F2)


def test_mesh_caps_are_checked_on_the_host():
    from ctrlhair_amd import warping as W
    V = np.zeros((W.MAX_V + 1, 2), np.float32)
    with pytest.raises(ValueError, match='vertices'):
        W.check_mesh(V, np.zeros((1, 3), np.int32), np.zeros(0, np.int32))
    with pytest.raises(ValueError, match='out of range'):
        W.check_mesh(np.zeros((4, 2), np.float32), np.array([[0, 1, 4]], np.int32), np.zeros(0, np.int32))


def test_sampling_rule_on_hand_made_vectors():
    """cv2.remap's documented arithmetic on a 0/1 mask, then truncation: hair iff every tap of non-zero weight is hair."""
    m = np.zeros((4, 4), np.uint8)
    m[1:3, 1:3] = 1
    f = np.float32
    #               exact pixel    half-way to a 0    fraction below 1/64 rounds to the pixel   outside
    uv = np.array([[[1 / 4, 1 / 4], [1.5 / 4, 2.5 / 4], [(1 + 1 / 128) / 4, 1 / 4], [-1.0, -1.0], [1.5 / 4, 1.5 / 4]]], f)
    assert O.sample(m, uv).tolist() == [[1, 0, 1, 0, 1]]


@pytest.mark.parametrize('i', range(3))
def test_oracle_labels_are_stable_under_the_arap_tolerance(i):
    """What test_hip_warp's end-to-end check relies on: moving the oracle's U by the ARAP tolerance changes the label map only
    on the one-pixel band around the warped-hair boundary, on at most 2 % of that band."""
    c = cases()[i]
    labels, _, U = oracle(i)
    rng = np.random.default_rng(i)
    Up = (U.astype(np.float64) + rng.uniform(-HARD_DU_PX, HARD_DU_PX, U.shape) / np.sqrt(2)).astype(np.float32)
    Up[c['b']] = U[c['b']]
    lab2, _ = O.warp_from_U(c['hair'], c['face'], c['V'], c['F'], Up)
    band = boundary_band(labels == 13)
    diff = labels != lab2
    print(f'case {i}: {int(diff.sum())} pixels differ, band {int(band.sum())} pixels')
    assert not (diff & ~band).any()
    assert diff.sum() <= 0.02 * band.sum()


def test_oracle_raster_equals_the_reference_rasteriser_fixture():
    """tests/golden/warp_meshcore_uv.npz: the UV image mesh_core.cpp's render_colors_core (plain g++ -O2) drew for the float32 U
    of the oracle on a Triangle -q30 mesh (warp_triangle_meshes.npz, pair 0): rows 220..380 as values, the whole canvas as a
    coverage bitmap and a SHA-256.  Pixels may differ only where the inside test sits within 1e-6 of an edge, on at most
    0.1 % of the canvas (measured when the fixture was made: none differ)."""
    import hashlib
    import os
    from tests.warp_cases import CANVAS_PX, GOLDEN, NEAR_EDGE, NEAR_EDGE_CAP
    z = np.load(os.path.join(GOLDEN, 'warp_meshcore_uv.npz'))
    m = np.load(os.path.join(GOLDEN, 'warp_triangle_meshes.npz'))
    uv, margin = O.render_uv(z['U'], m['V0'], m['F0'], return_margin=True)
    r0, r1 = z['uv_rows']
    covered = np.unpackbits(z['covered'])[:CANVAS_PX].reshape(672, 672).astype(bool)
    bad = (uv[..., 0] != -1) != covered
    bad[r0:r1] |= (uv[r0:r1] != z['uv']).any(-1)
    same_hash = hashlib.sha256(np.ascontiguousarray(uv).tobytes()).digest() == z['sha256'].tobytes()
    print(f'{int(bad.sum())} pixels differ from the mesh_core fixture; whole-canvas SHA-256 equal: {same_hash}')
    assert (margin[bad] <= NEAR_EDGE).all() and bad.sum() <= NEAR_EDGE_CAP * CANVAS_PX
    assert same_hash or bad.any()


def test_arap_properties_on_a_triangle_made_mesh():
    import os
    from tests.warp_cases import GOLDEN
    m = np.load(os.path.join(GOLDEN, 'warp_triangle_meshes.npz'))
    V, F, bc = m['V1'].astype(np.float64), m['F1'], m['bc1']
    b = np.arange(273)
    _, E = O.arap(V, F, b, bc, return_energy=True)
    assert (np.diff(E) <= 1e-12 * E[0]).all()
    assert np.abs(O.arap(V, F, b, V[b]) - V).max() < 1e-9
