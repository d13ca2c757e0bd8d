"""GPU: ch_mask_warp_batch (csrc/mask_warp.hip) against the host oracle (tests/warp_oracle.py) on given meshes.

The ARAP bound is a measurement: profiles/warp_batch.json holds max |dU| over the fixture meshes of the first run on the
MI355X (tools/warp_time.py); the assertion is 4x that figure and never more than 0.05 px (the output is sampled at 1/32 px)."""
import json
import os

import numpy as np
import pytest

from tests import warp_oracle as O
from tests.warp_cases import (CANVAS_PX, GOLDEN, HARD_DU_PX, NEAR_EDGE, NEAR_EDGE_CAP, ROOT, boundary_band, cases, oracle,
                              triangle_meshes)

pytestmark = pytest.mark.gpu


def _du_bound():
    with open(os.path.join(ROOT, 'profiles', 'warp_batch.json')) as f:
        measured = float(json.load(f)['arap_max_dU_px'])
    return min(4.0 * measured, HARD_DU_PX)


@pytest.fixture(scope='module')
def warper(hip_lib):
    from ctrlhair_amd.warping import MaskWarper
    return MaskWarper(device='cuda:0')


def _mesh(c):
    return c['V'], c['F'], c['b'], c['bc']


@pytest.mark.parametrize('i', range(4))
def test_arap_matches_the_float64_oracle(warper, i):
    c = cases()[i]
    U = warper.warp_with_mesh(c['hair'], c['face'], *_mesh(c), return_U=True)['U'].cpu().numpy()
    ref = O.arap(*_mesh(c))
    d = float(np.linalg.norm(U - ref, axis=1).max())
    print(f'case {i}: max |U_gpu - U_oracle| = {d:.3e} px (bound {_du_bound():.3e})')
    assert d <= _du_bound()


@pytest.mark.parametrize('i', range(2))
def test_arap_matches_the_oracle_on_triangle_made_meshes(warper, i):
    c = triangle_meshes()[i]
    r = warper.warp_with_mesh(c['hair'], c['face'], *_mesh(c), return_U=True)
    ref = O.arap(*_mesh(c))
    d = float(np.linalg.norm(r['U'].cpu().numpy() - ref, axis=1).max())
    print(f'Triangle mesh {i}: max |U_gpu - U_oracle| = {d:.3e} px (bound {_du_bound():.3e})')
    assert d <= _du_bound()
    labels = O.warp_from_U(c['hair'], c['face'], c['V'], c['F'], ref.astype(np.float32))[0]
    band, diff = boundary_band(labels == 13), r['labels'].cpu().numpy() != labels
    print(f'Triangle mesh {i}: {int(diff.sum())} label pixels differ from the oracle, band {int(band.sum())} pixels')
    assert not (diff & ~band).any() and diff.sum() <= 0.02 * band.sum()


def test_gpu_raster_equals_the_reference_rasteriser_fixture(warper):
    """UV drawn on the GPU from the fixture's U against what mesh_core.cpp itself drew (rows 220..380 and the coverage)."""
    z = np.load(os.path.join(GOLDEN, 'warp_meshcore_uv.npz'))
    c = triangle_meshes()[0]
    uv = warper.warp_with_mesh(c['hair'], c['face'], *_mesh(c), U=z['U'], return_uv=True)['uv'].cpu().numpy()
    _, margin = O.render_uv(z['U'], c['V'], c['F'], return_margin=True)
    r0, r1 = z['uv_rows']
    covered = np.unpackbits(z['covered'])[:CANVAS_PX].reshape(672, 672).astype(bool)
    inner = np.zeros((672, 672), bool)
    inner[1:-2, 1:-2] = True             # the edge fix rewrites rows / columns 0, 670, 671 after the raster
    bad = ((uv[..., 0] != -1) != covered) & inner
    bad[r0:r1] |= (uv[r0:r1] != z['uv']).any(-1) & inner[r0:r1]
    print(f'{int(bad.sum())} pixels differ from the mesh_core fixture')
    assert (margin[bad] <= NEAR_EDGE).all() and bad.sum() <= NEAR_EDGE_CAP * CANVAS_PX


def test_arap_rigid_and_identity_constraints(warper):
    c = cases()[0]
    V = c['V'].astype(np.float64)
    co, si = np.cos(0.2), np.sin(0.2)
    rigid = lambda P: (P - 336.0) @ np.array([[co, si], [-si, co]]) + 336.0 + np.array([7.0, -4.0])
    U = warper.warp_with_mesh(c['hair'], c['face'], c['V'], c['F'], c['b'], rigid(V[c['b']]), return_U=True)['U'].cpu().numpy()
    d = float(np.linalg.norm(U - rigid(V), axis=1).max())
    print(f'rigid constraints: max |U - rigid(V)| = {d:.3e} px')
    assert d <= _du_bound()
    U = warper.warp_with_mesh(c['hair'], c['face'], c['V'], c['F'], c['b'], c['V'][c['b']], return_U=True)['U'].cpu().numpy()
    d = float(np.linalg.norm(U - V, axis=1).max())
    print(f'identity constraints: max |U - V| = {d:.3e} px')
    assert d <= _du_bound()


@pytest.mark.parametrize('i', range(4))
def test_raster_and_sampling_equal_the_oracle_on_a_given_U(warper, i):
    """U comes from the oracle, so no ARAP error enters: UV and labels are the oracle's bit for bit, except pixels whose
    inside test sits within 1e-6 of a triangle edge (counted, at most 0.1 % of the canvas)."""
    c = cases()[i]
    labels, uv, U = oracle(i)
    r = warper.warp_with_mesh(c['hair'], c['face'], *_mesh(c), U=U, return_uv=True)
    g_uv, g_lab = r['uv'].cpu().numpy(), r['labels'].cpu().numpy()
    _, margin = O.render_uv(U, c['V'], c['F'], return_margin=True)
    bad = (g_uv != uv).any(-1)
    print(f'case {i}: {int(bad.sum())} UV pixels differ from the oracle, {int((g_lab != labels).sum())} label pixels')
    assert (margin[bad] <= NEAR_EDGE).all()
    assert bad.sum() <= NEAR_EDGE_CAP * CANVAS_PX
    assert not ((g_lab != labels) & ~bad[80:-80, 80:-80]).any()


@pytest.mark.parametrize('i', range(4))
def test_end_to_end_labels_differ_only_on_the_boundary_band(warper, i):
    c = cases()[i]
    labels = oracle(i)[0]
    g = warper.warp_batch(c['hair'][None], c['face'][None], c['hair_lm'][None], c['face_lm'][None])[0].cpu().numpy()
    band = boundary_band(labels == 13)
    diff = g != labels
    print(f'case {i}: {int(diff.sum())} pixels differ from the oracle, band {int(band.sum())} pixels')
    assert not (diff & ~band).any()
    assert diff.sum() <= 0.02 * band.sum()
    res, extra = warper.warp(c['hair'], c['face'], c['hair_lm'], c['face_lm'])
    assert np.array_equal(res, g.astype('int')) and np.array_equal(extra['hair_mask'], (g == 13).astype('uint8'))


def test_batch_of_eight_mixed_pairs_equals_single_calls(warper):
    cs = cases()
    pairs = []
    for k in range(8):
        c = dict(cs[k % 4])
        if k == 5:                       # identical landmark sets: U = V
            c['face_lm'] = c['hair_lm']
        if k == 6:                       # one donor's hair on another face
            c['face'] = cs[0]['face']
        pairs.append(c)
    assert len({len(c['V']) for c in pairs}) > 1
    stack = lambda key: np.stack([c[key] for c in pairs])
    out = warper.warp_batch(stack('hair'), stack('face'), stack('hair_lm'), stack('face_lm')).cpu().numpy()
    for k, c in enumerate(pairs):
        one = warper.warp_batch(c['hair'][None], c['face'][None], c['hair_lm'][None], c['face_lm'][None])[0].cpu().numpy()
        assert np.array_equal(out[k], one), f'pair {k} differs between the batch and the single call'
    nohair = out[3]                      # case 3: the donor has no hair
    expect = cs[3]['face'].copy()
    expect[expect == 13] = 255
    assert not (nohair == 13).any() and np.array_equal(nohair, expect)
    # Identical landmark sets: U = V, but the reference's own arithmetic is not the identity map -- the mesh is coloured with
    # V / (W - 1) and sampled at u * W, so canvas pixel x reads the mask at x * 672 / 671, 0.12 .. 0.88 px to the lower right of
    # itself inside the image.  Both bilinear taps per axis then carry weight, and with the truncation the pixel is hair iff
    # the donor's mask is hair on the 2 x 2 block starting at it: the donor's mask comes back eroded by exactly that block.
    got = out[5] == 13
    donor = pairs[5]['hair'] == 13
    expect = donor[:-1, :-1] & donor[:-1, 1:] & donor[1:, :-1] & donor[1:, 1:]
    assert np.array_equal(got[2:-2, 2:-2], expect[2:-1, 2:-1])


def test_seventeen_pairs_are_one_batch(warper):
    """More pairs than one descriptor store launch carries (16): every pair still equals its single call."""
    cs = cases()
    singles = [warper.warp_meshes(c['hair'][None], c['face'][None], [_mesh(c)]).cpu().numpy()[0] for c in cs]
    sel = [cs[(3 * k) % 4] for k in range(17)]
    out = warper.warp_meshes(np.stack([c['hair'] for c in sel]), np.stack([c['face'] for c in sel]),
                             [_mesh(c) for c in sel]).cpu().numpy()
    for k in range(17):
        assert np.array_equal(out[k], singles[(3 * k) % 4]), f'pair {k} differs between the batch and the single call'


def test_a_collapsed_triangle_paints_only_its_own_box(warper):
    """mesh_core.cpp tests a pixel against a triangle only inside the triangle's clipped bounding box.  A triangle whose
    deformed vertices are collinear has den == 0, so u = v = 0 and the inside test passes for EVERY pixel: put first in face
    order it would paint whole tiles if the box were only used for binning.  U is given, so UV must equal the oracle's."""
    c = cases()[0]
    V, F = c['V'], c['F'].copy()
    U = oracle(0)[2].copy()
    free = (F >= 273).all(1)
    cen = V[F].mean(1)
    t = int(np.argmin(np.where(free, ((cen - np.array([308.0, 300.0])) ** 2).sum(1), np.inf)))
    F[[0, t]] = F[[t, 0]]                                  # first in face order: it wins wherever it is tested
    U[F[0, 0]], U[F[0, 1]], U[F[0, 2]] = (300.0, 300.0), (308.0, 300.0), (316.0, 300.0)
    uv, margin = O.render_uv(U, V, F, return_margin=True)
    col = (V[F[0, 0]].astype(np.float64) / 671).astype(np.float32)
    painted = (uv == col).all(-1)
    assert painted[300, 300:317].all() and painted.sum() == 17          # the oracle: row 300, x = 300..316 only
    uv = O.edge_fix(uv)
    labels = O.compose(O.sample(O.padded_mask(c['hair']), uv), c['face'])
    r = warper.warp_with_mesh(c['hair'], c['face'], V, F, c['b'], c['bc'], U=U, return_uv=True)
    g_uv, g_lab = r['uv'].cpu().numpy(), r['labels'].cpu().numpy()
    bad = (g_uv != uv).any(-1)
    print(f'{int(bad.sum())} UV pixels differ from the oracle, {int((g_lab != labels).sum())} label pixels')
    assert (margin[bad] <= NEAR_EDGE).all() and bad.sum() <= NEAR_EDGE_CAP * CANVAS_PX
    assert not ((g_lab != labels) & ~bad[80:-80, 80:-80]).any()


def test_recorded_timing_has_the_batch_cheaper_per_pair():
    """profiles/warp_batch.json (tools/warp_time.py, which itself fails otherwise): B = 16 costs less per pair than one pair."""
    with open(os.path.join(ROOT, 'profiles', 'warp_batch.json')) as f:
        j = json.load(f)
    assert j['B16_whole_call']['median'] < j['B1_whole_call']['median'] and j['batch16_cheaper_per_pair_than_single'] is True


def test_mesh_caps_are_refused(warper):
    import ctypes as C
    import torch
    from ctrlhair_amd import warping as W
    c = cases()[0]
    with pytest.raises(ValueError, match='vertices'):
        warper.warp_with_mesh(c['hair'], c['face'], np.zeros((W.MAX_V + 1, 2), np.float32), c['F'], c['b'], c['bc'])
    # and by the library itself
    z = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda:0')
    ws = torch.empty(int(warper.handle.lib.ch_mask_warp_workspace_bytes(1)), dtype=torch.uint8, device='cuda:0')
    desc = np.array([[0, W.MAX_V + 1, 0, 10, 0, 0]], np.int32)
    with pytest.raises(RuntimeError, match='supported'):
        warper.handle.call('ch_mask_warp_batch', z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                           desc.ctypes.data_as(C.c_void_p), None, z.data_ptr(), None, None, ws.data_ptr(), ws.numel(), 1, None)
