"""GPU: ch_delaunay_batch (csrc/delaunay.hip), ch_mask_warp_batch_dev and warp_batch(mesher='device').

Every mesh is checked by the exact integer checker of tests/delaunay_oracle.py: there is no tolerance in the meshing tests.
The end-to-end criterion and the ARAP bound are those of tests/test_hip_warp.py (profiles/warp_batch.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import delaunay_oracle as D
from tests import warp_oracle as O
from tests.warp_cases import ROOT, boundary_band, cases

pytestmark = pytest.mark.gpu

G = float(D.GRID)
# Quadruples (a, b, c, d) in grid units, (a, b, c) counter-clockwise, on which the plain float64 incircle determinant has the wrong
# sign while the exact one is not zero: a and b are a few grid units apart, c and d far away, so the determinant (the product of
# the side lengths times d's distance from the circle) is smaller than the rounding of its 2^120-sized terms.  Recorded from a
# seeded search; every coordinate is a float32 multiple of 2^-20.
HARD = [
    [(4194360, 4194359), (4194363, 4194356), (895544768, 644572480), (303021952, 945424832)],
    [(4194305, 4194323), (4194308, 4194322), (517325696, 340298752), (310457472, 720937152)],
    [(4194308, 4194332), (4194311, 4194332), (385997952, 881267200), (475341888, 749724416)],
    [(4194339, 4194314), (4194340, 4194312), (570936064, 559539904), (688957760, 467024896)],
    [(4194309, 4194311), (4194312, 4194308), (844515840, 405621504), (367118080, 847092928)],
    [(4194330, 4194306), (4194331, 4194304), (812755712, 712049472), (1049963968, 335764800)],
]


@pytest.fixture(scope='module')
def warper():
    from ctrlhair_amd.warping import MaskWarper
    return MaskWarper(device='cuda:0')


def f32(points):
    V = np.asarray(points, np.float64).astype(np.float32)
    assert np.array_equal(V.astype(np.float64), np.asarray(points, np.float64))
    return V


def small_sets():
    ring = [(10, 5), (8, 9), (2, 9), (0, 5), (2, 1), (8, 1)]                       # six points on the circle of radius 5 about (5, 5)
    return {
        'triangle': f32([(0, 0), (1, 0), (0, 1)]),
        'unit square': f32([(0, 0), (1, 0), (1, 1), (0, 1)]),
        'lattice 5x5': f32([(x, y) for y in range(5) for x in range(5)]),
        'lattice 3x3 + hull midpoints': f32([(2 * x, 2 * y) for y in range(3) for x in range(3)] + [(1, 0), (3, 0), (0, 1), (4, 3), (3, 4)]),
        'ring of six around a seventh': f32(ring + [(5, 5)]),
        'empty ring of six and an outsider': f32([(40, 5)] + ring),
        'shifted lattice, reversed order': f32([(100.5 + 13.6875 * x, 7.25 + 13.6875 * y) for y in range(4) for x in range(6)][::-1]),
    }


def random_grid_points(n, seed):
    """n distinct random float32 points of [0, 1024)^2 on the 2^-20 grid (every float32 >= 8 is on it; below 8 they are rounded)."""
    rng = np.random.default_rng(seed)
    V = (np.rint(rng.uniform(0, 1024, (n + 64, 2)).astype(np.float32).astype(np.float64) * G) / G).astype(np.float32)
    V = V[np.sort(np.unique(V, axis=0, return_index=True)[1])][:n]
    assert len(V) == n and (V < 1024).all()
    return V


def test_smallest_shapes_pass_the_exact_checker(warper):
    sets = small_sets()
    res = warper.triangulate(list(sets.values()))
    for (name, V), (F, st) in zip(sets.items(), res):
        assert st == 0, name
        h, _ = D.check(V, F)
        print(f'{name}: n = {len(V)}, h = {h}, {len(F)} triangles')
    assert len(res[0][0]) == 1 and len(res[1][0]) == 2 and len(res[2][0]) == 32
    ring = res[5][0]                                     # the empty six-gon is fanned from its smallest index
    assert sum(1 for r in ring if r[0] == 1) == 4


def test_degenerate_sets_report_a_status_and_write_no_triangles(warper):
    from ctrlhair_amd import warping as W
    line = f32([(3 * k, 2 * k) for k in range(9)])
    dup = f32([(0, 0), (4, 0), (0, 4), (4, 0), (7, 7)])
    offgrid = np.array([(0, 0), (4, 0), (2.0 + 2.0 ** -21, 4)], np.float32)
    outside = np.array([(0, 0), (4, 0), (1024, 4)], np.float32)
    nan = np.array([(0, 0), (4, 0), (np.nan, 4)], np.float32)
    res = warper.triangulate([line, dup, offgrid, outside, nan, f32([(0, 0), (1, 1)]), np.zeros((W.MAX_V + 1, 2), np.float32)])
    assert [st for _, st in res] == [4, 3, 2, 2, 2, 1, 1]
    assert all(len(F) == 0 for F, _ in res)


def test_cap_sized_random_set(warper):
    from ctrlhair_amd import warping as W
    V = random_grid_points(W.MAX_V, 1)
    (F, st), = warper.triangulate([V])
    assert st == 0
    h, _ = D.check(V, F)
    print(f'n = {len(V)}: h = {h}, {len(F)} triangles')


def naive_incircle(a, b, c, d):
    a, b, c, d = [np.array(p, np.float64) for p in (a, b, c, d)]
    adx, ady, bdx, bdy, cdx, cdy = a[0] - d[0], a[1] - d[1], b[0] - d[0], b[1] - d[1], c[0] - d[0], c[1] - d[1]
    return float((adx * adx + ady * ady) * (bdx * cdy - cdx * bdy) + (bdx * bdx + bdy * bdy) * (cdx * ady - adx * cdy)
                 + (cdx * cdx + cdy * cdy) * (adx * bdy - bdx * ady))


def test_sets_on_which_float64_alone_decides_wrongly(warper):
    wrong = 0
    sets = []
    rng = np.random.default_rng(3)
    for q in HARD:
        e, f = D.incircle(*q), naive_incircle(*q)
        wrong += e != 0 and (f == 0 or (f > 0) != (e > 0))
        others = np.stack([rng.choice(np.arange(1, 1 << 16), 12, replace=False), rng.choice(np.arange(1 << 10, 1 << 16), 12, replace=False)], 1)
        sets.append(f32(np.concatenate([np.array(q, np.float64), others.astype(np.float64) * (1 << 14)]) / G))
    assert wrong >= 1, 'the recorded quadruples no longer defeat the float64 determinant: the test would prove nothing'
    print(f'{wrong} of {len(HARD)} quadruples have the wrong float64 sign')
    for V, (F, st) in zip(sets, warper.triangulate(sets)):
        assert st == 0 and len(V) == 16
        D.check(V, F)


@pytest.fixture(scope='module')
def fixture_meshes(warper):
    return warper.triangulate([c['V'] for c in cases()])


@pytest.mark.parametrize('i', range(4))
def test_fixture_meshes_differ_from_qhull_only_inside_cocircular_groups(fixture_meshes, i):
    c = cases()[i]
    F, st = fixture_meshes[i]
    assert st == 0
    h, uniq_dev = D.check(c['V'], F, want_unique=True)
    _, uniq_host = D.check(c['V'], c['F'], want_unique=True)
    assert h == 196 and len(F) == len(c['F'])
    dev, host = {tuple(r) for r in F.tolist()}, {tuple(r) for r in c['F'].tolist()}
    print(f'case {i}: {len(F)} triangles, {len(uniq_dev)} unique, {len(dev & host)} shared with the Qhull mesh')
    assert uniq_dev <= host and uniq_host <= dev


def test_seventeen_mixed_sets_are_one_call_and_equal_their_single_calls(warper):
    from ctrlhair_amd import warping as W
    cs = cases()
    sets = [cs[k % 4]['V'] if k % 3 == 0 else random_grid_points(3 + (k * 47) % 600, 10 + k) for k in range(17)]
    sets[2] = cs[2]['V']                                 # 806 points
    sets[1] = random_grid_points(3, 5)
    sets[8] = f32([(k, k) for k in range(40)])           # a failed set in the middle
    assert {len(V) for V in sets} >= {3, 806}
    batch = warper.triangulate(sets)
    assert batch[8][1] == 4 and len(batch[8][0]) == 0
    for k, V in enumerate(sets):
        (F, st), = warper.triangulate([V])
        assert st == batch[k][1] and np.array_equal(F, batch[k][0]), f'set {k} differs between the batch and the single call'
        if k != 8:
            assert st == 0
            D.check(V, F)


def _dev_call(warper, cs, desc, return_U=False):
    """ch_mask_warp_batch_dev with packed host-made meshes and the given descriptors uploaded."""
    import torch
    dev = warper.device
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    B = len(cs)
    V, F = up(np.concatenate([c['V'] for c in cs])), up(np.concatenate([c['F'] for c in cs]))
    b, bc = up(np.concatenate([c['b'] for c in cs])), up(np.concatenate([c['bc'] for c in cs]))
    hair, face = up(np.stack([c['hair'] for c in cs])), up(np.stack([c['face'] for c in cs]))
    out = torch.zeros(B, 512, 512, dtype=torch.uint8, device=dev)
    U = torch.zeros(len(V), 2, dtype=torch.float32, device=dev) if return_U else None
    need = int(warper.handle.lib.ch_mask_warp_workspace_bytes(B))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    warper.handle.call('ch_mask_warp_batch_dev', hair.data_ptr(), face.data_ptr(), V.data_ptr(), F.data_ptr(), b.data_ptr(), bc.data_ptr(),
                       up(desc.astype(np.int32)).data_ptr(), None, out.data_ptr(), None, U.data_ptr() if return_U else None, ws.data_ptr(),
                       need, B, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), (U.cpu().numpy() if return_U else None)


def _host_desc(cs):
    desc = np.zeros((len(cs), 6), np.int32)
    vo = fo = bo = 0
    for i, c in enumerate(cs):
        desc[i] = (vo, len(c['V']), fo, len(c['F']), bo, len(c['b']))
        vo, fo, bo = vo + len(c['V']), fo + len(c['F']), bo + len(c['b'])
    return desc


@pytest.fixture(scope='module')
def host_call(warper):
    cs = cases()
    r = warper.warp_meshes(np.stack([c['hair'] for c in cs]), np.stack([c['face'] for c in cs]),
                           [(c['V'], c['F'], c['b'], c['bc']) for c in cs], return_U=True)
    return r['labels'].cpu().numpy(), np.concatenate([u.cpu().numpy() for u in r['U']])


def test_device_descriptors_give_the_bytes_of_the_host_call(warper, host_call):
    cs = cases()
    labels, U = _dev_call(warper, cs, _host_desc(cs), return_U=True)
    assert np.array_equal(labels, host_call[0])
    assert np.array_equal(U.view(np.int32), host_call[1].view(np.int32))


def _identity_labels(c):
    """What an undeformed pair is: UV = pixel / 671 (float32(np.linspace)), then the oracle's edge fix, sampling and composition."""
    lin = (np.arange(672, dtype=np.float64) * (1.0 / 671)).astype(np.float32)
    lin[671] = 1.0
    uv = np.stack(np.broadcast_arrays(lin[None, :], lin[:, None]), -1).astype(np.float32)
    return O.compose(O.sample(O.padded_mask(c['hair']), O.edge_fix(uv)), c['face'])


@pytest.mark.parametrize('bad', ['n_f = 0', 'n_f over the cap', 'n_v over the cap', 'negative offset'])
def test_a_refused_descriptor_renders_that_pair_undeformed(warper, host_call, bad):
    from ctrlhair_amd import warping as W
    cs = cases()
    desc = _host_desc(cs)
    k = 1
    if bad == 'n_f = 0':
        desc[k, 3] = 0
    elif bad == 'n_f over the cap':
        desc[k, 3] = W.MAX_F + 1
    elif bad == 'n_v over the cap':
        desc[k, 1] = W.MAX_V + 1
    else:
        desc[k, 2] = -3
    labels, _ = _dev_call(warper, cs, desc)
    for i in range(4):
        if i != k:
            assert np.array_equal(labels[i], host_call[0][i]), f'pair {i} changed'
    assert np.array_equal(labels[k], _identity_labels(cs[k]))


def _du_bound():
    from tests.warp_cases import HARD_DU_PX
    with open(os.path.join(ROOT, 'profiles', 'warp_batch.json')) as f:
        return min(4.0 * float(json.load(f)['arap_max_dU_px']), HARD_DU_PX)


@pytest.mark.parametrize('i', range(4))
def test_device_mesher_end_to_end_equals_the_oracle_on_the_device_made_mesh(warper, i):
    c = cases()[i]
    g = warper.warp_batch(c['hair'][None], c['face'][None], c['hair_lm'][None], c['face_lm'][None], mesher='device')[0].cpu().numpy()
    assert int(warper.last_mesh_status[0]) == 0
    m = warper.last_mesh
    n, nf = int(m['counts'][0]), int(m['n_f'][0])
    V, F = m['V'][:n].cpu().numpy(), m['F'][0, :nf].cpu().numpy()
    assert np.array_equal(V.view(np.int32), c['V'].view(np.int32))
    D.check(V, F)
    U = warper.warp_with_mesh(c['hair'], c['face'], V, F, c['b'], c['bc'], return_U=True)['U'].cpu().numpy()
    labels, _, ref_U = O.warp(c['hair'], c['face'], V, F, c['b'], c['bc'])
    d = float(np.linalg.norm(U - ref_U, axis=1).max())
    print(f'case {i}: max |U_gpu - U_oracle| on the device-made mesh = {d:.3e} px (bound {_du_bound():.3e})')
    assert d <= _du_bound()
    band, diff = boundary_band(labels == 13), g != labels
    print(f'case {i}: {int(diff.sum())} pixels differ from the oracle, band {int(band.sum())} pixels')
    assert not (diff & ~band).any()
    assert diff.sum() <= 0.02 * band.sum()
    res, extra = warper.warp(c['hair'], c['face'], c['hair_lm'], c['face_lm'], mesher='device')
    assert np.array_equal(res, g.astype('int')) and np.array_equal(extra['hair_mask'], (g == 13).astype('uint8'))


def test_device_mesher_batch_of_eight_equals_single_calls(warper):
    cs = cases()
    pairs = []
    for k in range(8):
        c = dict(cs[k % 4])
        if k == 5:
            c['face_lm'] = c['hair_lm']
        if k == 6:
            c['face'] = cs[0]['face']
        pairs.append(c)
    stack = lambda key: np.stack([c[key] for c in pairs])
    out = warper.warp_batch(stack('hair'), stack('face'), stack('hair_lm'), stack('face_lm'), mesher='device').cpu().numpy()
    assert int(warper.last_mesh_status.abs().sum()) == 0
    for k, c in enumerate(pairs):
        one = warper.warp_batch(c['hair'][None], c['face'][None], c['hair_lm'][None], c['face_lm'][None], mesher='device')[0].cpu().numpy()
        assert np.array_equal(out[k], one), f'pair {k} differs between the batch and the single call'


def test_default_mesher_is_the_host_one(warper):
    c = cases()[0]
    a = warper.warp_batch(c['hair'][None], c['face'][None], c['hair_lm'][None], c['face_lm'][None]).cpu().numpy()
    b = warper.warp_batch(c['hair'][None], c['face'][None], c['hair_lm'][None], c['face_lm'][None], mesher='host').cpu().numpy()
    r = warper.warp_meshes(c['hair'][None], c['face'][None], [(c['V'], c['F'], c['b'], c['bc'])]).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, r)
    with pytest.raises(ValueError, match='mesher'):
        warper.warp_batch(c['hair'][None], c['face'][None], c['hair_lm'][None], c['face_lm'][None], mesher='gpu')


def test_argument_errors(warper):
    import torch
    lib, h = warper.handle.lib, warper.handle._h
    z = torch.zeros(1 << 20, dtype=torch.uint8, device='cuda:0')
    p = z.data_ptr()
    vd = np.array([[0, 3]], np.int32)
    vdp = vd.ctypes.data_as(C.c_void_p)
    need = int(lib.ch_delaunay_workspace_bytes(1))
    assert need > 0 and int(lib.ch_delaunay_workspace_bytes(0)) == 0
    Vt = torch.tensor([[0, 0], [1, 0], [0, 1]], dtype=torch.float32, device='cuda:0')
    Ft = torch.zeros(4096 * 3, dtype=torch.int32, device='cuda:0')
    nf, st = torch.zeros(1, dtype=torch.int32, device='cuda:0'), torch.ones(1, dtype=torch.int32, device='cuda:0')
    dws = torch.empty(need, dtype=torch.uint8, device='cuda:0')
    V, F, n, s, w = Vt.data_ptr(), Ft.data_ptr(), nf.data_ptr(), st.data_ptr(), dws.data_ptr()
    assert lib.ch_delaunay_batch(h, V, vdp, F, n, s, w, need, 1, None) == 0
    torch.cuda.synchronize()
    assert int(nf[0]) == 1 and int(st[0]) == 0 and Ft[:3].tolist() == [0, 1, 2]
    for args in [(None, vdp, F, n, s, w, need, 1), (V, None, F, n, s, w, need, 1), (V, vdp, None, n, s, w, need, 1),
                 (V, vdp, F, None, s, w, need, 1), (V, vdp, F, n, None, w, need, 1), (V, vdp, F, n, s, None, need, 1),
                 (V, vdp, F, n, s, w, need, 0), (V, vdp, F, n, s, w, need - 1, 1)]:
        assert lib.ch_delaunay_batch(h, *args, None) == 1          # CH_ERR_ARG
        assert b'ch_delaunay_batch' in lib.ch_last_error(h)
    neg = np.array([[-1, 3]], np.int32)
    assert lib.ch_delaunay_batch(h, V, neg.ctypes.data_as(C.c_void_p), F, n, s, w, need, 1, None) == 1
    wneed = int(lib.ch_mask_warp_workspace_bytes(1))
    ws = torch.empty(wneed, dtype=torch.uint8, device='cuda:0')
    ok = (p, p, p, p, p, p, p, None, p, None, None, ws.data_ptr(), wneed, 1)
    for k in (0, 1, 2, 3, 6, 8, 11):
        a = list(ok)
        a[k] = None
        assert lib.ch_mask_warp_batch_dev(h, *a, None) == 1
    assert lib.ch_mask_warp_batch_dev(h, *ok[:12], wneed - 1, 1, None) == 1
    assert lib.ch_mask_warp_batch_dev(h, *ok[:13], 0, None) == 1
    assert b'ch_mask_warp_batch_dev' in lib.ch_last_error(h)
    torch.cuda.synchronize()


def test_recorded_timing_has_the_device_mesher_faster_per_pair():
    """profiles/delaunay_batch.json (tools/mesh_time.py, which itself fails otherwise): at B = 16 the whole warp_batch call
    with the device mesher is faster per pair than with the host mesher by more than the spread of both."""
    with open(os.path.join(ROOT, 'profiles', 'delaunay_batch.json')) as f:
        j = json.load(f)
    c, d = j['B16']['warp_batch_host_mesher_ms_per_pair'], j['B16']['warp_batch_device_mesher_ms_per_pair']
    assert d['median'] < c['median'] and d['max'] < c['min'] and j['device_mesher_faster_at_B16'] is True
