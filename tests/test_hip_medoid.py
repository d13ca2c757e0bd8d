"""The style-code medoid on the HIP library (csrc/style_medoid.hip) against the float64 difference-form oracle of tests/medoid_oracle.py.

Acceptance rule, used throughout (`check`): every row sum within 2e-5 relative of the float64 one -- the worst-case bound of the
contract is (dim + 2) * 2^-24 / 2 for the float32 squared distance (dim subtractions, dim fused multiply-adds, halved by the square
root) plus 2^-24 for sqrtf, ~1.6e-5 at dim 512 -- and the index equal to the oracle's whenever the oracle's runner-up is further than
4e-5 relative (twice the bound); otherwise any index whose float64 sum lies within 4e-5 of the minimum.  Every case but the
two-cluster one states its gap in an assert, so the escape clause cannot hide a failure there."""
import os
import pickle

import numpy as np
import pytest
import torch

from ctrlhair_amd import stylestats as SS
from tests import medoid_oracle as O

pytestmark = pytest.mark.gpu
SUM_BOUND, GAP_BOUND = 2e-5, 4e-5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'medoid_golden.npz')


@pytest.fixture(scope='module')
def sm(hip_lib):
    from ctrlhair_amd import lib
    return SS.StyleMedoid(lib.Handle(0), torch.device('cuda', 0))


def run(sm, x, offsets=None, n_split=0):
    """-> (index int32 [R], sums float64 [total], mean float32 [R, dim]) as numpy."""
    off = np.array([0, len(x)], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    index, sums, mean = sm.segments(x, off, n_split=n_split)
    torch.cuda.synchronize()
    return index.cpu().numpy(), sums.cpu().numpy(), mean.cpu().numpy()


def check(name, x, index, sums, min_gap=None):
    """The acceptance rule for one segment; min_gap: the gap the case is known to have (asserted), None = the escape clause may apply."""
    want, s64, gap = O.medoid_f64(x)
    assert sums.dtype == np.float64 and sums.shape == s64.shape
    with np.errstate(invalid='ignore', divide='ignore'):
        rel = np.where(s64 > 0, np.abs(sums - s64) / s64, np.abs(sums))
    err = float(rel.max()) if len(rel) else 0.0
    print(f'{name}: n={len(x)} dim={x.shape[1]} max |S - S64| / S64 = {err:.3e}, gap {gap:.3e}, index {index} (oracle {want})')
    assert err <= SUM_BOUND, err
    if min_gap is not None:
        assert gap > min_gap > GAP_BOUND, (gap, min_gap)
    if gap > GAP_BOUND:
        assert index == want, (index, want)
    else:
        assert 0 <= index < len(x) and s64[index] <= s64.min() * (1 + GAP_BOUND), (index, want)
    return err


@pytest.mark.parametrize('n,dim', [(1, 512), (2, 512), (3, 512), (127, 512), (128, 512), (129, 512), (257, 512), (1000, 512), (130, 4),
                                   (130, 12)])
def test_planted_medoid(sm, n, dim):
    """One tile, the tile edge on either side, several tiles, several column ranges (n = 1000 splits 8 ways); dim below and off the
    16-wide K slab.  The planted row wins by ~36 % at dim 512 (3.9 % at dim 4, 12 % at dim 12)."""
    x, m = O.planted(n, dim, seed=n)
    index, sums, _ = run(sm, x)
    if n == 1:
        assert index[0] == 0 and sums[0] == 0.0
        return
    if n == 2:                  # d_01 and d_10 are the same float32 operations: an exact tie, the first index wins
        assert sums[0] == sums[1] and index[0] == 0
        check('planted', x, int(index[0]), sums)
        return
    check('planted', x, int(index[0]), sums, min_gap=0.03 if dim < 512 else 0.3)
    assert index[0] == m


def test_saturated_cluster(sm):
    """130 codes of 0.79 + 1e-3 N(0,1): the reference's Gram arithmetic is 3.6 % off and picks another code (asserted here and in
    tests/test_stylestats.py); the difference form must pick the float64 medoid, whose runner-up is 8.9e-3 away."""
    x = O.saturated()
    index, sums, _ = run(sm, x)
    check('saturated', x, int(index[0]), sums, min_gap=5e-3)
    assert O.reference_f32(x)[0] != index[0]


def test_ties_and_zeros(sm):
    x = np.repeat(O.tanh_codes(1, 512, seed=5), 200, axis=0)
    index, sums, _ = run(sm, x)
    assert index[0] == 0 and (sums == 0.0).all()                     # d_ij = sqrt(sum (x - x)^2) = 0 exactly
    x, m = O.planted(150, 512, seed=6)
    twin = (m + 77) % 150
    x[twin] = x[m]
    index, sums, _ = run(sm, x)
    assert sums[m] == sums[twin] and index[0] == min(m, twin)
    s64 = O.row_sums_f64(x)
    others = np.delete(s64, [m, twin])
    assert (others.min() - s64[m]) / s64[m] > 0.3                    # the twins win by far: only the tie-break decides
    assert (np.abs(sums - s64) <= SUM_BOUND * s64).all()


RAGGED = (0, 1, 2, 129, 300, 5, 0, 128, 257, 64, 3, 640, 127, 1, 200, 33, 0, 130, 96)


def test_ragged_segments_alone_and_together(sm):
    """R = 19 segments in one call: every segment's sums bit-equal to the segment run alone, a second run bit-equal to the first."""
    assert len(RAGGED) == 19
    off = np.concatenate([[0], np.cumsum(RAGGED)]).astype(np.int64)
    x = O.tanh_codes(int(off[-1]), 512, seed=19)
    planted_at = {}
    for r, n in enumerate(RAGGED):
        if n >= 3:
            seg, m = O.planted(n, 512, seed=100 + r)
            x[off[r]:off[r + 1]] = seg
            planted_at[r] = m
    index, sums, mean = run(sm, x, off)
    index2, sums2, mean2 = run(sm, x, off)
    assert np.array_equal(index, index2) and np.array_equal(sums, sums2) and np.array_equal(mean, mean2)
    for r, n in enumerate(RAGGED):
        seg = x[off[r]:off[r + 1]]
        if n == 0:
            assert index[r] == -1 and (mean[r] == 0).all()
            continue
        i1, s1, m1 = run(sm, seg)
        assert np.array_equal(sums[off[r]:off[r + 1]], s1) and index[r] == i1[0] and np.array_equal(mean[r], m1[0])
        if n >= 3:
            check(f'segment {r}', seg, int(index[r]), s1, min_gap=0.2)
            assert index[r] == planted_at[r]
        else:
            assert index[r] == 0


def test_forced_split(sm):
    """n = 300 is three column tiles: 1, 2 or 3 column ranges give the same index and sums equal to float64 rounding; auto is one of
    them bit for bit; a split count beyond the tiles is clamped."""
    x, m = O.planted(300, 512, seed=300)
    runs = {k: run(sm, x, n_split=k) for k in (1, 2, 3)}
    for k, (index, sums, _) in runs.items():
        check(f'n_split={k}', x, int(index[0]), sums, min_gap=0.3)
        assert index[0] == m
        assert np.abs(sums - runs[1][1]).max() <= 1e-12 * runs[1][1].min()
    auto = run(sm, x)
    assert any(np.array_equal(auto[1], r[1]) and np.array_equal(auto[0], r[0]) for r in runs.values())
    assert np.array_equal(run(sm, x, n_split=50)[1], runs[3][1])


def test_mean(sm):
    off = np.array([0, 1, 1, 301, 1301], np.int64)
    x = O.tanh_codes(1301, 512, seed=77)
    _, _, mean = run(sm, x, off)
    for r in range(4):
        seg = x[off[r]:off[r + 1]].astype(np.float64)
        want = seg.mean(axis=0).astype(np.float32) if len(seg) else np.zeros(512, np.float32)
        assert np.abs(mean[r].astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -24
    assert np.array_equal(mean[0], x[0])


def test_two_clusters_escape_clause(sm):
    """70 + 60 codes at +-0.7 with 1e-3 spread: the best two row sums are 2.8e-5 apart, inside what float32 distances can resolve in the
    worst case.  Only the escape clause is exercised: sums within the bound, the index among the float64 near-minima."""
    x = O.two_clusters()
    _, s64, gap = O.medoid_f64(x)
    assert gap < GAP_BOUND, gap
    index, sums, _ = run(sm, x)
    check('two clusters', x, int(index[0]), sums)


def test_bad_arguments_are_rejected(sm):
    x = O.tanh_codes(8, 512, seed=1)
    with pytest.raises(ValueError):
        sm.segments(x[:, :510], np.array([0, 8], np.int64))          # dim not a multiple of 4
    with pytest.raises(ValueError):
        sm.segments(x, np.array([0, 9], np.int64))
    d = torch.from_numpy(x).cuda()
    off = np.array([0, 8], np.int64)
    out = torch.empty(600, dtype=torch.float32, device='cuda')
    with pytest.raises(RuntimeError, match='workspace'):
        sm.handle.call('ch_style_medoid', d.data_ptr(), off.ctypes.data, 1, 512, 0, out.data_ptr(), None, out.data_ptr(), out.data_ptr(), 16,
                       None)


def test_golden_rows(sm):
    """median_style_codes on the golden input returns the rows the reference's own script recorded, exactly."""
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    codes = O.golden_codes()
    res = sm.median_style_codes(codes)
    packaged = SS.load_mean_style_code()
    assert np.array_equal(res['count'], g['presence'].sum(axis=0)) and np.array_equal(res['index'], g['index'])
    _, _, mean64, _ = O.median_rows_f64(codes)
    for j in range(19):
        if g['written'][j]:
            assert np.array_equal(res['median'][j], g['rows'][j])
            assert np.abs(res['mean'][j] - mean64[j].astype(np.float32)).max() <= 2.0 ** -24
        else:
            assert res['index'][j] == -1 and np.array_equal(res['median'][j], packaged['median'][j])
            assert np.array_equal(res['mean'][j], packaged['mean'][j])
    as_dict = sm.median_style_codes({f'k{i}': codes[i] for i in range(len(codes))})
    assert as_dict['keys'][as_dict['index'][0]] == f'k{g["index"][0]}' and np.array_equal(as_dict['median'], res['median'])


def test_dataset_job_and_loader_end_to_end(hip_lib, tmp_path, capsys):
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.hair_editor import HairEditor
    root = str(tmp_path)
    N, absent = 40, 4
    codes = np.stack([O.tanh_codes(19, 512, seed=4000 + i) for i in range(N)])
    pres = P._rng(41, 'medoid.e2e').random((N, 19)) < 0.8
    pres[:, absent] = False
    codes[~pres] = 0.0
    for j in range(19):                                            # a planted medoid per region: the choice is never close
        rows = np.nonzero(pres[:, j])[0]
        if len(rows) >= 3:
            mu = codes[rows, j].astype(np.float64).mean(axis=0)
            codes[rows[j % len(rows)], j] = (mu + 0.1 * (codes[rows[j % len(rows)], j] - mu)).astype(np.float32)
    with open(os.path.join(root, 'sean_code_dict.pkl'), 'wb') as f:
        pickle.dump({f'ds___{i:05d}': codes[i] for i in range(N)}, f)
    D.main(['median', root, '--tree', os.path.join(root, 'styles_test')])
    printed = capsys.readouterr().out
    index, count, mean64, gaps = O.median_rows_f64(codes)
    assert (gaps[count > 1] > 0.1).all(), gaps
    path = os.path.join(root, 'mean_style_code.npz')
    got = SS.load_mean_style_code(path)
    packaged = SS.load_mean_style_code()
    for j in range(19):
        if count[j]:
            assert np.array_equal(got['median'][j], codes[index[j], j]), j
            assert np.abs(got['mean'][j] - mean64[j].astype(np.float32)).max() <= 2.0 ** -24
            assert f'ds___{index[j]:05d}' in printed
        else:
            assert np.array_equal(got['median'][j], packaged['median'][j])
    assert count[absent] == 0
    tree = SS.read_reference_tree(os.path.join(root, 'styles_test'))
    assert np.array_equal(tree['median'], got['median']) and np.array_equal(tree['mean'], got['mean'])

    default = HairEditor(True, True, weights='procedural', device=0)
    custom = HairEditor(True, True, weights='procedural', device=0, models=default.models, mean_style_code=path)
    rows = custom.load_average_feature()
    assert all(np.array_equal(rows[str(j)]['ACE'].cpu().numpy(), got['median'][j]) for j in range(19))
    rows = default.load_average_feature()
    assert all(np.array_equal(rows[str(j)]['ACE'].cpu().numpy(), packaged['median'][j]) for j in range(19))
    labels = P.blocky_labels(1, 256, grid=8)
    region = int(np.bincount(labels.reshape(-1), minlength=19)[1:].argmax()) + 1     # a region the label map shows, code absent
    assert region != absent
    c = P.style_codes(1)
    c[0, region] = 0.0
    noise = torch.from_numpy(P.noise_planes(1, 256)).to(default.device)
    a = default.gen_imgs(c, labels, noise=noise)
    b = custom.gen_imgs(c, labels, noise=noise)
    a2 = default.gen_imgs(c, labels, noise=noise)
    torch.cuda.synchronize()
    assert torch.equal(a, a2) and not torch.equal(a, b)
    assert float((a - b).abs().max()) > 1e-3
