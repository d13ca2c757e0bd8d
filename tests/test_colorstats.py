"""Hair colour statistics, host side (no GPU): the numpy re-statement of the reference scripts (tests/colorstats_ref.py)
against brute force, and the finishing functions of ctrlhair_amd.colorstats (exact from int64 sums) against it."""
import pickle

import numpy as np
import pytest

from ctrlhair_amd import colorstats as CS
from ctrlhair_amd import hostutil as U
from tests import colorstats_ref as R


def test_ellipse_rows():
    assert CS.ellipse_half_widths(19).tolist() == [0, 4, 6, 7, 7, 8, 8, 9, 9, 9, 9, 9, 8, 8, 7, 7, 6, 4, 0]
    assert CS.ellipse_half_widths(13).tolist() == [0, 3, 4, 5, 6, 6, 6, 6, 6, 5, 4, 3, 0]     # c_hw13 of poisson_kernels.hip
    assert CS.ellipse_half_widths(5).tolist() == [0, 2, 2, 2, 0]                             # c_hw5
    assert CS.ellipse_half_widths(1).tolist() == [0]
    for bad in (0, 4, -3):
        with pytest.raises(ValueError):
            CS.ellipse_half_widths(bad)


@pytest.mark.parametrize('ksize', [1, 3, 5, 13, 19])
def test_reference_erosion_matches_brute_force(ksize):
    rng = np.random.default_rng(ksize)
    for shape in ((23, 31), (40, 17)):
        m = (rng.random(shape) < 0.85).astype(np.uint8)
        m[5:9, :] = 1
        assert np.array_equal(R.erode(m, ksize), R.erode_brute(m, ksize))
    ones = np.ones((12, 12), np.uint8)
    assert R.erode(ones, ksize).all()                         # the border never erodes
    line = np.zeros((15, 15), np.uint8)
    line[7, :] = 1
    assert R.erode(line, ksize).any() == (ksize == 1)


def _points(rng, n):
    p = rng.integers(0, 256, (n, 3)).astype(np.uint8)
    p[:, 1] = (p[:, 0] // 2 + p[:, 1] // 4).astype(np.uint8)
    return p


def _sums_of_points(p):
    return R.sums(p.reshape(1, -1, 3), np.ones((1, len(p)), np.uint8))


@pytest.mark.parametrize('n', [0, 1, 5, 6, 7, 100, 5000])
def test_finishing_matches_restatement(n):
    rng = np.random.default_rng(n + 11)
    p = _points(rng, n)
    s = _sums_of_points(p)
    R.assert_moments_close(CS.rgb_stat_from_sums(s), R.rgb_stat(p))
    if n:
        assert np.array_equal(CS.mean_from_sums(s), p.mean(0))        # bit for bit
    else:
        assert np.isnan(CS.rgb_stat_from_sums(s)[3]).all()
    got, ref = CS.color_var_from_sums(s), R.color_var(p)
    assert (got is None) == (ref is None) == (n <= 5)
    if got is None:
        return
    assert sorted(got) == ['var_hsv', 'var_pca', 'var_pca_comp', 'var_pca_mean', 'var_rgb']
    np.testing.assert_allclose(got['var_rgb'], ref['var_rgb'], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got['var_hsv'], ref['var_hsv'], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got['var_pca'], ref['var_pca'], rtol=1e-10)
    assert np.array_equal(got['var_pca_mean'], ref['var_pca_mean'])
    assert got['var_pca_comp'].shape == (2, 3)
    ev = ref['eigvals']
    if ev[0] - ev[1] > 1e-6 * ev[0] and ev[1] - ev[2] > 1e-6 * ev[0]:
        np.testing.assert_allclose(got['var_pca_comp'], ref['var_pca_comp'], atol=1e-8)


def test_uniform_colour():
    p = np.tile(np.array([[200, 10, 77]], np.uint8), (50, 1))
    s = _sums_of_points(p)
    m = CS.rgb_stat_from_sums(s)
    assert np.array_equal(m[0], [200.0, 10.0, 77.0]) and all((mk == 0).all() for mk in m[1:])
    v = CS.color_var_from_sums(s)
    assert (v['var_rgb'] == 0).all() and (v['var_hsv'] == 0).all() and v['var_pca'] == 0.0


def test_int64_bound_all_hair_1024():
    """A 1024^2 image of all-255 hair: the largest sums fit in int64 and the moments come out exact."""
    n = 1024 * 1024
    s = np.zeros(CS.NSTAT, np.int64)
    s[0] = n
    s[1:16] = [255 * n] * 3 + [255 ** 2 * n] * 3 + [255 ** 3 * n] * 3 + [255 ** 4 * n] * 3 + [255 ** 2 * n] * 3
    assert 255 ** 4 * n < 2 ** 63 and s[10] == 255 ** 4 * n
    s[20], s[21] = 255 * n, 255 * 255 * n                     # V; H = S = 0 for grey
    m = CS.rgb_stat_from_sums(s)
    assert np.array_equal(m[0], [255.0] * 3) and all((mk == 0).all() for mk in m[1:])
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
    img[:64] = 255
    s = R.sums(img, np.ones((1024, 1024), np.uint8))
    p = img.reshape(-1, 3)
    # numpy's .mean(axis=0) of an [n,3] array sums row after row: at n = 2^20 the reference's own moments carry ~1e-11
    # relative rounding error, while the finish from integer sums is exact
    R.assert_moments_close(CS.rgb_stat_from_sums(s), R.rgb_stat(p), tol=1e-10)
    np.testing.assert_allclose(CS.color_var_from_sums(s)['var_rgb'], (p / 255).var(0), rtol=1e-10)


def test_pca_matches_sklearn():
    PCA = pytest.importorskip('sklearn.decomposition').PCA
    rng = np.random.default_rng(3)
    for n in (6, 40, 3000):
        base = rng.normal(size=(n, 1)) * np.array([[60.0, 30.0, -20.0]]) + rng.normal(size=(n, 3)) * np.array([[8.0, 4.0, 2.0]])
        p = np.clip(base + 128, 0, 255).astype(np.uint8)
        got = CS.color_var_from_sums(_sums_of_points(p))
        pca = PCA(n_components=2).fit(p)
        np.testing.assert_allclose(got['var_pca'], pca.transform(p)[:, 0].std(), rtol=1e-9)
        np.testing.assert_allclose(got['var_pca_mean'], pca.mean_, rtol=1e-13)
        np.testing.assert_allclose(got['var_pca_comp'], pca.components_, atol=1e-7)        # clear eigengap: signs agree


def test_hsv_table_roundtrip_through_dist_translation(tmp_path):
    rng = np.random.default_rng(9)
    d = {f'ds___{i:03d}': R.rgb_stat(_points(rng, int(rng.integers(0, 40)))) for i in range(30)}
    d['ds___nohair'] = R.rgb_stat(np.zeros((0, 3), np.uint8))
    t = CS.hsv_table(d)
    assert t.dtype == np.uint8 and t.shape == (31, 3)
    assert np.array_equal(t, R.hsv_table(d))
    assert all((np.diff(t[:, j].astype(int)) >= 0).all() for j in range(3))
    with open(tmp_path / 'hsv_stat_dict_ordered.pkl', 'wb') as f:
        pickle.dump(t, f)
    dt = U.DistTranslation(root=str(tmp_path))
    assert np.array_equal(dt.cols_hsv, t)
    v = int(t[15, 2])
    g = dt.val_to_gaussian(2, v)
    assert abs(int(dt.gaussian_to_val(2, g)) - v) <= int(t[-1, 2]) - int(t[0, 2])
    # a Backend pointed at the table uses it (ui/backend.py: DistTranslation(hsv_table))
    assert not np.array_equal(U.DistTranslation(root=str(tmp_path / 'missing')).cols_hsv, t)


def test_dataset_color_jobs_reject_unknown_and_non_square(tmp_path):
    from ctrlhair_amd import dataset as D
    with pytest.raises(ValueError):
        D.hair_color_stats(None, str(tmp_path), str(tmp_path), str(tmp_path), 'ds', jobs=('hls',))
    (tmp_path / 'img').mkdir()
    (tmp_path / 'label').mkdir()
    from PIL import Image
    Image.fromarray(np.zeros((20, 30, 3), np.uint8)).save(tmp_path / 'img' / 'a.png')
    D.write_label_png(str(tmp_path / 'label' / 'a.png'), np.zeros((20, 30), np.uint8))
    with pytest.raises(ValueError, match='square'):
        D.hair_color_stats(None, str(tmp_path / 'img'), str(tmp_path / 'label'), str(tmp_path), 'ds', jobs=('rgb',))


def test_merge_writes_reference_layout(tmp_path):
    """merge_color_stats: the merged dicts and the HSV table from per-image pickles, readable by DistTranslation."""
    from ctrlhair_amd import dataset as D
    rng = np.random.default_rng(1)
    rdir = tmp_path / 'hair_info_all_dataset' / 'rgb_stat'
    rdir.mkdir(parents=True)
    ref = {}
    for i in range(5):
        ref[f'ds___{i}'] = R.rgb_stat(_points(rng, i * 3))
        with open(rdir / f'ds___{i}.pkl', 'wb') as f:
            pickle.dump(ref[f'ds___{i}'], f)
    D.merge_color_stats(str(tmp_path), ('rgb',))
    with open(tmp_path / 'rgb_stat_dict.pkl', 'rb') as f:
        merged = pickle.load(f)
    assert sorted(merged) == sorted(ref)
    assert np.array_equal(U.DistTranslation(root=str(tmp_path)).cols_hsv, R.hsv_table(ref))
