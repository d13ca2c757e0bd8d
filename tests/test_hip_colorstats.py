"""Hair colour statistics on the HIP library (ch_resize_linear_u8, ch_hair_erode, ch_hair_color_stats): bit-exact against the
numpy re-statement of the reference scripts (tests/colorstats_ref.py), the dataset jobs end to end, and
HairEditor.get_hair_color against its host composition."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

from ctrlhair_amd import colorstats as CS
from ctrlhair_amd import hostutil as U
from tests import colorstats_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cs(hip_lib):
    from ctrlhair_amd import lib
    return CS.HairColorStats(lib.Handle(0), torch.device('cuda', 0))


def _labels(rng, B, L, kind):
    yy, xx = np.mgrid[:L, :L]
    out = []
    for b in range(B):
        lab = rng.integers(0, 19, (L, L)).astype(np.uint8)
        lab[lab == 13] = 0
        if kind == 'blobs':
            for _ in range(4):
                cy, cx = rng.integers(0, L, 2)
                rr = int(rng.integers(L // 16, L // 3))
                lab[(yy - cy) ** 2 + (xx - cx) ** 2 < rr * rr] = 13
            lab[rng.random((L, L)) < 0.002] = 5                  # isolated holes
        elif kind == 'lines':
            lab[::37, :] = 13
            lab[:, 11::41] = 13
            lab[100:140, 50:300] = 13
            lab[120, 50:300] = 0                                 # a 1-pixel gap inside a band
        elif kind == 'border':
            lab[:L // 5, :] = 13
            lab[:, :L // 6] = 13
            lab[-L // 7:, :] = 13
            lab[:, -L // 4:] = 13
        elif kind == 'all':
            lab[:] = 13
        elif kind == 'none':
            pass
        out.append(lab)
    return np.stack(out)


@pytest.mark.parametrize('kind,B,L,S,ksize', [
    ('blobs', 7, 512, 256, 19), ('blobs', 1, 512, 1024, 19), ('blobs', 3, 512, 384, 19), ('lines', 2, 512, 256, 19),
    ('lines', 1, 512, 1024, 19), ('border', 2, 512, 256, 19), ('border', 1, 512, 384, 19), ('all', 2, 512, 256, 19),
    ('none', 2, 512, 256, 19), ('blobs', 64, 512, 256, 19), ('blobs', 2, 100, 77, 31), ('border', 2, 64, 90, 13),
    ('lines', 2, 512, 256, 5), ('blobs', 2, 300, 256, 1)])
def test_erode_bit_exact(cs, kind, B, L, S, ksize):
    rng = np.random.default_rng(B * 1000 + L + S + ksize)
    lab = _labels(rng, B, L, kind)
    got = cs.erode(lab, S, ksize).cpu().numpy()
    assert got.shape == (B, S, S) and got.dtype == np.uint8
    for b in range(B):
        ref = R.hair_mask(lab[b], S, ksize)
        assert np.array_equal(got[b], ref), (b, int((got[b] != ref).sum()))
    if kind == 'all':
        assert got.all()
    if kind == 'none':
        assert not got.any()


def test_erode_non_square_and_other_label(cs):
    rng = np.random.default_rng(4)
    lab = _labels(rng, 2, 200, 'blobs')[:, :, :150]
    lab[:, 10:60, 20:90] = 7
    got = cs.erode(lab, (333, 250), 13, label=7).cpu().numpy()
    for b in range(2):
        assert np.array_equal(got[b], R.erode(U.resize_nearest(lab[b], (333, 250)) == 7, 13))


def test_erode_rejects_bad_ksize(cs):
    lab = np.zeros((1, 16, 16), np.uint8)
    for k in (0, 4, 33, -1):
        with pytest.raises(RuntimeError, match='ksize'):
            cs.erode(lab, 16, k)


@pytest.mark.parametrize('src,dst', [(256, 1024), (300, 1024), (1024, 1024), (512, 200)])
def test_resize_bit_exact(cs, src, dst):
    rng = np.random.default_rng(src + dst)
    imgs = rng.integers(0, 256, (2, src, src, 3), dtype=np.uint8)
    imgs[1, : src // 2] = 255
    imgs[1, src // 2:, : src // 3] = 0
    got = cs.resize(imgs, (dst, dst)).cpu().numpy()
    for b in range(2):
        assert np.array_equal(got[b], U.resize_bilinear(imgs[b], (dst, dst)))
    rect = rng.integers(0, 256, (40, 70, 3), dtype=np.uint8)
    assert np.array_equal(cs.resize(rect, (33, 91)).cpu().numpy()[0], U.resize_bilinear(rect, (33, 91)))


def test_sums_exact_and_batch_invariant(cs):
    rng = np.random.default_rng(7)
    B, S = 7, 256
    imgs = rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8)
    lab = _labels(rng, B, 512, 'blobs')
    lab[2] = 0                                                   # no hair
    lab[3] = 13                                                  # all hair
    got = cs.sums(imgs, lab)
    assert got.shape == (B, CS.NSTAT) and got.dtype == np.int64
    for b in range(B):
        assert np.array_equal(got[b], R.sums(imgs[b], R.hair_mask(lab[b], S))), b
        assert np.array_equal(cs.sums(imgs[b:b + 1], lab[b:b + 1])[0], got[b])
    assert got[2, 0] == 0 and got[3, 0] == S * S
    assert np.array_equal(cs.sums(imgs, lab), got)               # run-to-run deterministic


def test_sums_int64_bound_1024_all_hair(cs):
    img = np.full((1, 1024, 1024, 3), 255, np.uint8)
    img[0, :, :100] = (254, 3, 250)
    s = cs.sums(img, np.full((1, 512, 512), 13, np.uint8))[0]
    assert np.array_equal(s, R.sums(img[0], np.ones((1024, 1024), np.uint8)))
    assert s[10] == 255 ** 4 * (1024 * 1024 - 1024 * 100) + 254 ** 4 * 1024 * 100


def _write_tree(root, ds, n=20):
    from ctrlhair_amd import dataset as D
    from PIL import Image
    img_dir, lab_dir = os.path.join(root, ds, 'images_256'), os.path.join(root, ds, 'label')
    os.makedirs(img_dir)
    os.makedirs(lab_dir)
    rng = np.random.default_rng(2024)
    kinds = ['blob'] * 12 + ['none'] * 3 + ['few'] * 4 + ['all']
    for i in range(n):
        img, lab = R.synth_image_and_labels(rng, 256, 512, kinds[i % len(kinds)])
        Image.fromarray(img).save(os.path.join(img_dir, f'{i:03d}.png'))
        D.write_label_png(os.path.join(lab_dir, f'{i:03d}.png'), lab)


def _reference_tree(root, ds):
    from ctrlhair_amd import dataset as D
    img_dir, lab_dir = os.path.join(root, ds, 'images_256'), os.path.join(root, ds, 'label')
    rgb, var = {}, {}
    for n in D.list_images(img_dir):
        img = D.read_rgb(os.path.join(img_dir, n))
        lab = D.read_gray(os.path.join(lab_dir, n[:-4] + '.png'))
        pts = img[R.hair_mask(lab, img.shape[0]).astype(bool)]
        rgb[D.code_key(ds, n)] = R.rgb_stat(pts)
        v = R.color_var(pts)
        if v is not None:
            var[D.code_key(ds, n)] = v
    return rgb, var


def test_dataset_jobs_end_to_end(tmp_path):
    root, ds = str(tmp_path), 'synth'
    _write_tree(root, ds)
    env = dict(os.environ, PYTHONPATH=ROOT)
    for job in ('rgb', 'colorvar'):
        r = subprocess.run([sys.executable, '-m', 'ctrlhair_amd.dataset', job, root, ds, '--batch', '8'], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:]
    rgb_ref, var_ref = _reference_tree(root, ds)
    with open(os.path.join(root, 'rgb_stat_dict.pkl'), 'rb') as f:
        rgb = pickle.load(f)
    with open(os.path.join(root, 'color_var_stat_dict.pkl'), 'rb') as f:
        var = pickle.load(f)
    assert sorted(rgb) == sorted(rgb_ref) and len(rgb) == 20
    assert sorted(var) == sorted(var_ref) and 0 < len(var) < len(rgb)          # no-hair and <= 5 pixel images are skipped
    assert sorted(os.listdir(os.path.join(root, 'hair_info_all_dataset', 'color_var_stat'))) == [k + '.pkl' for k in sorted(var_ref)]
    assert sum(np.isnan(v[0]).all() for v in rgb.values()) >= 3
    for k in rgb_ref:
        assert isinstance(rgb[k], list) and len(rgb[k]) == 4
        R.assert_moments_close(rgb[k], rgb_ref[k])
    for k in var_ref:
        g, r = var[k], var_ref[k]
        assert sorted(g) == ['var_hsv', 'var_pca', 'var_pca_comp', 'var_pca_mean', 'var_rgb']
        np.testing.assert_allclose(g['var_rgb'], r['var_rgb'], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(g['var_hsv'], r['var_hsv'], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(g['var_pca'], r['var_pca'], rtol=1e-10)
        assert np.array_equal(g['var_pca_mean'], r['var_pca_mean'])
        ev = r['eigvals']
        if ev[0] - ev[1] > 1e-6 * ev[0] and ev[1] - ev[2] > 1e-6 * ev[0]:
            np.testing.assert_allclose(g['var_pca_comp'], r['var_pca_comp'], atol=1e-8)
    with open(os.path.join(root, 'hsv_stat_dict_ordered.pkl'), 'rb') as f:
        table = pickle.load(f)
    assert np.array_equal(table, R.hsv_table(rgb_ref))
    assert np.array_equal(U.DistTranslation(root=root).cols_hsv, table)


def test_get_hair_color_device_equals_host_composition(hip_lib):
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.hair_editor import HairEditor, procedural_weights
    w = procedural_weights(0, 64)
    w['sean'] = P.sean_state_dict(0, 16)
    he = HairEditor(True, True, weights=w, device=0)
    assert he.models.color_stats is not None
    rng = np.random.default_rng(0)
    for seed in (3, 4):
        img = ((P.synthetic_images(1, 256, seed=seed)[0].transpose(1, 2, 0) * 0.5 + 0.5) * 255).astype(np.uint8)
        got = he.get_hair_color(img)
        parsing = he.get_mask_fullres(img, 1024)
        mask = R.erode(parsing == 13, 19).astype(bool)
        ref = U.resize_bilinear(img, (1024, 1024))[mask].mean(axis=0) if mask.any() else np.full(3, np.nan)
        assert got.dtype == np.float64 and got.shape == (3,)
        assert np.array_equal(got, ref, equal_nan=True), (seed, got, ref, int(mask.sum()))
    # a parse with hair guaranteed: the same device pipeline on an injected label map
    img = rng.integers(0, 256, (300, 300, 3), dtype=np.uint8)
    lab = _labels(rng, 1, 512, 'blobs')
    cs = he.models.color_stats
    s = U.to_host(cs.mask_sums(cs.resize(img, 1024), cs.erode(lab, 1024)))[0]
    mask = R.hair_mask(lab[0], 1024).astype(bool)
    assert mask.any()
    assert np.array_equal(CS.mean_from_sums(s), U.resize_bilinear(img, (1024, 1024))[mask].mean(axis=0))
