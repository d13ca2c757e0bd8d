"""Numpy re-statement of the reference's hair colour arithmetic (dataset_scripts/script_get_rgb_hsv_label.py:49-90,
script_get_color_var_label.py:48-90, hair_editor.py:233-243), one image at a time, for the colour-statistics tests.
cv2's calls are replaced by their hostutil pins (resize_nearest, resize_bilinear, rgb_to_hsv_u8) and by an erosion written
from its definition; sklearn's PCA by np.linalg.eigh of the population covariance."""
import numpy as np

from ctrlhair_amd import hostutil as U
from ctrlhair_amd.colorstats import NSTAT, ellipse_half_widths

HAIR_IDX = 13


def ellipse_element(ksize):
    """cv2.getStructuringElement(MORPH_ELLIPSE, (ksize, ksize)) as a bool [ksize, ksize] array."""
    r = ksize // 2
    el = np.zeros((ksize, ksize), bool)
    for i, hw in enumerate(ellipse_half_widths(ksize)):
        el[i, r - hw:r + hw + 1] = True
    return el


def erode(mask, ksize):
    """cv2.erode(mask, ellipse, iterations=1), default border (outside = set): AND of the shifted mask over the element."""
    m = np.asarray(mask).astype(bool)
    r = ksize // 2
    H, W = m.shape
    pad = np.ones((H + 2 * r, W + 2 * r), bool)
    pad[r:r + H, r:r + W] = m
    out = np.ones_like(m)
    el = ellipse_element(ksize)
    for dy in range(ksize):
        for dx in range(ksize):
            if el[dy, dx]:
                out &= pad[dy:dy + H, dx:dx + W]
    return out.astype(np.uint8)


def erode_brute(mask, ksize):
    """Per-pixel definition, for small maps: pixel kept iff every element position inside the image is set."""
    m = np.asarray(mask).astype(bool)
    r = ksize // 2
    el = ellipse_element(ksize)
    H, W = m.shape
    out = np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            ok = True
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yy, xx = y + dy, x + dx
                    if el[dy + r, dx + r] and 0 <= yy < H and 0 <= xx < W and not m[yy, xx]:
                        ok = False
            out[y, x] = ok
    return out


def hair_mask(labels, size, ksize=19, label=HAIR_IDX):
    """script_get_rgb_hsv_label.py:52-56 for a square image of side `size` (or (w, h))."""
    size = (size, size) if np.isscalar(size) else tuple(size)
    return erode(U.resize_nearest(np.asarray(labels).astype(np.uint8), size) == label, ksize)


def sums(img, mask):
    """The CH_COLOR_STATS layout, by numpy int64 sums."""
    p = np.asarray(img).reshape(-1, 3)[np.asarray(mask).reshape(-1).astype(bool)].astype(np.int64)
    hsv = U.rgb_to_hsv_u8(p[None].astype(np.uint8))[0].astype(np.int64)
    out = [len(p)]
    for k in (1, 2, 3, 4):
        out += list((p ** k).sum(0))
    out += [(p[:, 0] * p[:, 1]).sum(), (p[:, 0] * p[:, 2]).sum(), (p[:, 1] * p[:, 2]).sum()]
    for j in range(3):
        out += [hsv[:, j].sum(), (hsv[:, j] ** 2).sum()]
    assert len(out) == NSTAT
    return np.array(out, np.int64)


def rgb_stat(points):
    """script_get_rgb_hsv_label.py:60-63 (NaN, with numpy's warnings silenced, for no points)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            moment1 = points.mean(axis=0)
            moment2 = ((points - moment1) ** 2).mean(axis=0)
            moment3 = ((points - moment1) ** 3).mean(axis=0)
            moment4 = ((points - moment1) ** 4).mean(axis=0)
    return [moment1, moment2, moment3, moment4]


def color_var(points):
    """script_get_color_var_label.py:58-86 without var_hls / var_yuv; None for <= 5 points."""
    if len(points) <= 5:
        return None
    var_rgb = (points / 255).var(axis=0)
    hsv = U.rgb_to_hsv_u8(points[None, ...].astype(np.uint8)) / np.array([180, 255, 255])
    var_hsv = hsv.var(axis=(0, 1))
    x = points.astype(np.float64)
    mean = x.mean(0)
    cov = (x - mean).T @ (x - mean) / len(x)
    w, v = np.linalg.eigh(cov)
    comp = v[:, ::-1][:, :2].T.copy()
    comp *= np.sign(comp[np.arange(2), np.argmax(np.abs(comp), axis=1)])[:, None]
    proj = (x - mean) @ comp[0]
    return {'var_rgb': var_rgb, 'var_hsv': var_hsv, 'var_pca': proj.std(), 'var_pca_mean': mean, 'var_pca_comp': comp,
            'eigvals': w[::-1]}


def hsv_table(rgb_stat_dict):
    """script_get_rgb_hsv_label.py:80-90."""
    cols = np.array([rgb_stat_dict[f][0] for f in list(rgb_stat_dict)])
    with np.errstate(invalid='ignore'):
        cols_hsv = U.rgb_to_hsv_u8(cols[None, ...].astype('uint8'))[0]
    for dim in range(3):
        cols_hsv[:, dim].sort()
    return cols_hsv


def assert_moments_close(got, ref, tol=1e-12):
    """Moments to rtol tol with atol tol * sigma^k; NaN exactly where the reference has NaN."""
    sigma = np.sqrt(np.nan_to_num(ref[1])) + 1.0
    for k, (g, r) in enumerate(zip(got, ref)):
        g, r = np.asarray(g, np.float64), np.asarray(r, np.float64)
        assert g.shape == r.shape == (3,)
        assert np.array_equal(np.isnan(g), np.isnan(r))
        ok = np.isnan(r) | (np.abs(g - r) <= tol * np.abs(r) + tol * sigma ** (k + 1))
        assert ok.all(), (k + 1, g, r)


def synth_image_and_labels(rng, size, lsize, kind):
    """A seeded (RGB uint8 [size,size,3], labels uint8 [lsize,lsize]) pair: kind 'blob' (hair blobs on random labels), 'none'
    (no hair), 'few' (a hair patch that erodes to a handful of pixels), 'all' (all hair)."""
    img = rng.integers(0, 256, (size, size, 3), dtype=np.uint8)
    img[..., 0] = (img[..., 0] // 3 + 80).astype(np.uint8)                   # some colour correlation for the PCA
    lab = rng.integers(0, 19, (lsize, lsize)).astype(np.uint8)
    lab[lab == HAIR_IDX] = 0
    yy, xx = np.mgrid[:lsize, :lsize]
    if kind == 'blob':
        for _ in range(3):
            cy, cx, rr = rng.integers(0, lsize, 2).tolist() + [int(rng.integers(lsize // 8, lsize // 3))]
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 < rr * rr] = HAIR_IDX
    elif kind == 'few':
        # a disc just larger than the element at image scale: erodes to a few pixels (possibly <= 5)
        s = lsize / size
        c, rr = lsize // 2, (9 + float(rng.integers(0, 3)) * 0.5) * s
        lab[(yy - c) ** 2 + (xx - c) ** 2 <= rr * rr] = HAIR_IDX
    elif kind == 'all':
        lab[:] = HAIR_IDX
    return img, lab
