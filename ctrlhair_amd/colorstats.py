"""Hair colour statistics on the HIP library: the colour labels of the dataset scripts and the HSV table of the colour sliders.

The reference computes them one image at a time with cv2, numpy and sklearn (dataset_scripts/script_get_rgb_hsv_label.py:49-90,
dataset_scripts/script_get_color_var_label.py:48-90, hair_editor.py:233-243):
  hair pixels = label 13 of the nearest-resized label map, eroded with the 19x19 MORPH_ELLIPSE element;
  rgb_stat    = [mean, central moments 2, 3, 4] of their RGB values (float64 [3] each, NaN when no pixel is left);
  color_var   = variances of RGB / 255 and HSV / [180, 255, 255], and a two-component PCA of the RGB points (only for > 5 pixels);
  hsv table   = the mean colours as uint8, converted to HSV, each column sorted (util/color_from_hsv_to_gaussian.py reads it).

Here the device computes the eroded mask and exact int64 sums of the masked pixels (`ch_hair_erode`, `ch_hair_color_stats`,
include/ctrlhair_hip.h), and the functions below finish the float64 statistics from those sums on the host: the moments and
variances exactly with Python integers, rounded once; the PCA from the exact covariance.  The host part needs no GPU.

Not computed: the `var_hls` and `var_yuv` entries of color_var_stat (script_get_color_var_label.py:66-80).  No reference program
reads them, and their 8-bit cv2 conversions cannot be pinned without cv2.  (`var_lab` is computed there but never stored.)
"""
from fractions import Fraction
from typing import Optional

import numpy as np
import torch

from . import hostutil as U
from .devop import DeviceOp
from .hostutil import HAIR_IDX

NSTAT = 22                # CH_COLOR_STATS: [n, sum c (3), c^2 (3), c^3 (3), c^4 (3), c0c1, c0c2, c1c2, H, H^2, S, S^2, V, V^2]
ERODE_KSIZE = 19          # script_get_rgb_hsv_label.py:55 / script_get_color_var_label.py:55 / hair_editor.py:240
MIN_VAR_POINTS = 5        # script_get_color_var_label.py:63: color_var_stat only for len(points) > 5


def ellipse_half_widths(ksize: int) -> np.ndarray:
    """Row half-widths of cv2.getStructuringElement(MORPH_ELLIPSE, (ksize, ksize)), dy = -r..r:
    dx = cvRound(c * sqrt((r^2 - dy^2) / r^2)), c = r = ksize // 2."""
    if ksize < 1 or ksize % 2 == 0:
        raise ValueError(f'ksize must be odd and positive, got {ksize}')
    r = ksize // 2
    inv_r2 = 1.0 / (r * r) if r else 0.0
    return np.array([int(np.rint(r * np.sqrt((r * r - dy * dy) * inv_r2))) for dy in range(-r, r + 1)], np.int64)


def _size(size):
    """int or cv2-order (w, h) -> (h, w)."""
    if isinstance(size, (int, np.integer)):
        return int(size), int(size)
    w, h = size
    return int(h), int(w)


class HairColorStats(DeviceOp):
    """Device side: resize, eroded hair mask and masked sums on one ch_handle.  Inputs are numpy arrays or torch tensors
    (uint8 or convertible); outputs are device tensors, except `sums` (numpy int64 [B, NSTAT])."""

    def _u8(self, a) -> torch.Tensor:
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        return t.to(self.device).to(torch.uint8).contiguous()

    def resize(self, img, size) -> torch.Tensor:
        """cv2.resize(img, size) (INTER_LINEAR, size = (w, h) or an int) of uint8 [H,W,C] / [B,H,W,C] -> uint8 [B,h,w,C]."""
        t = self._u8(img)
        if t.dim() == 3:
            t = t[None]
        B, Hs, Ws, C = t.shape
        h, w = _size(size)
        out = torch.empty(B, h, w, C, dtype=torch.uint8, device=self.device)
        self.handle.call('ch_resize_linear_u8', t.data_ptr(), out.data_ptr(), B, Hs, Ws, C, h, w, self._stream())
        return out

    def erode(self, labels, size, ksize: int = ERODE_KSIZE, label: int = HAIR_IDX) -> torch.Tensor:
        """Label maps uint8 [Hl,Wl] / [B,Hl,Wl] -> eroded hair mask uint8 0/1 [B,h,w]: nearest resize to size = (w, h) (or an
        int), label == `label`, cv2.erode with the ksize x ksize MORPH_ELLIPSE element."""
        t = self._u8(labels)
        if t.dim() == 2:
            t = t[None]
        B, Hl, Wl = t.shape
        h, w = _size(size)
        out = torch.empty(B, h, w, dtype=torch.uint8, device=self.device)
        self.handle.call('ch_hair_erode', t.data_ptr(), B, Hl, Wl, int(label), int(ksize), out.data_ptr(), h, w, self._stream())
        return out

    def mask_sums(self, imgs, mask) -> torch.Tensor:
        """RGB uint8 [B,H,W,3] and mask [B,H,W] (non-zero = counted) -> int64 [B, NSTAT] device tensor of exact sums."""
        x, m = self._u8(imgs), self._u8(mask)
        if x.dim() == 3:
            x = x[None]
        B, H, W, C = x.shape
        if C != 3 or tuple(m.shape[-2:]) != (H, W) or m.numel() != B * H * W:
            raise ValueError(f'mask_sums: images {tuple(x.shape)} and mask {tuple(m.shape)} do not match')
        out = torch.empty(B, NSTAT, dtype=torch.int64, device=self.device)
        self.handle.call('ch_hair_color_stats', x.data_ptr(), m.data_ptr(), B, H, W, out.data_ptr(), self._stream())
        return out

    def sums(self, imgs, labels, ksize: int = ERODE_KSIZE) -> np.ndarray:
        """The dataset scripts' per-image pipeline for a batch: RGB uint8 [B,H,W,3], label maps [B,Hl,Wl] -> int64 [B, NSTAT]."""
        x = self._u8(imgs)
        if x.dim() == 3:
            x = x[None]
        H, W = int(x.shape[1]), int(x.shape[2])
        return U.to_host(self.mask_sums(x, self.erode(labels, (W, H), ksize)))


# ---- host finishing (exact from the integer sums) --------------------------------------------------------------------------
def _ints(s):
    s = [int(v) for v in np.asarray(s).reshape(-1)]
    if len(s) != NSTAT:
        raise ValueError(f'expected {NSTAT} sums, got {len(s)}')
    return s


def _central(n, s1, s2, s3, s4):
    """Exact central moments 2-4 (population) from power sums, as Fractions."""
    m = Fraction(s1, n)
    return (Fraction(s2, n) - m * m,
            Fraction(s3, n) - 3 * m * Fraction(s2, n) + 2 * m ** 3,
            Fraction(s4, n) - 4 * m * Fraction(s3, n) + 6 * m * m * Fraction(s2, n) - 3 * m ** 4)


def mean_from_sums(s) -> np.ndarray:
    """img[mask].mean(axis=0): float64 [3] (NaN without hair pixels)."""
    s = _ints(s)
    if s[0] == 0:
        return np.full(3, np.nan)
    return np.array([float(Fraction(s[1 + j], s[0])) for j in range(3)])


def rgb_stat_from_sums(s):
    """[moment1, moment2, moment3, moment4] of script_get_rgb_hsv_label.py:60-63, each float64 [3]; all NaN when the eroded
    mask is empty (np.mean of an empty selection; color_texture_branch/dataset.py:24 uses it to detect 'no hair')."""
    s = _ints(s)
    n = s[0]
    if n == 0:
        return [np.full(3, np.nan) for _ in range(4)]
    cen = [_central(n, s[1 + j], s[4 + j], s[7 + j], s[10 + j]) for j in range(3)]
    return [mean_from_sums(s)] + [np.array([float(cen[j][k]) for j in range(3)]) for k in range(3)]


def color_var_from_sums(s) -> Optional[dict]:
    """color_var_stat of script_get_color_var_label.py:58-86 (without var_hls / var_yuv), or None for <= 5 pixels:
    var_rgb   population variance of points / 255
    var_hsv   population variance of hsv / [180, 255, 255]
    var_pca   std of the first principal projection = sqrt(largest eigenvalue of the population covariance)
    var_pca_mean, var_pca_comp   sklearn PCA(n_components=2).mean_ / .components_ (sign: each row's largest |entry| > 0)."""
    s = _ints(s)
    n = s[0]
    if n <= MIN_VAR_POINTS:
        return None

    def var(s1, s2, scale):
        return float(Fraction(n * s2 - s1 * s1, n * n * scale * scale))

    var_rgb = np.array([var(s[1 + j], s[4 + j], 255) for j in range(3)])
    var_hsv = np.array([var(s[16 + 2 * j], s[17 + 2 * j], d) for j, d in enumerate((180, 255, 255))])
    sq = [[s[4], s[13], s[14]], [s[13], s[5], s[15]], [s[14], s[15], s[6]]]
    cov = np.array([[float(Fraction(n * sq[i][j] - s[1 + i] * s[1 + j], n * n)) for j in range(3)] for i in range(3)])
    w, v = np.linalg.eigh(cov)                     # ascending eigenvalues
    comp = v[:, ::-1][:, :2].T.copy()              # [2,3]: principal axes, largest variance first
    idx = np.argmax(np.abs(comp), axis=1)
    comp *= np.sign(comp[np.arange(2), idx])[:, None]
    return {'var_rgb': var_rgb, 'var_hsv': var_hsv, 'var_pca': np.float64(np.sqrt(max(w[-1], 0.0))),
            'var_pca_mean': mean_from_sums(s), 'var_pca_comp': comp}


def hsv_table(rgb_stat_dict) -> np.ndarray:
    """hsv_stat_dict_ordered.pkl from rgb_stat_dict (script_get_rgb_hsv_label.py:76-90): the mean colours cast with
    .astype('uint8') (numpy's cast, NaN entries included), cv2's RGB2HSV, each column sorted.  uint8 [N,3]."""
    cols = np.array([rgb_stat_dict[f][0] for f in list(rgb_stat_dict)], dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid='ignore'):
        cols_u8 = cols[None, ...].astype('uint8')
    cols_hsv = U.rgb_to_hsv_u8(cols_u8)[0]
    for dim in range(3):
        cols_hsv[:, dim].sort()
    return cols_hsv
