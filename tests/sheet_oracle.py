"""numpy oracles of ch_sheet_compose and ch_sweep_stats (include/ctrlhair_hip.h): plain loops over cells and renders, nothing shared
with the kernels but the specification.  No GPU."""
import numpy as np

HAIR = 13
NSTAT = 16


def to_u8(x: np.ndarray) -> np.ndarray:
    """x * 127.5 and + 127.5 each rounded to float32 (numpy never fuses them), clamped to [0,255], truncated; NaN -> 0."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        b = x * np.float32(127.5) + np.float32(127.5)
        b = np.where(np.isnan(b), np.float32(0), np.clip(b, np.float32(0), np.float32(255)))
    return b.astype(np.uint8)


def nearest_index(n_out: int, n_in: int) -> np.ndarray:
    """cv2 INTER_NEAREST as hostutil.resize_nearest: min(int(dst * (in / out)), in - 1)."""
    return np.minimum((np.arange(n_out) * (n_in / n_out)).astype(np.int64), n_in - 1)


def as_rgb(src: np.ndarray, kind: int, lut: np.ndarray = None) -> np.ndarray:
    """One source -> uint8 [Hs,Ws,3].  kind 0: float32 [3,Hs,Ws]; 1: uint8 [Hs,Ws,3]; 2: uint8 labels [Hs,Ws] through lut [256,3]."""
    if kind == 0:
        return to_u8(src).transpose(1, 2, 0)
    if kind == 1:
        return np.asarray(src, dtype=np.uint8)
    return np.asarray(lut, dtype=np.uint8)[np.asarray(src, dtype=np.uint8)]


def compose(canvas: np.ndarray, srcs, kind: int, cells, rows: int, cols: int, H: int, W: int, margin: int, lut=None) -> np.ndarray:
    """util/canvas_grid.py process_draw_image for each source, in place: cell (i, j) starts at y = i H, x = j (W + margin); a source of
    another size is nearest-mapped; a cell outside the grid is skipped."""
    assert canvas.shape == (rows * H, cols * W + margin * (cols - 1), 3)
    for src, (i, j) in zip(srcs, cells):
        if not (0 <= i < rows and 0 <= j < cols):
            continue
        rgb = as_rgb(src, kind, lut)
        rgb = rgb[nearest_index(H, rgb.shape[0])][:, nearest_index(W, rgb.shape[1])]
        canvas[i * H:(i + 1) * H, j * (W + margin):j * (W + margin) + W] = rgb
    return canvas


def sweep_stats(img: np.ndarray, kind: int, labels: np.ndarray, ref) -> np.ndarray:
    """int64 [N,16]: the columns of CH_SWEEP_STATS.  img: float32 [N,3,H,W] (kind 0) or uint8 [N,H,W,3] (kind 1); labels [N,h,w]."""
    N = len(img)
    rgb = np.stack([as_rgb(im, kind) for im in img])
    H, W = rgb.shape[1:3]
    lab = np.asarray(labels)[:, nearest_index(H, labels.shape[1])][:, :, nearest_index(W, labels.shape[2])].astype(np.int64)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((N, NSTAT), np.int64)
    for n in range(N):
        hair = lab[n] == HAIR
        out[n, 0] = hair.sum()
        out[n, 1:5] = [xx[hair].sum(), yy[hair].sum(), (xx[hair] ** 2).sum(), (yy[hair] ** 2).sum()]
        out[n, 5:9] = [yy[hair].min(), yy[hair].max(), xx[hair].min(), xx[hair].max()] if hair.any() else [-1] * 4
        out[n, 9:12] = rgb[n][hair].astype(np.int64).sum(axis=0)
        r = int(ref[n])
        if r >= 0:
            hair_r = lab[r] == HAIR
            either = hair | hair_r
            out[n, 12] = (lab[n] != lab[r]).sum()
            out[n, 13] = (hair & hair_r).sum()
            out[n, 14] = np.abs(rgb[n][either].astype(np.int64) - rgb[r][either].astype(np.int64)).sum()
            out[n, 15] = either.sum()
    return out
