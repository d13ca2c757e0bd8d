"""numpy oracles of the image ingest (ctrlhair_amd/ingest.py, csrc/ingest.hip) and the shape lists its tests share.

pil_resize_bilinear applies ingest.pil_bilinear_coeffs exactly as the kernels do: horizontal pass into uint8, then the vertical pass,
each clip8(((1 << 21) + sum k p) >> 22) in integers, a pass whose size does not change skipped.  cv2_resize_linear and nearest restate
hostutil's two resizes with their own index arithmetic (not by calling them), so that test_ingest.py can compare the two."""
import numpy as np

from ctrlhair_amd import ingest as G

# (H, W) sources of the issue's list, then the three that run one pass only or none at 512
SHAPES = [(1, 1), (2, 3), (7, 5), (64, 48), (100, 131), (512, 512), (513, 511), (1024, 768), (40, 1300)]
SIZES = [16, 32, 64, 512]
ONE_PASS = [((512, 37), 512), ((37, 512), 512), ((512, 512), 512)]
# the ragged call of the GPU tests, N = 19: every shape with random and with ramp content, and one constant-255 image
BATCH19 = [('random', s) for s in SHAPES] + [('ramp', s) for s in SHAPES] + [('white', (513, 511))]


def content(kind: str, H: int, W: int, seed: int = 0) -> np.ndarray:
    """uint8 [H,W,3]: 'random', 'ramp' (a diagonal ramp, different per channel) or 'white' (constant 255: the clip8 edge)."""
    if kind == 'random':
        return np.random.default_rng(seed + 7919 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == 'ramp':
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(3 * x + y) % 256, (x + 5 * y) % 256, 255 - (x + y) % 256], -1).astype(np.uint8)
    if kind == 'white':
        return np.full((H, W, 3), 255, np.uint8)
    raise ValueError(kind)


def _pass(a: np.ndarray, n_out: int) -> np.ndarray:
    """One resample pass along axis 0 of uint8 [n_in, ...]."""
    n_in = a.shape[0]
    xmin, count, kk = G.pil_bilinear_coeffs(n_in, n_out)
    acc = np.full((n_out,) + a.shape[1:], 1 << (G.PRECISION_BITS - 1), np.int64)
    src = a.astype(np.int64)
    tail = (1,) * (a.ndim - 1)
    for j in range(kk.shape[1]):
        acc += kk[:, j].astype(np.int64).reshape((-1,) + tail) * src[np.minimum(xmin + j, n_in - 1)]    # kk is zero past count
    assert int(np.abs(acc).max()) < 2 ** 31                    # the kernels accumulate in int32
    return np.clip(acc >> G.PRECISION_BITS, 0, 255).astype(np.uint8)


def pil_resize_bilinear(img: np.ndarray, size: int) -> np.ndarray:
    """Image.fromarray(img).resize((size, size), Image.BILINEAR) for uint8 [H,W,3]."""
    a = np.asarray(img, np.uint8)
    if a.shape[1] != size:
        a = _pass(a.transpose(1, 0, 2), size).transpose(1, 0, 2)
    if a.shape[0] != size:
        a = _pass(a, size)
    return a


def _taps(n_out: int, n_in: int):
    f = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
    i0 = np.floor(f)
    fr = (f - i0).astype(np.float32)
    i0 = i0.astype(np.int64)
    fr[(i0 < 0) | (i0 >= n_in - 1)] = 0
    i0 = np.clip(i0, 0, n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), np.rint((np.float32(1) - fr) * np.float32(2048)).astype(np.int64), np.rint(fr * np.float32(2048)).astype(np.int64)


def cv2_resize_linear(img: np.ndarray, size: int) -> np.ndarray:
    """cv2.resize(img, (size, size)) (INTER_LINEAR) for uint8 [H,W,3]: the kernel's arithmetic, every axis filtered even at equal size."""
    a = np.asarray(img, np.uint8).astype(np.int64)
    x0, x1, a0, a1 = _taps(size, a.shape[1])
    y0, y1, b0, b1 = _taps(size, a.shape[0])
    rows = a[:, x0] * a0[None, :, None] + a[:, x1] * a1[None, :, None]
    top, bot = rows[y0] >> 4, rows[y1] >> 4
    out = (((b0[:, None, None] * top) >> 16) + ((b1[:, None, None] * bot) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def nearest(lab: np.ndarray, size: int) -> np.ndarray:
    """uint8 [h,w] -> [size,size]: src = min(int(dst * (in / out)), in - 1), the quotient in double."""
    h, w = lab.shape
    ys = np.array([min(int(y * (h / size)), h - 1) for y in range(size)])
    xs = np.array([min(int(x * (w / size)), w - 1) for x in range(size)])
    return lab[ys][:, xs]
