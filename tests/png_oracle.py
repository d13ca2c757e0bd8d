"""numpy oracles of the PNG encoder (test code only): the filtered byte stream ch_png_encode deflates (include/ctrlhair_hip.h; RFC 2083
section 6 and libpng's minimum-sum heuristic, restated with plain array arithmetic), and the "chunked RLE yardstick" the device
stream's size is compared with: zlib's own run-length strategy over the same chunks."""
import zlib

import numpy as np


def _neighbours(img: np.ndarray):
    """img uint8 [H,W,C] -> int32 [H, W*C] arrays x, a (one pixel left), b (above), c (above left); outside the image: 0."""
    H, W, C = img.shape
    x = img.reshape(H, W * C).astype(np.int32)
    a = np.zeros_like(x)
    a[:, C:] = x[:, :-C]
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    c = np.zeros_like(x)
    c[1:, C:] = x[:-1, :-C]
    return x, a, b, c


def filter_rows(img: np.ndarray):
    """The five filtered versions of every row: uint8 [5, H, W*C]."""
    x, a, b, c = _neighbours(img)
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - paeth]).astype(np.uint8)     # (the cast wraps modulo 256)


def filtered_stream(img: np.ndarray, filter: int = -1):
    """img uint8 [H,W] or [H,W,C] -> (the H * (1 + W*C) bytes a PNG's zlib stream holds, the filter type of every row).
    filter -1: per row the type with the smallest sum of |int8(byte)|, the lowest type on a tie; 0..4: that type."""
    img = np.asarray(img, dtype=np.uint8)
    if img.ndim == 2:
        img = img[:, :, None]
    H, W, C = img.shape
    rows = filter_rows(img)
    if filter < 0:
        cost = np.abs(rows.view(np.int8).astype(np.int64)).sum(axis=2)                     # [5,H]
        types = np.argmin(cost, axis=0)                                                     # first minimum = lowest type
    else:
        types = np.full(H, filter, dtype=np.int64)
    out = np.empty((H, 1 + W * C), np.uint8)
    out[:, 0] = types
    out[:, 1:] = rows[types, np.arange(H)]
    return out.tobytes(), types


def unfilter(stream: bytes, H: int, W: int, C: int) -> np.ndarray:
    """The inverse (a slow per-byte decoder, for the tests of this file's own functions)."""
    rb = W * C
    s = np.frombuffer(stream, np.uint8).reshape(H, 1 + rb)
    out = np.zeros((H, rb), np.int32)
    for y in range(H):
        t = int(s[y, 0])
        for j in range(rb):
            a = out[y, j - C] if j >= C else 0
            b = out[y - 1, j] if y else 0
            c = out[y - 1, j - C] if y and j >= C else 0
            if t == 4:
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
            else:
                pred = (0, a, b, (a + b) >> 1)[t]
            out[y, j] = (int(s[y, 1 + j]) + pred) & 255
    return out.astype(np.uint8).reshape(H, W, C)


def rle_yardstick(stream: bytes, chunk: int) -> int:
    """Bytes of the chunked RLE yardstick: per `chunk` bytes a raw deflate at level 1 with zlib's Z_RLE strategy (distance-1 matches and
    Huffman codes only) ended by a sync flush, or the stored form 5 + len if that is smaller; plus 8 bytes of framing (zlib header,
    final empty block, Adler-32)."""
    total = 8
    for a in range(0, len(stream), chunk):
        part = stream[a:a + chunk]
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        n = len(co.compress(part)) + len(co.flush(zlib.Z_SYNC_FLUSH))
        total += min(n, 5 + len(part))
    return total


def huffman_only(stream: bytes) -> int:
    """Bytes of the whole stream under zlib's Z_HUFFMAN_ONLY strategy (no matches at all)."""
    co = zlib.compressobj(6, zlib.DEFLATED, 15, 9, zlib.Z_HUFFMAN_ONLY)
    return len(co.compress(stream)) + len(co.flush())


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------------
def label_map(size: int = 256, discs: int = 18, seed: int = 0) -> np.ndarray:
    """uint8 [size,size]: random discs of labels 1..18 on 0."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:size, :size]
    lab = np.zeros((size, size), np.uint8)
    for k in range(discs):
        cy, cx, r = rng.integers(0, size), rng.integers(0, size), rng.integers(size // 16, size // 4)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = 1 + k % 18
    return lab


def smooth_cells(rows: int, cols: int, cell: int, seed: int = 0) -> np.ndarray:
    """uint8 [rows*cols, cell, cell, 3]: smooth colour gradients with a little noise, what renders look like to a compressor."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:cell, :cell] / float(cell)
    out = np.empty((rows * cols, cell, cell, 3), np.uint8)
    for k in range(rows * cols):
        f = rng.uniform(0.5, 3.0, (3, 2))
        ph = rng.uniform(0, 6.28, 3)
        base = np.stack([np.sin(f[c, 0] * 3 * yy + f[c, 1] * 3 * xx + ph[c]) for c in range(3)], axis=2) * 100 + 128
        out[k] = np.clip(base + rng.normal(0, 3, base.shape), 0, 255).astype(np.uint8)
    return out


def ramp(H: int, W: int, C: int) -> np.ndarray:
    """uint8 [H,W,C]: a horizontal ramp, the same in every row and channel."""
    return np.broadcast_to((np.arange(W) % 256).astype(np.uint8)[None, :, None], (H, W, C)).copy()
