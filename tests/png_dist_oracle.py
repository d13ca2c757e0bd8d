"""numpy / plain-Python oracle of the PNG encoder's parse with caller-given match distances (test code only): the rule of
ch_png_encode_dist (include/ctrlhair_hip.h) restated position by position, the replay of a token list, the size
yardstick (zlib's default strategy over the same chunks) and the synthetic contact sheets the tests share."""
import zlib

import numpy as np

from tests import png_oracle as PO


def interval_lengths(x: np.ndarray, d: int) -> np.ndarray:
    """int [n]: for every position the length of the maximal interval of eq_d = (i >= d and x[i] == x[i - d]) that holds it, 0 outside."""
    n = len(x)
    eq = np.zeros(n + 2, np.int8)                                                          # eq[1 + i], a false on either side
    if d < n:
        eq[1 + d:1 + n] = x[d:] == x[:n - d]
    step = np.diff(eq)
    out = np.zeros(n, np.int64)
    for s, e in zip(np.flatnonzero(step == 1), np.flatnonzero(step == -1)):               # [s, e) in positions
        out[s:e] = e - s
    return out


def classes(chunk: bytes, distances) -> np.ndarray:
    """int [n]: the index into (1,) + distances of the distance a position belongs to (the longest interval, the earlier distance on a
    tie), -1 for a literal (no interval of 3 or more)."""
    x = np.frombuffer(bytes(chunk), np.uint8)
    D = (1,) + tuple(int(d) for d in distances)
    lens = np.stack([interval_lengths(x, d) for d in D])
    return np.where(lens.max(axis=0) >= 3, lens.argmax(axis=0), -1)                        # argmax: the first maximum


def parse(chunk: bytes, distances) -> list:
    """The tokens of one chunk: ('L', byte) and ('M', length, distance).  A class run of R positions from p: R // 258 matches of 258,
    then the remainder as one match if it is >= 3, else as literals."""
    x = np.frombuffer(bytes(chunk), np.uint8)
    D = (1,) + tuple(int(d) for d in distances)
    cls = classes(chunk, distances)
    n, i, tokens = len(x), 0, []
    while i < n:
        c = int(cls[i])
        if c < 0:
            tokens.append(('L', int(x[i])))
            i += 1
            continue
        j = i
        while j < n and cls[j] == c:
            j += 1
        p = i
        for _ in range((j - i) // 258):
            tokens.append(('M', 258, D[c]))
            p += 258
        if j - p >= 3:
            tokens.append(('M', j - p, D[c]))
        else:
            tokens += [('L', int(x[q])) for q in range(p, j)]
        i = j
    return tokens


def replay(tokens) -> bytes:
    """The bytes a token list stands for; a match that reaches before the first byte is an error."""
    out = bytearray()
    for t in tokens:
        if t[0] == 'L':
            out.append(t[1])
        else:
            _, length, dist = t
            if dist < 1 or dist > len(out):
                raise ValueError(f'match {t} at position {len(out)} reaches before the start')
            for _ in range(length):
                out.append(out[-dist])
    return bytes(out)


def zlib_chunked(stream: bytes, chunk: int, level: int) -> int:
    """Bytes of the chunked zlib yardstick: per `chunk` bytes a fresh raw deflate at `level` with the default strategy ended by a sync
    flush, or the stored form 5 + len if that is smaller; plus 8 bytes of framing (the shape of png_oracle.rle_yardstick)."""
    total = 8
    for a in range(0, len(stream), chunk):
        part = stream[a:a + chunk]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        n = len(co.compress(part)) + len(co.flush(zlib.Z_SYNC_FLUSH))
        total += min(n, 5 + len(part))
    return total


def sheet(rows: int, variants: int, cell: int, margin: int, seed: int = 0) -> np.ndarray:
    """uint8 [rows * cell, (variants + 1) * cell + variants * margin, 3]: a synthetic contact sheet.  Column 0 of a row is a
    smooth_cells image; columns 1..variants are that image with an elliptical region replaced by another smooth_cells image, one per
    column -- renders that agree outside the hair.  The background (the margins) is white."""
    base = PO.smooth_cells(rows, 1, cell, seed)
    other = PO.smooth_cells(rows, variants, cell, seed + 1000)
    yy, xx = np.mgrid[:cell, :cell] / float(cell)
    inside = ((yy - 0.36) / 0.28) ** 2 + ((xx - 0.5) / 0.24) ** 2 <= 1.0                       # about a fifth of the cell
    cols = variants + 1
    out = np.full((rows * cell, cols * cell + margin * (cols - 1), 3), 255, np.uint8)
    for r in range(rows):
        for c in range(cols):
            img = base[r].copy()
            if c:
                img[inside] = other[r * variants + c - 1][inside]
            x0 = c * (cell + margin)
            out[r * cell:(r + 1) * cell, x0:x0 + cell] = img
    return out


def tile(n: int, period: int = 120, seed: int = 0) -> np.ndarray:
    """uint8 [n]: a random tile of `period` bytes repeated, with a run of 40 equal bytes inside the tile and, in the third repetition, a
    defect of two changed bytes."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 256, period, dtype=np.uint8)
    t[30:70] = 77
    x = np.tile(t, n // period + 1)[:n].copy()
    x[2 * period + 10:2 * period + 12] ^= 0x55
    return x
