"""A plain numpy restatement of PNG unfiltering (RFC 2083 section 6; test code only): the filtered bytes of an 8-bit, non-interlaced image
-- per row the filter type byte and W * C bytes -- back to pixels.  None, Sub and Up rows are whole-row array arithmetic; Average and Paeth
depend on the pixel to the left and run pixel by pixel."""
import numpy as np


class BadFilter(ValueError):
    pass


def _paeth(a: int, b: int, c: int) -> int:
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def unfilter(filtered: bytes, H: int, W: int, C: int) -> np.ndarray:
    """H * (1 + W * C) filtered bytes -> uint8 [H,W,C].  Arithmetic modulo 256; the row above row 0 and the pixel left of column 0 are zero."""
    s = np.frombuffer(bytes(filtered), np.uint8)
    if s.size != H * (1 + W * C):
        raise ValueError(f'{s.size} bytes for {H} rows of 1 + {W * C}')
    s = s.reshape(H, 1 + W * C)
    out = np.zeros((H, W, C), np.uint8)
    up = np.zeros((W, C), np.int64)
    for y in range(H):
        t = int(s[y, 0])
        raw = s[y, 1:].reshape(W, C).astype(np.int64)
        if t == 0:
            row = raw
        elif t == 1:
            row = np.cumsum(raw, axis=0) & 255                                             # x[i] = raw[i] + x[i - 1]
        elif t == 2:
            row = (raw + up) & 255
        elif t in (3, 4):
            row = np.zeros((W, C), np.int64)
            r, u = raw.tolist(), up.tolist()
            for c in range(C):
                a = cc = 0
                for x in range(W):
                    b = u[x][c]
                    pred = (a + b) >> 1 if t == 3 else _paeth(a, b, cc)
                    a = (r[x][c] + pred) & 255
                    cc = b
                    row[x, c] = a
        else:
            raise BadFilter(f'row {y}: filter type {t}')
        out[y] = row
        up = row
    return out
