"""The corpus of the PNG decoder's tests, built from seeds at test time (no binary fixtures): pixels -> filtered bytes
(png_oracle.filtered_stream) -> a zlib stream made with chosen zlib parameters -> a PNG file (pngenc.wrap_png); two long streams whose
FILTERED bytes are given and whose pixels follow from them; files written by Pillow at its defaults.  And the malformed set: zlib streams
of a 17 x 31 x 3 image broken by byte surgery, or written bit by bit, each with the status class the decoder must give it.

check_conditions() asserts, through the token lists of tests/deflate_tokens.py, that the corpus holds what the decoder has to meet: all
three block types, a stream of several blocks, far and near distances, the longest match, overlapping matches, every filter type."""
import collections
import functools
import io
import zlib

import numpy as np

from ctrlhair_amd import pngdec, pngenc
from tests import deflate_tokens as DT
from tests import png_oracle as PO
from tests import png_unfilter_oracle as UO

Case = collections.namedtuple('Case', 'name H W C pixels filtered stream png')     # pixels uint8 [H,W,C]

SHAPES = [(1, 1), (1, 7), (3, 5), (17, 31), (64, 64), (65, 130), (70, 53)]
# status classes (== CH_PNG_DEC_* of include/ctrlhair_hip.h)
OK, BAD_HEADER, BAD_BLOCK, BAD_CODE, BAD_SYMBOL, BAD_DISTANCE, INPUT_END, SIZE, ADLER, BAD_FILTER = range(10)


def _deflate(data: bytes, level=6, wbits=15, mem=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, wbits, mem, strategy)
    if flush_at is None:
        return co.compress(data) + co.flush()
    return co.compress(data[:flush_at]) + co.flush(zlib.Z_FULL_FLUSH) + co.compress(data[flush_at:]) + co.flush()


# name -> how the filtered bytes are deflated: stored blocks only / a fixed block / dynamic blocks / no matches (empty distance code) /
# CINFO < 7 / an empty stored block in mid-stream / many blocks per stream
VARIANTS = [
    ('stored', lambda d: _deflate(d, level=0)),
    ('fixed', lambda d: _deflate(d, strategy=zlib.Z_FIXED)),
    ('level9', lambda d: _deflate(d, level=9)),
    ('level1', lambda d: _deflate(d, level=1)),
    ('huffman_only', lambda d: _deflate(d, strategy=zlib.Z_HUFFMAN_ONLY)),
    ('wbits9', lambda d: _deflate(d, wbits=9)),
    ('full_flush', lambda d: _deflate(d, flush_at=len(d) // 2)),
    ('mem1', lambda d: _deflate(d, level=6, mem=1)),
]


def pixels_for(H: int, W: int, C: int, seed: int) -> np.ndarray:
    """uint8 [H,W,C]: a smooth ramp with noise in the upper half and few-valued steps in the lower: literals, runs and matches."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    base = (3 * xx + 5 * yy)[:, :, None] + 40 * np.arange(C)[None, None, :]
    img = (base + rng.integers(0, 6, (H, W, C))).astype(np.uint8)
    steps = (rng.integers(0, 4, (H, W, C)) * 70).astype(np.uint8)
    img[H // 2:] = steps[H // 2:]
    return img


def _case(name, pixels, filt, deflate) -> Case:
    H, W, C = pixels.shape
    filtered, _ = PO.filtered_stream(pixels, filt)
    stream = deflate(filtered)
    return Case(name, H, W, C, pixels, filtered, stream, pngenc.wrap_png(stream, H, W, C))


def _from_filtered(name, data: np.ndarray, H: int, W: int, level: int) -> Case:
    """A grey image whose FILTERED bytes are `data` (its row-start bytes forced to a filter type): the stream is what zlib makes of them."""
    d = np.array(data, np.uint8).reshape(H, 1 + W)
    d[:, 0] %= 5
    filtered = d.tobytes()
    stream = _deflate(filtered, level=level)
    return Case(name, H, W, 1, UO.unfilter(filtered, H, W, 1), filtered, stream, pngenc.wrap_png(stream, H, W, 1))


def _pillow_case(name, pixels) -> Case:
    from PIL import Image
    H, W, C = pixels.shape
    buf = io.BytesIO()
    Image.fromarray(pixels[:, :, 0] if C == 1 else pixels).save(buf, 'PNG')
    png = buf.getvalue()
    h, w, c, stream = pngdec.parse_png(png)
    assert (h, w, c) == (H, W, C)
    return Case(name, H, W, C, pixels, zlib.decompress(stream), stream, png)


@functools.lru_cache(maxsize=None)
def corpus():
    cases = []
    i = 0
    for (H, W) in SHAPES:
        for C in (1, 3, 4):
            vname, deflate = VARIANTS[i % len(VARIANTS)]
            filt = (i * 5) % 6 - 1                                                          # -1, 4, 3, 2, 1, 0, ... against the variants' 8
            cases.append(_case(f'{H}x{W}x{C}-f{filt}-{vname}', pixels_for(H, W, C, 100 + i), filt, deflate))
            i += 1
    # every variant and every fixed filter at one more shape each, so that neither depends on the rotation above
    for k, (vname, deflate) in enumerate(VARIANTS):
        cases.append(_case(f'17x31x3-f{k % 5}-{vname}', pixels_for(17, 31, 3, 200 + k), k % 5, deflate))
    rng = np.random.default_rng(7)
    block = rng.integers(0, 256, 30000, dtype=np.uint8)
    cases.append(_from_filtered('repeat30000', np.concatenate([block, block, block[:9000]]), 300, 229, 9))
    mix = np.concatenate([np.zeros(5000, np.uint8), np.tile(np.array([1, 2, 3], np.uint8), 2000), rng.integers(0, 256, 20000, dtype=np.uint8),
                          rng.integers(0, 4, 40000).astype(np.uint8) * 85])
    cases.append(_from_filtered('mix71000', mix, 500, 141, 9))
    cases.append(_case('crop256', PO.smooth_cells(1, 1, 256, seed=3)[0], -1, lambda d: _deflate(d, level=6)))
    cases.append(_pillow_case('pillow-64x64x3', pixels_for(64, 64, 3, 300)))
    cases.append(_pillow_case('pillow-70x53x1', pixels_for(70, 53, 1, 301)))
    cases.append(_pillow_case('pillow-65x130x4', pixels_for(65, 130, 4, 302)))
    cases.append(_pillow_case('pillow-label256', PO.label_map(256)[:, :, None]))
    return tuple(cases)


def check_conditions():
    """The corpus as a whole holds what the decoder must meet; a zlib that stops producing one of these is named here."""
    btypes, most_blocks, far, longest, overlap, near, filters = set(), 0, 0, 0, False, False, set()
    for c in corpus():
        tokens, out, blocks = DT.inflate_zlib(c.stream)
        assert out == c.filtered, c.name
        btypes |= {b.btype for b in blocks}
        most_blocks = max(most_blocks, len(blocks))
        for t in tokens:
            if t[0] == 'M':
                far, longest = max(far, t[2]), max(longest, t[1])
                overlap |= t[2] < t[1]
                near |= t[2] == 1
        filters |= set(np.frombuffer(c.filtered, np.uint8).reshape(c.H, 1 + c.W * c.C)[:, 0].tolist())
    assert btypes == {0, 1, 2}, f'block types in the corpus: {sorted(btypes)}'
    assert most_blocks >= 3, f'no stream of at least 3 blocks (most: {most_blocks})'
    assert far >= 24577, f'largest distance {far} < 24577'
    assert longest == 258, f'longest match {longest}'
    assert overlap, 'no match with dist < len'
    assert near, 'no match at distance 1'
    assert filters == {0, 1, 2, 3, 4}, f'filter types in the corpus: {sorted(filters)}'


# ---- the malformed set ---------------------------------------------------------------------------------------------------------------
class _BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, value: int, n: int):                                                     # n bits, least significant first
        self.bits += [(value >> k) & 1 for k in range(n)]
        return self

    def code(self, code: int, n: int):                                                     # a Huffman code, most significant bit first
        self.bits += [(code >> (n - 1 - k)) & 1 for k in range(n)]
        return self

    def bytes(self, pad_to: int = 0) -> bytes:
        bits = self.bits + [0] * (-len(self.bits) % 8)
        out = bytes(sum(bits[8 * i + k] << k for k in range(8)) for i in range(len(bits) // 8))
        return out + bytes(max(0, pad_to - len(out)))


def _dynamic_header(hlit: int, hdist: int):
    """BFINAL = 1, BTYPE = 2, and a code-length code of two 1-bit codes: '0' = length 1, '1' = symbol 18 (a run of zeros)."""
    w = _BitWriter().put(1, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(18 - 4, 4)
    for sym in [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1]:
        w.put(1 if sym in (1, 18) else 0, 3)
    return w


def _zeros(w: _BitWriter, n: int):
    while n:
        k = min(n, 138)
        assert k >= 11
        w.code(1, 1).put(k - 11, 7)
        n -= k


@functools.lru_cache(maxsize=None)
def malformed():
    """((name, zlib stream, expected status, zlib.decompress must reject it), ...) for H, W, C = 17, 31, 3."""
    H, W, C = 17, 31, 3
    px = pixels_for(H, W, C, 400)
    filtered, _ = PO.filtered_stream(px, -1)
    z, z0 = zlib.compress(filtered, 6), zlib.compress(filtered, 0)

    def patched(s, at, value):
        b = bytearray(s)
        b[at] = value
        return bytes(b)

    def header(cmf, flg_bits):
        flg = flg_bits
        flg += (31 - ((cmf << 8) | flg) % 31) % 31
        return bytes([cmf, flg]) + z[2:]

    out = [
        ('bad-fcheck', patched(z, 1, z[1] ^ 1), BAD_HEADER, True),
        ('fdict', header(0x78, 0x20), BAD_HEADER, True),
        ('cm7', header(0x77, 0x00), BAD_HEADER, True),
        ('btype3', patched(z, 2, z[2] | 0x06), BAD_BLOCK, True),
        ('stored-nlen', patched(z0, 5, z0[5] ^ 0x10), BAD_BLOCK, True),
        ('hlit287', b'\x78\x9c' + _BitWriter().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(0, 4).bytes(pad_to=64), BAD_CODE, True),
    ]
    # code-length code {0: '0', 16: '1'} (HCLEN = 4: symbols 16, 17, 18, 0), and the first code-length symbol is 16
    w = _BitWriter().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4).put(1, 3).put(0, 3).put(0, 3).put(1, 3).code(1, 1).put(0, 2)
    out.append(('repeat-first', b'\x78\x9c' + w.bytes(pad_to=64), BAD_CODE, True))
    # literal / length code: symbols 0, 1, 2 and 256 all of length 1
    w = _dynamic_header(257, 1)
    w.code(0, 1).code(0, 1).code(0, 1)
    _zeros(w, 253)
    w.code(0, 1).code(0, 1)                                                                  # symbol 256, the one distance code
    out.append(('oversubscribed', b'\x78\x9c' + w.bytes(pad_to=64), BAD_CODE, True))
    # a complete literal code (symbols 0 and 1) without the end-of-block symbol
    w = _dynamic_header(257, 1)
    w.code(0, 1).code(0, 1)
    _zeros(w, 255)
    w.code(0, 1)
    out.append(('no-eob', b'\x78\x9c' + w.bytes(pad_to=64), BAD_CODE, True))
    # fixed block whose first token is a match: length symbol 257 (7 bits 0000001), distance symbol 0 (5 bits)
    w = _BitWriter().put(1, 1).put(1, 2).code(1, 7).code(0, 5)
    out.append(('distance-first', b'\x78\x9c' + w.bytes(pad_to=64), BAD_DISTANCE, True))
    for cut in (1, 2, 10, len(z) // 2, len(z) - 3):
        out.append((f'cut{cut}', z[:cut], INPUT_END, True))
    out.append(('adler', patched(z, len(z) - 1, z[-1] ^ 0xFF), ADLER, True))
    for h in (H - 1, H + 1):
        out.append((f'rows{h}', zlib.compress(PO.filtered_stream(pixels_for(h, W, C, 401), -1)[0], 6), SIZE, False))
    f5 = bytearray(filtered)
    f5[3 * (1 + W * C)] = 5
    out.append(('filter5', zlib.compress(bytes(f5), 6), BAD_FILTER, False))
    return (H, W, C, px, z), tuple(out)
