"""The JPEG decoder's corpus, built at test time with Pillow (Pillow is the reference, so no recorded files): every size x subsampling x
quality x optimize x content of the lists below, a few files made for single conditions, and three larger streams that span three or more
chunks of the entropy kernel.  malformed() is the set the sanitizer program and the device must answer with a status, never with a fault.
check_conditions() asserts that the corpus holds what can go wrong."""
import io
from collections import namedtuple

import numpy as np

from tests import jpegdec_oracle as JO

SIZES = ((1, 1), (2, 2), (3, 5), (5, 4), (9, 3), (7, 9), (16, 16), (17, 33), (37, 29), (100, 131))        # (H, W)
SUBSAMPLINGS = ('grey', 0, 1, 2)                                                                          # Pillow's numbers: 4:4:4, 4:2:2, 4:2:0
QUALITIES = (1, 10, 75, 95, 100)
CONTENTS = ('noise', 'smooth', 'flat')
SUBSEQ, CHUNK = 128, 128 * 64             # bytes per lane and per workgroup of the entropy kernel (csrc/jpeg_entropy_core.h)

Case = namedtuple('Case', 'name jpg H W C sampling')

_cache = {}


def content(kind: str, H: int, W: int, C: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if kind == 'noise':
        a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    elif kind == 'smooth':
        y, x = np.mgrid[0:H, 0:W]
        a = np.stack([(y * (3 + c) + x * (5 - c) + 40 * c) % 256 if c == 1 else 255 * (y + (c + 1) * x) // max(H + (c + 1) * W, 1)
                      for c in range(C)], -1).astype(np.uint8)
    elif kind == 'flat':
        a = np.broadcast_to(rng.integers(0, 256, (1, 1, C), dtype=np.uint8), (H, W, C)).copy()
    elif kind == 'checker':               # 8 x 8 blocks of 0 and 255: DC differences of category 11 at quality 100
        y, x = np.mgrid[0:H, 0:W]
        a = np.broadcast_to(((((y // 8) + (x // 8)) & 1) * 255).astype(np.uint8)[:, :, None], (H, W, C)).copy()
    else:
        raise ValueError(kind)
    return a[:, :, 0] if C == 1 else a


def save(px: np.ndarray, **kw) -> bytes:
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def _case(name, px, sub, **kw):
    C = 1 if px.ndim == 2 else 3
    jpg = save(px, **({} if sub == 'grey' else {'subsampling': sub}), **kw)
    return Case(name, jpg, px.shape[0], px.shape[1], C, 0 if sub == 'grey' else sub)


def corpus():
    if 'corpus' not in _cache:
        out, seed = [], 0
        for H, W in SIZES:
            for sub in SUBSAMPLINGS:
                for kind in CONTENTS:
                    seed += 1
                    px = content(kind, H, W, 1 if sub == 'grey' else 3, seed)
                    for q in QUALITIES:
                        for opt in (False, True):
                            out.append(_case(f'{H}x{W}-{sub}-{kind}-q{q}{"-opt" if opt else ""}', px, sub, quality=q, optimize=opt))
        for sub in SUBSAMPLINGS:
            out.append(_case(f'checker-{sub}', content('checker', 40, 56, 1 if sub == 'grey' else 3, 0), sub, quality=100))
        _cache['corpus'] = out
    return _cache['corpus']


def sync_streams():
    """Three streams of three or more chunks each: the hand-over between workgroups."""
    if 'sync' not in _cache:
        noise = content('noise', 256, 256, 3, 77)
        y, x = np.mgrid[0:200, 0:320]
        grad = np.stack([255 * (y + x) // 518, 255 - 255 * (2 * y + x) // 718, 255 * (y + 3 * x) // 1156], -1).astype(np.uint8)
        _cache['sync'] = [_case('sync-noise-444', noise, 0, quality=95), _case('sync-noise-420-opt', noise, 2, quality=95, optimize=True),
                          _case('sync-gradient-q100', grad, 0, quality=100)]
    return _cache['sync']


def scan_of(jpg: bytes) -> bytes:
    return JO.parse(jpg).scan


def splice(jpg: bytes, scan: bytes) -> bytes:
    """The file with its entropy-coded scan replaced."""
    old = scan_of(jpg)
    at = jpg.rindex(old)
    return jpg[:at] + scan + jpg[at + len(old):]


def malformed():
    """[(name, file bytes)]: damaged scans inside intact containers, and one damaged Huffman table.  Some still decode (a flipped bit may
    leave a valid stream); the rule for every one is: a non-zero status, or Pillow's pixels."""
    if 'bad' not in _cache:
        base = _case('base', content('noise', 37, 29, 3, 5), 2, quality=75).jpg
        scan = scan_of(base)
        out = [(f'cut-{k}', splice(base, scan[:k])) for k in range(0, len(scan), 97)]
        rng = np.random.default_rng(9)
        for k in rng.integers(0, 8 * len(scan), 200).tolist():
            s = bytearray(scan)
            s[k >> 3] ^= 0x80 >> (k & 7)
            out.append((f'flip-{k}', splice(base, bytes(s))))
        # a Huffman table with an unused code the data hits: an optimised AC table holds only symbols the scan uses; its last symbol is
        # dropped (the count taken from the longest length, the segment one byte shorter), so the code it had is no code any more
        grey = _case('g', content('noise', 16, 16, 1, 3), 'grey', quality=100, optimize=True).jpg
        at = 2
        while not (grey[at + 1] == 0xC4 and grey[at + 4] >> 4 == 1):
            at += 2 + int.from_bytes(grey[at + 2:at + 4], 'big')
        n = int.from_bytes(grey[at + 2:at + 4], 'big')
        seg = bytearray(grey[at:at + 2 + n])
        seg[5 + max(i for i in range(16) if seg[5 + i])] -= 1
        seg[2:4] = (n - 1).to_bytes(2, 'big')
        out.append(('unused-code', grey[:at] + bytes(seg[:-1]) + grey[at + 2 + n:]))
        out.append(('empty-scan', splice(base, b'')))
        out.append(('all-ff00', splice(base, b'\xff\x00' * (len(scan) // 2))))
        _cache['bad'] = out
    return _cache['bad']


def decoded():
    """[(case, oracle's Parsed, oracle's coefficients)] of corpus() + sync_streams(), decoded once; the oracle's counters over them."""
    if 'decoded' not in _cache:
        JO.reset_counters()
        out = []
        for c in corpus() + sync_streams():
            p = JO.parse(c.jpg)
            out.append((c, p, JO.coefficients(p)))
        _cache['decoded'] = (out, dict(JO.COUNTERS))
    return _cache['decoded']


def check_conditions():
    ff_on_boundary = dummy = narrow_chroma = 0
    cases, n = decoded()
    for c, p, _ in cases:
        assert (p.H, p.W, p.C, p.sampling) == (c.H, c.W, c.C, c.sampling), c.name
        s = p.scan
        ff_on_boundary += sum(1 for i in range(SUBSEQ, len(s), SUBSEQ) if s[i] == 0xFF or s[i - 1] == 0xFF)
        if c.C == 3 and c.sampling:
            hs, vs = ((2, 1), (2, 2))[c.sampling - 1]
            dummy += (-(-c.W // 8)) % hs + ((-(-c.H // 8)) % vs)
            narrow_chroma += -(-c.W // 2) <= 2
    assert n['zrl'] > 0 and n['no_eob'] > 0 and n['eob'] > 0 and n['stuffed'] > 0, n
    assert n['max_code_len'] == 16 and n['max_dc_cat'] == 11, n
    assert ff_on_boundary > 0 and dummy > 0 and narrow_chroma > 0
    for c in sync_streams():
        assert len(scan_of(c.jpg)) > 2 * CHUNK, (c.name, len(scan_of(c.jpg)))


def hostile(kind: str, sub) -> bytes:
    """A quality-100 file with every quantiser set to 255, so that the coefficients are far beyond what samples of 8 bits give.  On
    'checker' (DC only) libjpeg's C code with its `x & 1023` table and libjpeg-turbo's SIMD code still agree; on 'noise' they do not."""
    j = bytearray(_case('h', content(kind, 40, 56, 1 if sub == 'grey' else 3, 0), sub, quality=100).jpg)
    at = 2
    while j[at + 1] != 0xDA:
        n = int.from_bytes(j[at + 2:at + 4], 'big')
        if j[at + 1] == 0xDB:
            j[at + 5:at + 69] = bytes([255]) * 64
        at += 2 + n
    return bytes(j)
