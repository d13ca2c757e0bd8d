"""Baseline JPEG encoding restated in numpy: libjpeg's arithmetic, operation by operation, so that the files equal Pillow's
(libjpeg-turbo, optimize=False) to the byte.  The checker of ch_jpeg_encode and ctrlhair_amd.jpegenc; it shares no code with either.

  colour      jccolor's 16-bit fixed point (FIX(x) = int(x * 65536 + 0.5))
  4:2:0       (a + b + c + d + bias) >> 2 over 2x2, bias 1, 2, 1, 2 along the output columns
  edges       luma replicated to whole blocks; chroma: last row to an even height, last column out to whole chroma blocks, downsample,
              last downsampled row to whole blocks; a luma block of a 2x2 MCU beyond ceil(W/8) or ceil(H/8) is a dummy block: AC zero,
              DC that of the block before it in MCU order
  transform   level shift, the slow-integer forward DCT (CONST_BITS 13, PASS1_BITS 2; 8 x the DCT), quantiser (|c| + (q8 >> 1)) // q8
  entropy     the Annex K.3 Huffman tables, no restart markers, 1-bit padding, 0x00 after every 0xFF

scan(img, quality, subsampling) -> the entropy-coded bytes between the SOS header and EOI;  file(...) -> the whole file.
COUNTERS collects, over the calls since reset_counters(), what the inputs exercised.
"""
import struct

import numpy as np

BASE_LUMA = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    np.int64)
BASE_CHROMA = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99], np.int64)
# natural index of zigzag position k
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)

# Annex K.3: (number of codes of length 1..16, symbols in code order)
DC_LUMA = (bytes.fromhex('00010501010101010100000000000000'), bytes(range(12)))
DC_CHROMA = (bytes.fromhex('00030101010101010101010000000000'), bytes(range(12)))
AC_LUMA = (bytes.fromhex('0002010303020403050504040000017d'), bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a'
    '535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7'
    'c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa'))
AC_CHROMA = (bytes.fromhex('00020102040403040705040400010277'), bytes.fromhex(
    '0001020311040521310612415107617113223281081442'
    '91a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a535455565758595a636465666768696a737475767778'
    '797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9ea'
    'f2f3f4f5f6f7f8f9fa'))

COUNTER_NAMES = ('zrl', 'eob', 'no_eob', 'stuffed', 'dummy', 'max_dc_cat', 'max_ac_size')
COUNTERS = dict.fromkeys(COUNTER_NAMES, 0)


def reset_counters():
    for k in COUNTER_NAMES:
        COUNTERS[k] = 0


def quant_tables(quality):
    """(luma, chroma) int64 [64] in natural order: jpeg_quality_scaling and jpeg_add_quant_table with force_baseline."""
    q = int(quality)
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((base * s + 50) // 100, 1, 255) for base in (BASE_LUMA, BASE_CHROMA))


def _codes(table):
    """symbol -> (code, length), Annex C."""
    bits, vals = table
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _lut(table, n):
    code, length = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for sym, (c, ln) in _codes(table).items():
        code[sym], length[sym] = c, ln
    return code, length


def ycc(rgb):
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    fix = lambda x: int(x * 65536 + 0.5)
    half, off = 32768, 128 << 16
    y = (fix(0.29900) * r + fix(0.58700) * g + fix(0.11400) * b + half) >> 16
    cb = (-fix(0.16874) * r - fix(0.33126) * g + fix(0.50000) * b + off + half - 1) >> 16
    cr = (fix(0.50000) * r - fix(0.41869) * g - fix(0.08131) * b + off + half - 1) >> 16
    return y, cb, cr


def _pad(plane, rows, cols):
    return np.pad(plane, ((0, rows - plane.shape[0]), (0, cols - plane.shape[1])), mode='edge')


def _ceil(a, b):
    return -(-a // b)


def downsample_420(plane):
    """h2v2_downsample with libjpeg's edge order; returns the plane padded to whole 8x8 blocks."""
    H, W = plane.shape
    bw = _ceil(_ceil(W, 2), 8)
    p = _pad(plane, H + (H & 1), 2 * 8 * bw)
    bias = np.tile(np.array([1, 2], np.int64), 4 * bw)[None, :]
    d = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    return _pad(d, 8 * _ceil(d.shape[0], 8), d.shape[1])


def _pass(d, first):
    """One pass of jfdctint.c over the last axis of d [..., 8]."""
    C = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
             f2562=20995, f3072=25172)
    CONST_BITS, PASS1_BITS = 13, 2
    desc = lambda x, n: (x + (1 << (n - 1))) >> n
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = np.empty_like(d)
    n = CONST_BITS - PASS1_BITS if first else CONST_BITS + PASS1_BITS
    if first:
        out[..., 0], out[..., 4] = (t10 + t11) << PASS1_BITS, (t10 - t11) << PASS1_BITS
    else:
        out[..., 0], out[..., 4] = desc(t10 + t11, PASS1_BITS), desc(t10 - t11, PASS1_BITS)
    z1 = (t12 + t13) * C['f0541']
    out[..., 2] = desc(z1 + t13 * C['f0765'], n)
    out[..., 6] = desc(z1 - t12 * C['f1847'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * C['f1175']
    t4, t5, t6, t7 = t4 * C['f0298'], t5 * C['f2053'], t6 * C['f3072'], t7 * C['f1501']
    z1, z2, z3, z4 = -z1 * C['f0899'], -z2 * C['f2562'], -z3 * C['f1961'] + z5, -z4 * C['f0390'] + z5
    out[..., 7] = desc(t4 + z1 + z3, n)
    out[..., 5] = desc(t5 + z2 + z4, n)
    out[..., 3] = desc(t6 + z2 + z3, n)
    out[..., 1] = desc(t7 + z1 + z4, n)
    return out


def blocks_quantised(plane, qtab):
    """plane int64 [8a, 8b] -> quantised coefficients int64 [a, b, 64] in zigzag order."""
    a, b = plane.shape[0] // 8, plane.shape[1] // 8
    d = plane.reshape(a, 8, b, 8).transpose(0, 2, 1, 3) - 128          # [a, b, row, col]
    d = _pass(d, True)                                                 # along the rows
    d = _pass(d.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)    # along the columns
    c = d.reshape(a, b, 64)
    q8 = (qtab << 3)[None, None, :]
    mag = (np.abs(c) + (q8 >> 1)) // q8
    return (np.sign(c) * mag)[..., ZIGZAG]


def _bit_length(v):
    n = np.zeros(v.shape, np.int64)
    for k in range(16):
        n += (v >> k) > 0
    return n


def scan_blocks(img, quality, subsampling):
    """The blocks of the scan in coding order: (coef int64 [B, 64] zigzag, comp int64 [B] 0 / 1 / 2)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        img = img[..., None]
    H, W, C = img.shape
    assert C in (1, 3) and subsampling in (0, 2)
    ql, qc = quant_tables(quality)
    bh, bw = _ceil(H, 8), _ceil(W, 8)
    if C == 1:
        y = blocks_quantised(_pad(img[..., 0].astype(np.int64), 8 * bh, 8 * bw), ql)
        return y.reshape(-1, 64), np.zeros(bh * bw, np.int64)
    y, cb, cr = ycc(img)
    if subsampling == 0:
        planes = [blocks_quantised(_pad(p, 8 * bh, 8 * bw), q) for p, q in ((y, ql), (cb, qc), (cr, qc))]
        coef = np.stack(planes, axis=2).reshape(-1, 64)                # [bh, bw, 3, 64]
        return coef, np.tile(np.arange(3), bh * bw)
    mh, mw = _ceil(H, 16), _ceil(W, 16)
    yq = blocks_quantised(_pad(y, 16 * mh, 16 * mw), ql)               # the blocks beyond bh / bw are overwritten below
    yq = yq.reshape(mh, 2, mw, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, 4, 64).copy()
    for k in range(1, 4):                                              # dummy blocks, in MCU order so that the DC chains
        dummy = np.zeros((mh, mw), bool)
        if k & 1:
            dummy[:, 2 * np.arange(mw) + 1 >= bw] = True
        if k & 2:
            dummy[2 * np.arange(mh) + 1 >= bh, :] = True
        yq[dummy, k, 1:] = 0
        yq[dummy, k, 0] = yq[dummy, k - 1, 0]
        COUNTERS['dummy'] += int(dummy.sum())
    cbq, crq = (blocks_quantised(downsample_420(p), qc) for p in (cb, cr))
    assert cbq.shape[:2] == (mh, mw)
    coef = np.concatenate([yq, cbq[:, :, None], crq[:, :, None]], axis=2).reshape(-1, 64)
    return coef, np.tile(np.array([0, 0, 0, 0, 1, 2]), mh * mw)


def entropy_code(coef, comp):
    """Huffman-code the blocks (in coding order), pad with 1-bits and stuff; returns bytes."""
    B = coef.shape[0]
    chroma = comp > 0
    pred = np.zeros(B, np.int64)
    for c in range(3):
        idx = np.nonzero(comp == c)[0]
        if len(idx):
            pred[idx[1:]] = coef[idx[:-1], 0]
    dc_code = [_lut(t, 12) for t in (DC_LUMA, DC_CHROMA)]
    ac_code = [_lut(t, 256) for t in (AC_LUMA, AC_CHROMA)]
    pick = lambda tabs, sym, k: np.where(chroma if sym.ndim == 1 else chroma[:, None], tabs[1][k][sym], tabs[0][k][sym])
    # every block: DC | 63 x (3 ZRL slots, 1 symbol slot) | EOB; unused slots have length 0
    val, nbits = np.zeros((B, 254), np.int64), np.zeros((B, 254), np.int64)
    diff = coef[:, 0] - pred
    cat = _bit_length(np.abs(diff))
    extra = np.where(diff < 0, diff - 1, diff) & ((1 << cat) - 1)
    val[:, 0] = (pick(dc_code, cat, 0) << cat) | extra
    nbits[:, 0] = pick(dc_code, cat, 1) + cat
    ac = coef[:, 1:]
    nz = ac != 0
    pos = np.arange(1, 64)[None, :]
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=1)
    prev = np.concatenate([np.zeros((B, 1), np.int64), last[:, :-1]], axis=1)       # position of the non-zero before k (0: the DC)
    run = np.where(nz, pos - prev - 1, 0)
    size = np.where(nz, _bit_length(np.abs(ac)), 0)
    sym = ((run & 15) << 4) | size
    extra = np.where(ac < 0, ac - 1, ac) & ((1 << size) - 1)
    zrl_code, zrl_len = pick(ac_code, np.full(B, 0xF0), 0), pick(ac_code, np.full(B, 0xF0), 1)
    for j in range(3):
        on = nz & ((run >> 4) > j)
        val[:, 1 + j:253:4] = np.where(on, zrl_code[:, None], 0)
        nbits[:, 1 + j:253:4] = np.where(on, zrl_len[:, None], 0)
    val[:, 4:253:4] = np.where(nz, (pick(ac_code, sym, 0) << size) | extra, 0)
    nbits[:, 4:253:4] = np.where(nz, pick(ac_code, sym, 1) + size, 0)
    eob = ~nz[:, 62]
    val[:, 253] = np.where(eob, pick(ac_code, np.zeros(B, np.int64), 0), 0)
    nbits[:, 253] = np.where(eob, pick(ac_code, np.zeros(B, np.int64), 1), 0)
    COUNTERS['zrl'] += int((np.where(nz, run >> 4, 0)).sum())
    COUNTERS['eob'] += int(eob.sum())
    COUNTERS['no_eob'] += int((~eob).sum())
    COUNTERS['max_dc_cat'] = max(COUNTERS['max_dc_cat'], int(cat.max()))
    COUNTERS['max_ac_size'] = max(COUNTERS['max_ac_size'], int(size.max()))
    # the pieces as one bit string, MSB first
    val, nbits = val.reshape(-1), nbits.reshape(-1)
    keep = nbits > 0
    val, nbits = val[keep], nbits[keep]
    total = int(nbits.sum())
    start = np.cumsum(nbits) - nbits
    within = np.arange(total) - np.repeat(start, nbits)
    bits = ((np.repeat(val, nbits) >> (np.repeat(nbits, nbits) - 1 - within)) & 1).astype(np.uint8)
    bits = np.concatenate([bits, np.ones((-total) % 8, np.uint8)])
    raw = np.packbits(bits)
    ff = raw == 0xFF
    COUNTERS['stuffed'] += int(ff.sum())
    out = np.zeros(len(raw) + int(ff.sum()), np.uint8)
    out[np.arange(len(raw)) + np.cumsum(ff) - ff] = raw
    return out.tobytes()


def scan(img, quality=75, subsampling=2):
    return entropy_code(*scan_blocks(img, quality, subsampling))


def _segment(marker, payload):
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


def file(img, quality=75, subsampling=2):
    """The whole file as Pillow writes it: SOI, APP0, DQT per table, SOF0, DHT per table, SOS, scan, EOI."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    C = 1 if img.ndim == 2 else img.shape[2]
    ql, qc = quant_tables(quality)
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    for k, q in enumerate((ql, qc)[:1 if C == 1 else 2]):
        out.append(_segment(0xDB, bytes([k]) + bytes(int(v) for v in q[ZIGZAG])))
    samp = 0x22 if subsampling == 2 else 0x11      # Pillow sets the factor for grey as well; one component: no effect on the scan
    comps = [(1, samp, 0)] + ([(2, 0x11, 1), (3, 0x11, 1)] if C == 3 else [])
    out.append(_segment(0xC0, struct.pack('>BHHB', 8, H, W, C) + b''.join(bytes(c) for c in comps)))
    tables = [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([(0x01, DC_CHROMA), (0x11, AC_CHROMA)] if C == 3 else [])
    for ident, (bits, vals) in tables:
        out.append(_segment(0xC4, bytes([ident]) + bits + vals))
    sel = [(1, 0x00)] + ([(2, 0x11), (3, 0x11)] if C == 3 else [])
    out.append(_segment(0xDA, bytes([C]) + b''.join(bytes(s) for s in sel) + b'\x00\x3f\x00'))
    out.append(scan(img, quality, subsampling))
    out.append(b'\xff\xd9')
    return b''.join(out)
