"""Baseline JPEG decoding restated in numpy: the marker walk, a serial Huffman decoder and libjpeg's integer arithmetic after it, operation
by operation, so that the pixels equal Pillow's (libjpeg-turbo: slow-integer IDCT, fancy upsampling, 16-bit fixed-point colour) to the byte.
The checker of ch_jpeg_decode, csrc/jpeg_entropy_core.h and ctrlhair_amd.jpegdec; it shares no code with any of them.

  parse(data)            -> Parsed: sizes, sampling (0 = 4:4:4 or grey, 1 = 4:2:2, 2 = 4:2:0), per-component tables, the scan bytes
  coefficients(parsed)   -> int64 [blocks, 64] in scan order, natural order inside a block, the DC values summed up (16-bit truncation)
  pixels(parsed, coef)   -> uint8 [H, W] or [H, W, 3]
  decode(data)           -> pixels(parse(data))
COUNTERS collects, over the coefficients() calls since reset_counters(), what the streams exercised.
"""
import struct
from collections import namedtuple

import numpy as np

ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63], np.int64)

Parsed = namedtuple('Parsed', 'H W C sampling quant dc ac scan')     # quant: C x int64 [64] natural; dc / ac: C x (bits, vals)

COUNTER_NAMES = ('zrl', 'eob', 'no_eob', 'stuffed', 'max_code_len', 'max_dc_cat', 'blocks')
COUNTERS = dict.fromkeys(COUNTER_NAMES, 0)


class Bad(ValueError):
    """The stream is not one this oracle decodes, or is damaged (the reason is the message)."""


def reset_counters():
    for k in COUNTER_NAMES:
        COUNTERS[k] = 0


def parse(data: bytes) -> Parsed:
    data = bytes(data)
    if data[:2] != b'\xff\xd8':
        raise Bad('no SOI')
    pos, quant, huff, frame = 2, {}, {}, None
    while True:
        if pos + 4 > len(data) or data[pos] != 0xFF:
            raise Bad('marker expected')
        m = data[pos + 1]
        if m == 0xFF:
            pos += 1
            continue
        n = struct.unpack('>H', data[pos + 2:pos + 4])[0]
        body = data[pos + 4:pos + 2 + n]
        pos += 2 + n
        if m == 0xDB:
            while body:
                if body[0] >> 4:
                    raise Bad('16-bit quantiser')
                q = np.zeros(64, np.int64)
                q[ZIGZAG] = np.frombuffer(body[1:65], np.uint8)
                quant[body[0] & 15] = q
                body = body[65:]
        elif m == 0xC4:
            while body:
                bits = body[1:17]
                k = sum(bits)
                huff[body[0]] = (bytes(bits), bytes(body[17:17 + k]))
                body = body[17 + k:]
        elif m == 0xC0:
            P, H, W, C = struct.unpack('>BHHB', body[:6])
            frame = (P, H, W, [tuple(body[6 + 3 * k:9 + 3 * k]) for k in range(C)])
        elif m in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise Bad('not a baseline frame')
        elif m == 0xDD:
            if struct.unpack('>H', body[:2])[0]:
                raise Bad('restart interval')
        elif m == 0xDA:
            break
    P, H, W, comps = frame
    C = len(comps)
    if P != 8 or C not in (1, 3) or body[0] != C:
        raise Bad('precision, components or scan')
    samp = [c[1] for c in comps]
    if C == 1:
        sampling = 0
    else:
        if samp[1:] != [0x11, 0x11] or samp[0] not in (0x11, 0x21, 0x22):
            raise Bad('sampling')
        sampling = {0x11: 0, 0x21: 1, 0x22: 2}[samp[0]]
    sel = {body[1 + 2 * k]: body[2 + 2 * k] for k in range(C)}
    end = pos
    while True:
        end = data.index(b'\xff', end)
        if data[end + 1] != 0:
            break
        end += 2
    if data[end + 1] != 0xD9:
        raise Bad('marker inside the scan')
    return Parsed(H, W, C, sampling, [quant[c[2]] for c in comps], [huff[sel[c[0]] >> 4] for c in comps],
                  [huff[0x10 | (sel[c[0]] & 15)] for c in comps], data[pos:end])


def _lut(table):
    """(symbol, length) of every 16-bit window, length 0 where no code matches (Annex C code assignment)."""
    bits, vals = table
    sym, ln = np.zeros(65536, np.int64), np.zeros(65536, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            lo = code << (16 - length)
            sym[lo:lo + (1 << (16 - length))] = vals[k]
            ln[lo:lo + (1 << (16 - length))] = length
            code += 1
            k += 1
        code <<= 1
    return sym.tolist(), ln.tolist()


def geometry(H, W, C, sampling):
    """(hs, vs, MCUs across, MCUs down, blocks per MCU, component of each block of an MCU)."""
    if C == 1:
        return 1, 1, -(-W // 8), -(-H // 8), 1, [0]
    hs, vs = ((1, 1), (2, 1), (2, 2))[sampling]
    return hs, vs, -(-W // (8 * hs)), -(-H // (8 * vs)), hs * vs + 2, [0] * (hs * vs) + [1, 2]


def coefficients(p: Parsed) -> np.ndarray:
    hs, vs, mw, mh, bpm, comp_of = geometry(p.H, p.W, p.C, p.sampling)
    nblocks = mw * mh * bpm
    raw = p.scan.replace(b'\xff\x00', b'\xff')
    COUNTERS['stuffed'] += len(p.scan) - len(raw)
    total = 8 * len(raw)
    buf = raw + b'\0\0\0\0\0\0'
    dcl, acl = [_lut(t) for t in p.dc], [_lut(t) for t in p.ac]
    zz = ZIGZAG.tolist()
    out = np.zeros((nblocks, 64), np.int64)
    pred = [0, 0, 0]
    pos = 0

    def window(pos, n):
        b = pos >> 3
        v = int.from_bytes(buf[b:b + 5], 'big')
        return (v >> (40 - (pos & 7) - n)) & ((1 << n) - 1)

    def extend(v, s):
        return v if v >> (s - 1) else v - (1 << s) + 1

    for blk in range(nblocks):
        c = comp_of[blk % bpm]
        row = [0] * 64
        w = window(pos, 16)
        s, ln = dcl[c][0][w], dcl[c][1][w]
        if ln == 0:
            raise Bad('invalid DC code')
        COUNTERS['max_code_len'] = max(COUNTERS['max_code_len'], ln)
        COUNTERS['max_dc_cat'] = max(COUNTERS['max_dc_cat'], s)
        pos += ln
        diff = extend(window(pos, s), s) if s else 0
        pos += s
        pred[c] = ((pred[c] + diff + 32768) & 0xFFFF) - 32768
        row[0] = pred[c]
        k = 1
        while k < 64:
            w = window(pos, 16)
            rs, ln = acl[c][0][w], acl[c][1][w]
            if ln == 0:
                raise Bad('invalid AC code')
            if ln > COUNTERS['max_code_len']:
                COUNTERS['max_code_len'] = ln
            pos += ln
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r != 15:
                    COUNTERS['eob'] += 1
                    break
                COUNTERS['zrl'] += 1
                k += 16
                if k > 63:
                    raise Bad('coefficient index past 63')
                continue
            k += r
            if k > 63:
                raise Bad('coefficient index past 63')
            row[zz[k]] = extend(window(pos, s), s)
            pos += s
            k += 1
            if k == 64:
                COUNTERS['no_eob'] += 1
        if pos > total:
            raise Bad('input exhausted')
        out[blk] = row
    COUNTERS['blocks'] += nblocks
    if total - pos >= 8:
        raise Bad('bytes left after the last block')
    return out


F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
         f2562=20995, f3072=25172)


def _idct_pass(d, n):
    """jidctint.c's one-dimensional inverse over the last axis of d [..., 8], descaled by n bits."""
    desc = lambda x: (x + (1 << (n - 1))) >> n
    z2, z3 = d[..., 2], d[..., 6]
    z1 = (z2 + z3) * F['f0541']
    tmp2 = z1 - z3 * F['f1847']
    tmp3 = z1 + z2 * F['f0765']
    tmp0, tmp1 = (d[..., 0] + d[..., 4]) << 13, (d[..., 0] - d[..., 4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F['f1175']
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F['f0298'], tmp1 * F['f2053'], tmp2 * F['f3072'], tmp3 * F['f1501']
    z1, z2, z3, z4 = -z1 * F['f0899'], -z2 * F['f2562'], -z3 * F['f1961'] + z5, -z4 * F['f0390'] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.empty_like(d)
    out[..., 0], out[..., 7] = desc(tmp10 + tmp3), desc(tmp10 - tmp3)
    out[..., 1], out[..., 6] = desc(tmp11 + tmp2), desc(tmp11 - tmp2)
    out[..., 2], out[..., 5] = desc(tmp12 + tmp1), desc(tmp12 - tmp1)
    out[..., 3], out[..., 4] = desc(tmp13 + tmp0), desc(tmp13 - tmp0)
    return out


def range_limit(x):
    """libjpeg's table behind `x & 1023`, the + 128 included."""
    i = x & 1023
    return np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))


RANGE_COEF, RANGE_PASS1, RANGE_OUT = 8191, 8191, (-512, 511)


def idct(coef, q, check=True):
    """coef int64 [B, 64] natural order, q int64 [64] -> samples int64 [B, 8, 8].  Raises Bad('range') for values no sane file holds:
    beyond them libjpeg's C code (64-bit, the table behind `x & 1023`), its SIMD code (16-bit sums, saturating packs) and a 32-bit
    restatement part ways, so the device reports them (CH_JPEG_DEC_RANGE) and the file is Pillow's.  check=False: libjpeg's C code."""
    d = (coef * q[None, :]).reshape(-1, 8, 8)
    d1 = _idct_pass(d.transpose(0, 2, 1), 11).transpose(0, 2, 1)      # along the columns
    x = _idct_pass(d1, 18)                                               # along the rows
    if check and (np.abs(d).max(initial=0) > RANGE_COEF or np.abs(d1).max(initial=0) > RANGE_PASS1 or x.min(initial=0) < RANGE_OUT[0] or \
            x.max(initial=0) > RANGE_OUT[1]):
        raise Bad('range')
    return range_limit(x)


def _plane(samples, mw, mh, bpm, first, hs, vs):
    """The blocks of one component ([blocks, 8, 8] of the whole scan) as a plane [mh * vs * 8, mw * hs * 8]."""
    s = samples.reshape(mh, mw, bpm, 8, 8)[:, :, first:first + hs * vs].reshape(mh, mw, vs, hs, 8, 8)
    return s.transpose(0, 2, 4, 1, 3, 5).reshape(mh * vs * 8, mw * hs * 8)


def upsample_h2v1(p):
    if p.shape[1] <= 2:
        return np.repeat(p, 2, axis=1)
    left, right = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    out = np.empty((p.shape[0], 2 * p.shape[1]), np.int64)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def upsample_h2v2(p):
    if p.shape[1] <= 2:
        return np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)
    up, down = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    rows = np.empty((2 * p.shape[0], p.shape[1]), np.int64)
    rows[0::2], rows[1::2] = 3 * p + up, 3 * p + down
    left, right = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    out = np.empty((rows.shape[0], 2 * rows.shape[1]), np.int64)
    out[:, 0::2] = (3 * rows + left + 8) >> 4
    out[:, 1::2] = (3 * rows + right + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr):
    fix = lambda x: int(x * 65536 + 0.5)
    cb, cr = cb - 128, cr - 128
    r = y + ((fix(1.40200) * cr + 32768) >> 16)
    g = y + ((-fix(0.34414) * cb - fix(0.71414) * cr + 32768) >> 16)
    b = y + ((fix(1.77200) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def pixels(p: Parsed, coef: np.ndarray, check=True) -> np.ndarray:
    hs, vs, mw, mh, bpm, comp_of = geometry(p.H, p.W, p.C, p.sampling)
    comp = np.tile(np.array(comp_of), mw * mh)
    samples = np.zeros((coef.shape[0], 8, 8), np.int64)
    for c in range(p.C):
        samples[comp == c] = idct(coef[comp == c], p.quant[c], check)
    y = _plane(samples, mw, mh, bpm, 0, hs, vs)[:p.H, :p.W]
    if p.C == 1:
        return y.astype(np.uint8)
    ch, cw = -(-p.H // vs), -(-p.W // hs)
    planes = []
    for c in (1, 2):
        pl = _plane(samples, mw, mh, bpm, hs * vs + c - 1, 1, 1)[:ch, :cw]
        if p.sampling == 1:
            pl = upsample_h2v1(pl)
        elif p.sampling == 2:
            pl = upsample_h2v2(pl)
        planes.append(pl[:p.H, :p.W])
    return ycc_to_rgb(y, planes[0], planes[1])


def decode(data: bytes) -> np.ndarray:
    p = parse(data)
    return pixels(p, coefficients(p))
