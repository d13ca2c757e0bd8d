"""The corpus of the JPEG decoder's restart intervals (DRI, RST0..RST7), built at test time with Pillow's restart_marker_blocks= and
restart_marker_rows= (Pillow is the reference for the pixels, so no recorded files): every size x subsampling x content of the lists below
under every restart setting, the quality and optimize= cycling; files found by a deterministic seed search whose markers lie on the
boundaries of the entropy kernel's subsequences and chunks; and malformed(), streams that are invalid by construction.

coefficients() restates the entropy decode of a scan with restart markers serially, interval by interval, on tests/jpegdec_oracle.py's
tables: the checker of the coefficients csrc/jpeg_entropy_core.h gives.  It is strict where the decoder's contract is: every marker where
the interval puts it, numbered cyclically, behind fewer than 8 unread bits."""
import re
from collections import namedtuple

import numpy as np

from tests import jpegdec_cases as JC
from tests import jpegdec_oracle as JO

SIZES = ((1, 1), (3, 5), (16, 16), (17, 33), (37, 29), (100, 131))                                        # (H, W)
SUBSAMPLINGS = ('grey', 0, 1, 2)
QUALITIES = (10, 75, 100)
CONTENTS = ('noise', 'smooth', 'flat')
RESTARTS = ('b1', 'b2', 'b3', 'b7', 'rows', 'all', 'max')      # restart_marker_blocks 1, 2, 3, 7; restart_marker_rows 1; Ri = the MCU count; 65535
SUBSEQ, CHUNK = JC.SUBSEQ, JC.CHUNK
RST = re.compile(rb'\xff[\xd0-\xd7]')

Case = namedtuple('Case', 'name jpg H W C sampling ri')

_cache = {}


def mcus(H, W, C, sampling):
    hs, vs, mw, mh, _, _ = JO.geometry(H, W, C, sampling)
    return mw, mh


def restart_kw(kind, H, W, C, sampling):
    """(Pillow's keyword, the Ri the file's DRI segment then holds)."""
    mw, mh = mcus(H, W, C, sampling)
    if kind == 'rows':
        return {'restart_marker_rows': 1}, mw
    n = {'all': mw * mh, 'max': 65535}.get(kind) or int(kind[1:])
    return {'restart_marker_blocks': n}, n


def _case(name, px, sub, ri, **kw):
    c = JC._case(name, px, sub, **kw)
    return Case(c.name, c.jpg, c.H, c.W, c.C, c.sampling, ri)


def corpus():
    if 'corpus' not in _cache:
        out, seed = [], 1000
        for H, W in SIZES:
            for sub in SUBSAMPLINGS:
                for kind in CONTENTS:
                    seed += 1
                    C = 1 if sub == 'grey' else 3
                    px = JC.content(kind, H, W, C, seed)
                    for k, r in enumerate(RESTARTS):
                        q, opt = QUALITIES[(seed + k) % 3], (seed + k) % 4 == 0
                        kw, ri = restart_kw(r, H, W, C, 0 if sub == 'grey' else sub)
                        out.append(_case(f'{H}x{W}-{sub}-{kind}-{r}-q{q}{"-opt" if opt else ""}', px, sub, ri, quality=q, optimize=opt, **kw))
        _cache['corpus'] = out
    return _cache['corpus']


def scan_of(jpg: bytes) -> bytes:
    """The bytes between the SOS header and EOI, restart markers included (a marker walk of its own)."""
    at = 2
    while jpg[at + 1] != 0xDA:
        at += 2 + int.from_bytes(jpg[at + 2:at + 4], 'big')
    at += 2 + int.from_bytes(jpg[at + 2:at + 4], 'big')
    end = re.compile(rb'\xff[^\x00\xd0-\xd7]').search(jpg, at).start()
    return jpg[at:end]


def markers(scan: bytes):
    """Offsets of the restart markers' 0xFF bytes in a valid scan (0xFF 0xDn is never data: a data 0xFF is followed by 0x00)."""
    return [m.start() for m in RST.finditer(scan)]


NAMED = ('ff-last-of-subsequence', 'ff-first-of-subsequence', 'ff-last-of-chunk', 'ff-second-to-last-of-chunk')


def _named_hits(scan):
    at = markers(scan)
    return {'ff-last-of-subsequence': any(a % SUBSEQ == SUBSEQ - 1 for a in at), 'ff-first-of-subsequence': any(a and a % SUBSEQ == 0 for a in at),
            'ff-last-of-chunk': any(a % CHUNK == CHUNK - 1 for a in at), 'ff-second-to-last-of-chunk': any(a % CHUNK == CHUNK - 2 for a in at)}


def named():
    """{condition: Case}: the first seed of a fixed search (noise of 60..140 px a side, 4:4:4, quality 90, Ri 1..3) whose scan holds a
    restart marker at the named place; plus 'wraps-twice', a file of at least 17 markers."""
    if 'named' not in _cache:
        out = {}
        for seed in range(2000):
            rng = np.random.default_rng(seed)
            H, W, ri = int(rng.integers(60, 141)), int(rng.integers(60, 141)), int(rng.integers(1, 4))
            c = _case(f'seed{seed}-{H}x{W}-ri{ri}', JC.content('noise', H, W, 3, seed), 0, ri, quality=90, restart_marker_blocks=ri)
            for k, hit in _named_hits(scan_of(c.jpg)).items():
                if hit and k not in out:
                    out[k] = c
            if len(out) == len(NAMED):
                break
        px = JC.content('noise', 37, 29, 3, 5)
        out['wraps-twice'] = _case('wraps-twice', px, 0, 1, quality=75, restart_marker_blocks=1)       # 5 x 4 MCUs, 19 markers
        _cache['named'] = out
    return _cache['named']


MIXED_SHAPE = (48, 80, 3, 2)


def mixed_batch():
    """Files of one shape (H, W, C, sampling) with no restart interval, different ones, one per row and one without a marker."""
    if 'mixed' not in _cache:
        H, W, C, sub = MIXED_SHAPE
        out = []
        for i, (kind, r, q) in enumerate((('noise', None, 95), ('noise', 'b1', 75), ('smooth', 'b2', 50), ('flat', 'rows', 20), ('noise', 'b7', 100),
                                           ('checker', 'max', 100), ('smooth', None, 75), ('noise', 'b3', 90))):
            kw, ri = restart_kw(r, H, W, C, sub) if r else ({}, 0)
            out.append(_case(f'mixed-{i}-{kind}-{r}', JC.content(kind, H, W, C, 300 + i), sub, ri, quality=q, optimize=i % 2 == 1, **kw))
        _cache['mixed'] = out
    return _cache['mixed']


def many_blocks():
    """More DC values per component than one pass of the DC kernel's workgroup takes (2048), under intervals that straddle its passes,
    and one interval longer than two passes."""
    if 'many' not in _cache:
        grey, rgb = JC.content('smooth', 400, 400, 1, 1), JC.content('smooth', 400, 416, 3, 2)
        big = JC.content('smooth', 640, 640, 1, 3)
        _cache['many'] = [_case('many-grey-b7', grey, 'grey', 7, quality=75, restart_marker_blocks=7),
                          _case('many-420-rows', rgb, 2, 26, quality=75, restart_marker_rows=1),
                          _case('many-444-b3', rgb, 0, 3, quality=50, restart_marker_blocks=3),
                          _case('many-grey-b5000', big, 'grey', 5000, quality=75, restart_marker_blocks=5000)]
    return _cache['many']


def all_cases():
    return corpus() + list(named().values()) + mixed_batch() + many_blocks()


# ---- the serial restatement ------------------------------------------------------------------------------------------------------------
def tables_of(jpg: bytes) -> JO.Parsed:
    """The oracle's Parsed of the file (its scan field: the scan with its restart markers).  The oracle refuses DRI, so it is given the
    container without the DRI segment and with an empty scan."""
    at, parts = 2, [jpg[:2]]
    while True:
        n = 2 + int.from_bytes(jpg[at + 2:at + 4], 'big')
        if jpg[at + 1] != 0xDD:
            parts.append(jpg[at:at + n])
        at += n
        if jpg[at - n + 1] == 0xDA:
            break
    p = JO.parse(b''.join(parts) + b'\xff\xd9')
    return p._replace(scan=scan_of(jpg))


def _blocks(raw: bytes, count: int, first: int, bpm: int, comp_of, dcl, acl, out):
    """`count` blocks from the unstuffed bytes `raw` of one interval into out[first:], the DC predictors from 0.  Returns the bits read."""
    total = 8 * len(raw)
    buf = raw + b'\0\0\0\0\0\0'
    zz = JO.ZIGZAG.tolist()
    pred, pos = [0, 0, 0], 0

    def window(pos, n):
        b = pos >> 3
        return (int.from_bytes(buf[b:b + 5], 'big') >> (40 - (pos & 7) - n)) & ((1 << n) - 1)

    def extend(v, s):
        return v if v >> (s - 1) else v - (1 << s) + 1

    for blk in range(first, first + count):
        c = comp_of[blk % bpm]
        row = [0] * 64
        w = window(pos, 16)
        s, ln = dcl[c][0][w], dcl[c][1][w]
        if ln == 0 or s > 15:
            raise JO.Bad('invalid DC code')
        pos += ln
        diff = extend(window(pos, s), s) if s else 0
        pos += s
        pred[c] = ((pred[c] + diff + 32768) & 0xFFFF) - 32768
        row[0] = pred[c]
        k = 1
        while k < 64:
            if pos > total:
                raise JO.Bad('input exhausted')
            w = window(pos, 16)
            rs, ln = acl[c][0][w], acl[c][1][w]
            if ln == 0:
                raise JO.Bad('invalid AC code')
            pos += ln
            r, s = rs >> 4, rs & 15
            if s == 0:
                if r != 15:
                    break
                k += 16
                if k > 63:
                    raise JO.Bad('coefficient index past 63')
                continue
            k += r
            if k > 63:
                raise JO.Bad('coefficient index past 63')
            row[zz[k]] = extend(window(pos, s), s)
            pos += s
            k += 1
        if pos > total:
            raise JO.Bad('input exhausted')
        out[blk] = row
    return pos


def coefficients(p: JO.Parsed, ri: int) -> np.ndarray:
    """int64 [blocks, 64] of a scan with restart interval ri (0, or at least the MCU count: none), or JO.Bad."""
    hs, vs, mw, mh, bpm, comp_of = JO.geometry(p.H, p.W, p.C, p.sampling)
    nmcu = mw * mh
    if ri == 0 or ri >= nmcu:
        if RST.search(p.scan):
            raise JO.Bad('marker inside the scan')
        return JO.coefficients(p)
    other = re.search(rb'\xff[^\x00\xd0-\xd7]', p.scan[:-1])
    if other:
        raise JO.Bad('marker inside the scan')
    parts, numbers = RST.split(p.scan), [m.group()[1] & 7 for m in RST.finditer(p.scan)]
    if len(parts) != -(-nmcu // ri) or numbers != [k % 8 for k in range(len(parts) - 1)]:
        raise JO.Bad('restart markers')
    dcl, acl = [JO._lut(t) for t in p.dc], [JO._lut(t) for t in p.ac]
    out = np.zeros((nmcu * bpm, 64), np.int64)
    for k, part in enumerate(parts):
        raw = part.replace(b'\xff\x00', b'\xff')
        count = min(ri, nmcu - k * ri) * bpm
        used = _blocks(raw, count, k * ri * bpm, bpm, comp_of, dcl, acl, out)
        if 8 * len(raw) - used >= 8:
            raise JO.Bad('bytes left before a restart marker')
    return out


def decoded():
    """[(case, Parsed with the restart scan, coefficients)] of all_cases(), decoded once."""
    if 'decoded' not in _cache:
        out = []
        for c in all_cases():
            p = tables_of(c.jpg)
            out.append((c, p, coefficients(p, c.ri)))
        _cache['decoded'] = out
    return _cache['decoded']


def check_conditions():
    cases = all_cases()
    assert len(corpus()) == len(SIZES) * len(SUBSAMPLINGS) * len(CONTENTS) * len(RESTARTS)
    with_markers = without = optimised = 0
    for c in cases:
        scan = scan_of(c.jpg)
        n, nm = len(markers(scan)), np.prod(mcus(c.H, c.W, c.C, c.sampling))
        assert (b'\xff\xdd' in c.jpg) == (c.ri > 0), c.name
        if c.ri:
            assert c.jpg[c.jpg.index(b'\xff\xdd') + 4:][:2] == c.ri.to_bytes(2, 'big'), c.name
        assert n == (-(-nm // c.ri) - 1 if c.ri else 0), (c.name, n)
        assert [scan[a + 1] & 7 for a in markers(scan)] == [k % 8 for k in range(n)], c.name        # Pillow numbers them 0, 1, 2, ...
        with_markers += n > 0
        without += c.ri >= nm
        optimised += c.name.endswith('-opt')
    assert with_markers > 200 and without >= 2 * len(SIZES) * len(SUBSAMPLINGS) * len(CONTENTS) and optimised > 50
    nd = named()
    assert set(nd) == set(NAMED) | {'wraps-twice'}, sorted(nd)
    for k in NAMED:
        assert _named_hits(scan_of(nd[k].jpg))[k], k
    for k in ('ff-last-of-chunk', 'ff-second-to-last-of-chunk'):
        assert len(scan_of(nd[k].jpg)) > CHUNK
    assert len(markers(scan_of(nd['wraps-twice'].jpg))) >= 17
    for c in many_blocks():
        hs, vs = JO.geometry(c.H, c.W, c.C, c.sampling)[:2]
        assert np.prod(mcus(c.H, c.W, c.C, c.sampling)) * hs * vs > 2048 and 2048 % (c.ri * hs * vs), c.name     # luma DC values, and per interval
    assert many_blocks()[-1].ri > 2 * 2048
    mixed = mixed_batch()
    assert {(c.H, c.W, c.C, c.sampling) for c in mixed} == {MIXED_SHAPE}
    assert sum(c.ri == 0 for c in mixed) >= 2 and len({c.ri for c in mixed if c.ri}) >= 4


# ---- the malformed set -------------------------------------------------------------------------------------------------------------------
def malformed_base():
    """The valid file the malformed set damages: 48 x 80, 4:2:0 (5 x 3 MCUs), Ri = 2, seven markers."""
    if 'base' not in _cache:
        H, W, C, sub = MIXED_SHAPE
        _cache['base'] = _case('malformed-base', JC.content('noise', H, W, C, 11), sub, 2, quality=75, restart_marker_blocks=2)
    return _cache['base']


def malformed():
    """[(name, scan, Ri)]: the scan of malformed_base() and its Ri, each invalid by construction (the tables and sizes stay the base's).
    The streams go to the decoder as they are: a parser would keep some of them from it."""
    if 'bad' not in _cache:
        base = malformed_base()
        scan = scan_of(base.jpg)
        at = markers(scan)
        assert len(at) == 7
        # a marker with ordinary bytes around it, and the middle of an interval
        a = next(a for a in at[1:-1] if scan[a - 1] not in (0, 0xFF) and scan[a + 2] not in (0, 0xFF) and scan[a + 3] not in (0, 0xFF))
        k = at.index(a)
        mid = (at[2] + 2 + at[3]) // 2
        while scan[mid - 1] == 0xFF or scan[mid] in (0, 0xFF):
            mid += 1
        number = lambda s, i, m: s[:at[i] + 1] + bytes([0xD0 | m]) + s[at[i] + 2:]

        def renumbered(shift):
            b = bytearray(scan)
            for i, x in enumerate(at):
                b[x + 1] = 0xD0 | ((i + shift) % 8)
            return bytes(b)

        out = [
            ('marker-deleted', scan[:a] + scan[a + 2:], 2),
            ('first-marker-deleted', scan[:at[0]] + scan[at[0] + 2:], 2),
            ('markers-swapped', number(number(scan, 1, 2), 2, 1), 2),
            ('marker-one-byte-late', scan[:a] + scan[a + 2:a + 3] + scan[a:a + 2] + scan[a + 3:], 2),
            ('marker-one-byte-early', scan[:a - 1] + scan[a:a + 2] + scan[a - 1:a] + scan[a + 2:], 2),
            ('marker-number-changed', number(scan, k, (k + 1) % 8), 2),
            ('numbers-from-1', renumbered(1), 2),
            ('dri-1', scan, 1),
            ('dri-3', scan, 3),
            ('dri-4', scan, 4),
            ('dri-all', scan, 15),
            ('dri-0', scan, 0),
            ('marker-mid-block', scan[:mid] + b'\xff\xd3' + scan[mid:], 2),
            ('cut-after-marker', scan[:a + 2], 2),
            ('cut-after-first-marker', scan[:at[0] + 2], 2),
            ('marker-doubled', scan[:a + 2] + scan[a:], 2),
            ('marker-doubled-next-number', scan[:a + 2] + bytes([0xFF, 0xD0 | ((k + 1) % 8)]) + scan[a + 2:], 2),
            ('fill-ff-before-marker', scan[:a] + b'\xff' + scan[a:], 2),
            ('zero-byte-before-marker', scan[:a] + b'\x00' + scan[a:], 2),
            ('ff-c4-inside', scan[:mid] + b'\xff\xc4' + scan[mid:], 2),
            ('ff-c4-for-a-marker', scan[:a] + b'\xff\xc4' + scan[a + 2:], 2),
            ('marker-after-last-mcu', scan + b'\xff\xd7', 2),
            ('only-markers', b''.join(bytes([0xFF, 0xD0 | (i % 8)]) for i in range(7)), 2),
        ]
        _cache['bad'] = out
    return _cache['bad']
