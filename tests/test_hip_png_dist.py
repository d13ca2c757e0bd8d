"""ch_png_encode_dist on the GPU (csrc/png_encode.hip): matches at caller-given distances.  Every stream inflates
to the numpy oracle's filtered bytes and decodes to the pixels; per chunk the token sequence is the one tests/png_dist_oracle.parse
derives from the rule; nothing changes where no distance is given; the sheets shrink as the rule promises.

Measured ratios device (cell stride) / chunked zlib level 6 (deterministic; printed by test_sizes, table in DESIGN.md section 16):
sheet 2x4 cells of 40 margin 0: 0.9718, margin 4: 0.9677, sheet 3x7 cells of 64: 0.9392, the first under filter 0: 0.9988 -> MARGIN = the
largest rounded up to the next 0.05."""
import collections
import ctypes
import io
import os
import zlib

import numpy as np
import pytest
import torch

from ctrlhair_amd import directions as DS
from ctrlhair_amd import lib as L
from ctrlhair_amd import pngenc as PE
from ctrlhair_amd import procedural as P
from tests import deflate_tokens as DT
from tests import png_dist_oracle as DO
from tests import png_oracle as PO

pytestmark = pytest.mark.gpu
ERR_ARG = 1
NGF = 16
MODES = {1: 'L', 3: 'RGB', 4: 'RGBA'}
MARGIN = 1.00
SHEETS = {'sheet0': (2, 3, 40, 0), 'sheet4': (2, 3, 40, 4)}


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


@pytest.fixture(scope='module')
def enc(handle):
    return PE.PngEncoder(handle, 'cuda:0')


@pytest.fixture(scope='module')
def K(enc):
    assert enc.chunk == 32768                                                              # the constructed streams below are laid out for it
    return enc.chunk


_wanted = {}


def _want(img: np.ndarray, filt: int) -> bytes:
    """png_oracle.filtered_stream, computed once per (image, filter)."""
    key = (img.shape, filt, img.tobytes())
    if key not in _wanted:
        _wanted[key] = PO.filtered_stream(img, filt)[0]
    return _wanted[key]


def _check(enc, imgs: np.ndarray, filt: int, D):
    """Encode a batch [N,H,W,C] / [N,H,W] with distances D; every stream against the oracle, every file against the pixels.  -> streams"""
    from PIL import Image
    streams = enc.streams(torch.from_numpy(np.ascontiguousarray(imgs)).cuda(), filt, distances=D)
    N, H, W = imgs.shape[:3]
    C = imgs.shape[3] if imgs.ndim == 4 else 1
    bound = int(enc.handle.lib.ch_png_zlib_bound(H, W, C))
    assert len(streams) == N
    for n, s in enumerate(streams):
        assert len(s) <= bound
        d = zlib.decompressobj()
        got = d.decompress(s)
        assert d.eof and d.unused_data == b'' and d.unconsumed_tail == b''
        assert got == _want(imgs[n], filt), (imgs.shape, filt, D, n)
        im = Image.open(io.BytesIO(PE.wrap_png(s, H, W, C)))
        im.load()
        assert im.mode == MODES[C] and np.array_equal(np.asarray(im).reshape(imgs[n].shape), imgs[n])
    return streams


def _chunks(stream: bytes, K: int):
    """A device stream -> per chunk (tokens or None for a stored chunk, the chunk's bytes).  The layout of DESIGN.md section 16: per
    chunk a dynamic block followed by an empty stored block, or one stored block; at the end an empty fixed block."""
    tokens, out, blocks = DT.inflate_zlib(stream)
    assert blocks[-1].btype == 1 and blocks[-1].final and blocks[-1].out_start == blocks[-1].out_end
    res, k = [], 0
    body = blocks[:-1]
    while k < len(body):
        b = body[k]
        assert b.out_start == len(res) * K and b.out_end == min(len(out), b.out_start + K), (k, b)
        if b.btype == 2:
            e = body[k + 1]
            assert e.btype == 0 and e.out_start == e.out_end and e.bit_end % 8 == 0        # the realigning empty stored block
            used = {DT.DIST_BASE.index(max(v for v in DT.DIST_BASE if v <= t[2])) for t in tokens[b.tok_start:b.tok_end] if t[0] == 'M'}
            coded = {s for s, l in enumerate(b.dist_lengths) if l}
            assert coded == (used or {0}) and (len(used) > 1 or set(b.dist_lengths) <= {0, 1})     # one used symbol, or none: one bit
            res.append((tokens[b.tok_start:b.tok_end], out[b.out_start:b.out_end]))
            k += 2
        else:
            assert b.btype == 0 and b.out_end > b.out_start
            res.append((None, out[b.out_start:b.out_end]))
            k += 1
    assert len(res) == (len(out) + K - 1) // K
    return res


def _check_tokens(enc, img: np.ndarray, filt: int, D, K: int, stored_ok: bool = False):
    """_check, and per chunk the device's tokens equal the oracle's parse.  -> [(tokens | None, chunk bytes)]"""
    chunks = _chunks(_check(enc, img[None], filt, D)[0], K)
    for k, (tokens, data) in enumerate(chunks):
        if tokens is None:
            assert stored_ok, (k, D)
            continue
        pos = 0
        for t in tokens:                                                                   # no match reaches before its chunk's start
            assert t[0] == 'L' or (t[2] in (1,) + tuple(D) and 3 <= t[1] <= 258 and pos - t[2] >= 0), (k, t, pos)
            pos += 1 if t[0] == 'L' else t[1]
        want = DO.parse(data, D)
        if tokens != want:
            first = next(i for i, (a, b) in enumerate(zip(tokens + [None], want + [None])) if a != b)
            raise AssertionError(f'chunk {k}, distances {D}: token {first} is {tokens[first:first + 3]}, the rule gives {want[first:first + 3]}')
    return chunks


def _sheet(name: str, C: int = 3) -> np.ndarray:
    s = DO.sheet(*SHEETS[name])
    return s[..., 0].copy() if C == 1 else s if C == 3 else np.concatenate([s, s[..., :1]], axis=2)


def _stride(name: str, C: int = 3) -> int:
    _, _, cell, margin = SHEETS[name]
    return (cell + margin) * C


def _lists(C: int, stride: int):
    return [(C,) if C > 1 else (2,), (stride,), (3, stride) if stride != 3 else (3, 5), (127,), (128,), (129,), (258,), (32767,),
            (6000,),                                                                       # longer than the sheets' short last chunk
            (3 if stride != 3 else 5, stride, 128)]


# ---- 1. pixels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('shape', [(1, 1), (3, 5), (17, 31), (70, 53), 'sheet0', 'sheet4'])
def test_pixels_for_every_distance_list(enc, shape, C):
    if isinstance(shape, str):
        img, stride = _sheet(shape, C), _stride(shape, C)
    else:
        H, W = shape
        rng = np.random.default_rng(1000 * H + 10 * W + C)
        img = (rng.integers(0, 4, (H, W, C)) * 70).astype(np.uint8)                        # few values: intervals of every distance
        stride = max(1 + W * C, 2)                                                         # the row pitch of the filtered stream
    if C == 1:
        img = img.reshape(img.shape[:2])
    for filt in (-1, 0, 1, 4):
        for D in _lists(C, stride):
            _check(enc, img[None], filt, D)


# ---- 2. tokens -------------------------------------------------------------------------------------------------------------------------
def _image(stream: np.ndarray, K: int) -> np.ndarray:
    """The grey image [2, K - 1] whose filter-0 stream is `stream` [2 * K], two whole chunks -- up to the two type bytes, positions 0
    and K (the first byte of either chunk), which are 0 whatever `stream` holds there."""
    assert stream.shape == (2 * K,) and stream.dtype == np.uint8
    return stream.reshape(2, K)[:, 1:].copy()


@pytest.fixture(scope='module')
def streams_in(K):
    rng = np.random.default_rng(7)
    return {'tile': _image(DO.tile(2 * K), K), 'noise': _image(rng.integers(0, 256, 2 * K, dtype=np.uint8), K),
            'zeros': _image(np.zeros(2 * K, np.uint8), K)}


@pytest.mark.parametrize('which', range(10))
def test_tokens_are_the_rules(enc, K, streams_in, which):
    for name in SHEETS:
        D = _lists(3, _stride(name))[which]
        for filt in (-1, 0):
            assert len(_check_tokens(enc, _sheet(name), filt, D, K)) == 2                  # (no chunk of a sheet is stored)
    D = _lists(3, 120)[which]
    assert len(_check_tokens(enc, streams_in['tile'], 0, D, K)) == 2                       # (nor of the tile)
    noise = _check_tokens(enc, streams_in['noise'], 0, D, K, stored_ok=True)
    assert [t for t, _ in noise] == [None, None]
    for tokens, _ in _check_tokens(enc, streams_in['zeros'], 0, D, K):
        assert {t[2] for t in tokens if t[0] == 'M'} == {1} and tokens[0] == ('L', 0)


def test_the_stride_is_used_on_a_sheet(enc, K):
    for name in SHEETS:
        d = _stride(name)
        chunks = _check_tokens(enc, _sheet(name), -1, (d,), K)
        covered = sum(t[1] for tokens, _ in chunks for t in tokens if t[0] == 'M' and t[2] == d)
        assert covered > sum(len(data) for _, data in chunks) // 3


# ---- 3. constructed streams (filter 0) ----------------------------------------------------------------------------------------------------
def _background(K: int, seed: int) -> np.ndarray:
    """Two chunks of noise, each with one run of 10 000 sevens at [12000, 22000) -- 38 matches (258, 1) and one (195, 1) -- so that the
    chunk is coded, not stored, whatever little a test adds; the tests build their cases outside the run."""
    s = np.random.default_rng(seed).integers(0, 256, 2 * K, dtype=np.uint8)
    for base in (0, K):
        s[base + 12000:base + 22000] = 7
        s[base + 11999], s[base + 22000] = 8, 8
    return s


def _repeat(s: np.ndarray, a: int, b: int, d: int) -> None:
    """Make eq_d hold on exactly [a, b): s[i] = s[i - d] there, byte after byte (b - a may exceed d), and not at a - 1 nor at b."""
    if s[a - 1] == s[a - 1 - d]:
        s[a - 1] ^= 1
    for i in range(a, b):
        s[i] = s[i - d]
    if s[b] == s[b - d]:
        s[b] ^= 1


def _matches(chunks, d):
    return collections.Counter(t[1] for tokens, _ in chunks if tokens for t in tokens if t[0] == 'M' and t[2] == d)


@pytest.mark.parametrize('d', [2, 120, 128, 300])
def test_periodic_data_over_whole_chunks(enc, K, d):
    period = (1 + np.random.default_rng(d).permutation(255)[:min(d, 255)]).astype(np.uint8)    # distinct, none the type byte's 0
    if d > 255:
        period = np.concatenate([period, period[:d - 255][::-1] ^ 0x80])
    s = np.tile(period, 2 * K // d + 1)[:2 * K]
    chunks = _check_tokens(enc, _image(s, K), 0, (d,), K)
    assert len(chunks) == 2
    for tokens, data in chunks:
        # the chunk's first byte is the type byte, so eq_d holds on [d + 1, K): one overlapping interval, longer than its distance --
        # and a chunk starts with literals, since there is nothing to copy from
        assert all(t[0] == 'L' for t in tokens[:d + 1])
        m = _matches([(tokens, data)], d)
        assert m[258] == (K - d - 1) // 258 and sum(n * c for n, c in m.items()) >= K - d - 1 - 2


def test_intervals_of_every_length(enc, K):
    d = 300
    s = _background(K, 21)
    p = 1000
    for n in (2, 3, 4, 257, 258, 259, 260, 516, 517, 518):
        _repeat(s, p, p + n, d)
        p += n + 2 * d
    assert p < K
    chunks = _check_tokens(enc, _image(s, K), 0, (d,), K)
    # 2: literals; 3, 4, 257, 258: one match; 259 and 260: 258 and literals; 516: two of 258; 517 and 518: two of 258 and literals
    assert _matches(chunks[:1], d) == collections.Counter({3: 1, 4: 1, 257: 1, 258: 1 + 1 + 1 + 2 + 2 + 2})


def test_an_interval_across_a_chunk_boundary(enc, K):
    d = 200
    s = _background(K, 22)
    _repeat(s, K - 3000, K + 3000, d)
    chunks = _check_tokens(enc, _image(s, K), 0, (d,), K)
    first, second = chunks[0][0], chunks[1][0]
    assert first[-2:] == [('M', 258, d), ('M', 3000 % 258, d)]
    assert all(t[0] == 'L' for t in second[:d]) and ('M', 258, d) in second[d:d + 4]       # the second chunk cannot reach back into the first


def test_runs_inside_intervals_and_the_reverse(enc, K):
    d = 300
    s = _background(K, 23)
    s[1099], s[1140] = 8, 8
    s[1100:1140] = 9                                                                       # a run of 40 inside a tile that is repeated three times
    _repeat(s, 1300, 2200, d)
    s[4999], s[6000] = 5, 5
    s[5000:6000] = 4                                                                       # a run of 1000; eq_d holds on its last 700 positions only
    chunks = _check_tokens(enc, _image(s, K), 0, (d,), K)
    one, far = _matches(chunks[:1], 1), _matches(chunks[:1], d)
    assert far[258] == 3 and far[900 - 3 * 258] == 1                                       # the copies of the run go with d ...
    assert one[39] == 1 and one[258] == 3 + 38 and one[999 - 3 * 258] == 1                 # ... and the long run stays with distance 1


def test_the_tie_goes_to_distance_1(enc, K):
    d, q = 50, 4000
    s = _background(K, 24)
    for i in range(q - 10, q + 20):                                                        # no interval of either distance around
        while s[i] == s[i - 1] or s[i] == s[i - d]:
            s[i] = (int(s[i]) + 1) & 255
    s[q - 1:q + 10] = 33                                                                   # eq_1 on [q, q + 9]
    for i in (q - 2, q + 10):
        if s[i] == 33:
            s[i] = 34
    s[q - 5 - d:q + 5 - d] = s[q - 5:q + 5]                                                # eq_d on [q - 5, q + 4], 10 long as well
    if s[q + 5 - d] == 33:
        s[q + 5 - d] = 34
    tokens = _check_tokens(enc, _image(s, K), 0, (d,), K)[0][0]
    k = tokens.index(('M', 5, d))
    assert tokens[k + 1] == ('M', 10, 1)


def test_two_distances_interleave(enc, K):
    s = _background(K, 25)
    for i in range(3020, 3400):
        s[i] = s[i - 20]                                                                   # period 20: eq_100 from 3100, eq_260 from 3260
    _repeat(s, 3400, 3900, 260)                                                            # eq_260 goes on: [3260, 3900) outgrows [3100, 3500)
    p = 6000
    for n in range(12):                                                                    # intervals of the two distances in turn
        d = (100, 260)[n % 2]
        s[p:p + 50] = s[p - d:p - d + 50]
        p += 50
    for D in ((100, 260), (260, 100)):
        chunks = _check_tokens(enc, _image(s, K), 0, D, K)
        assert sum(_matches(chunks[:1], 100).values()) >= 4 and sum(_matches(chunks[:1], 260).values()) >= 4


# ---- 4. no change where nothing was asked -----------------------------------------------------------------------------------------------------
def _abi(handle, fn, x: torch.Tensor, filt: int, dist=None, ndist=None):
    lib = handle.lib
    N, H, W, C = x.shape
    bound, need = int(lib.ch_png_zlib_bound(H, W, C)), int(lib.ch_png_encode_workspace_bytes(N, H, W, C))
    out = torch.zeros(N * bound, dtype=torch.uint8, device='cuda')
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    sizes = torch.zeros(N, dtype=torch.int64, device='cuda')
    if fn == 'ch_png_encode':
        rc = lib.ch_png_encode(handle._h, x.data_ptr(), N, H, W, C, filt, out.data_ptr(), sizes.data_ptr(), ws.data_ptr(), need, None)
    else:
        arr = (ctypes.c_int * max(len(dist), 1))(*dist)
        rc = lib.ch_png_encode_dist(handle._h, x.data_ptr(), N, H, W, C, filt, arr, len(dist) if ndist is None else ndist, out.data_ptr(),
                                    sizes.data_ptr(), ws.data_ptr(), need, None)
    assert rc == 0, lib.ch_last_error(handle._h).decode()
    torch.cuda.synchronize()
    return [bytes(out[n * bound:n * bound + int(sizes[n])].cpu().numpy()) for n in range(N)]


@pytest.fixture(scope='module')
def batch():
    rng = np.random.default_rng(4)
    H, W = 80, 172
    return np.stack([_sheet('sheet4'), np.pad(_sheet('sheet0'), ((0, 0), (0, 12), (0, 0))), np.zeros((H, W, 3), np.uint8),
                     rng.integers(0, 256, (H, W, 3), dtype=np.uint8), (rng.integers(0, 5, (H, W, 3)) * 60).astype(np.uint8)])


def test_no_distances_is_ch_png_encode(handle, enc, batch):
    x = torch.from_numpy(batch).cuda()
    for filt in (-1, 0):
        old = _abi(handle, 'ch_png_encode', x, filt)
        assert _abi(handle, 'ch_png_encode_dist', x, filt, dist=()) == old
        assert _abi(handle, 'ch_png_encode_dist', x, filt, dist=(132,), ndist=0) == old    # the array is not read
        assert enc.streams(x, filt) == old and enc.streams(x, filt, distances=()) == old and enc.streams(x, filt, distances=[]) == old
        assert _abi(handle, 'ch_png_encode_dist', x, filt, dist=(132,)) != old


def test_batches_and_repeats_give_the_same_bytes(handle, enc, batch):
    assert batch.shape[1] * (1 + 3 * batch.shape[2]) > enc.chunk                           # more than one chunk per image
    for D in ((132,), (3, 132, 128)):
        together = _check(enc, batch, -1, D)
        assert _check(enc, batch, -1, D) == together
        assert _abi(handle, 'ch_png_encode_dist', torch.from_numpy(batch).cuda(), -1, dist=D) == together
        for n in range(5):
            assert _check(enc, batch[n:n + 1], -1, D)[0] == together[n], n
        assert len(set(together)) == 5


# ---- 5. argument errors ----------------------------------------------------------------------------------------------------------------------
def test_argument_errors_name_the_function(handle):
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    p = buf.data_ptr()
    lib = handle.lib
    need = int(lib.ch_png_encode_workspace_bytes(1, 4, 4, 3))
    assert 0 < need <= buf.numel()

    def call(dist, ndist, **change):
        a = dict(dict(img=p, N=1, H=4, W=4, C=3, filter=-1, out=p, sizes=p, ws=p, ws_bytes=need), **change)
        arr = None if dist is None else (ctypes.c_int * max(len(dist), 1))(*dist)
        rc = lib.ch_png_encode_dist(handle._h, a['img'], a['N'], a['H'], a['W'], a['C'], a['filter'], arr, ndist, a['out'], a['sizes'], a['ws'],
                                    a['ws_bytes'], None)
        return rc, lib.ch_last_error(handle._h).decode()

    for dist, ndist in (((2, 3, 4, 5), 4), ((2,), -1), (None, 1), (None, 3), ((0,), 1), ((1,), 1), ((32768,), 1), ((-7,), 1), ((5, 1), 2),
                        ((5, 5), 2), ((6, 7, 6), 3), ((7, 6, 6), 3)):
        rc, msg = call(dist, ndist)
        assert rc == ERR_ARG and 'ch_png_encode_dist' in msg, (dist, ndist, rc, msg)
    for change in (dict(img=None), dict(C=2), dict(filter=5), dict(N=0), dict(H=0), dict(W=40000), dict(ws_bytes=need - 1)):
        rc, msg = call((5,), 1, **change)
        assert rc == ERR_ARG and 'ch_png_encode_dist' in msg, (change, rc, msg)
    torch.cuda.synchronize()
    assert not bool(buf.any())                                                            # nothing was launched
    with pytest.raises(ValueError):
        PE.PngEncoder(handle, 'cuda:0').streams(buf[:48].reshape(1, 4, 4, 3), distances=(1,))


# ---- 6. sizes ------------------------------------------------------------------------------------------------------------------------------
def test_sizes(enc, K):
    ratios = {}
    for name, args, filt in (('sheet 2x4 cells of 40, margin 0', (2, 3, 40, 0), -1), ('sheet 2x4 cells of 40, margin 4', (2, 3, 40, 4), -1),
                             ('sheet 3x7 cells of 64, margin 0', (3, 6, 64, 0), -1), ('sheet 2x4 cells of 40, margin 0, filter 0', (2, 3, 40, 0), 0)):
        img = DO.sheet(*args)
        d = (args[2] + args[3]) * 3
        x = torch.from_numpy(img[None]).cuda()
        stream = _want(img, filt)
        plain, stride = len(enc.streams(x, filt)[0]), len(enc.streams(x, filt, distances=(d,))[0])
        z6, z1, rle = DO.zlib_chunked(stream, K, 6), DO.zlib_chunked(stream, K, 1), PO.rle_yardstick(stream, K)
        ratios[name] = stride / z6
        print(f'png-dist {name}: filtered {len(stream)} device() {plain} device({d},) {stride} chunked zlib-6 {z6} zlib-1 {z1} Z_RLE {rle} '
              f'stride/() {stride / plain:.4f} stride/zlib-6 {stride / z6:.4f}')
        if filt < 0:
            assert stride <= 0.6 * plain, (name, stride, plain)
    lab = PO.label_map()
    x = torch.from_numpy(lab[None]).cuda()
    print(f'png-dist label map 256x256: device() {len(enc.streams(x)[0])} device(257,) {len(enc.streams(x, distances=(257,))[0])}')
    for name, r in ratios.items():
        assert r <= MARGIN, (name, r)


# ---- 7. the job ------------------------------------------------------------------------------------------------------------------------------
def _weights():
    from ctrlhair_amd.hair_editor import procedural_weights
    w = procedural_weights(0, 64)
    w['sean'] = P.sean_state_dict(0, NGF)
    return w


def _decoded(folder):
    from PIL import Image
    return {n: np.asarray(Image.open(os.path.join(folder, n))) for n in sorted(os.listdir(folder))}


def test_find_directions_with_the_stride_writes_the_same_pixels(hip_lib, tmp_path):
    from ctrlhair_amd.pipeline import EditPipeline
    pipe = EditPipeline(_weights(), device=0, img_size=256, max_batch=4)
    try:
        search = DS.DirectionSearch(pipe, torch.from_numpy(P.synthetic_images(1, 256, seed=3)).cuda(), noise_seed=5)
        kw = dict(n=2, values=[-2.5, 2.5], seed=2)
        host, dev, strd = (str(tmp_path / n) for n in ('host', 'dev', 'stride'))
        a = DS.find_directions(search, 'shape', [], host, png='host', **kw)
        b = DS.find_directions(search, 'shape', [], dev, png='device', **kw)
        c = DS.find_directions(search, 'shape', [], strd, png='device', png_stride=True, **kw)
        assert a == b == c
        with pytest.raises(ValueError):
            DS.find_directions(search, 'shape', [], host, png='host', png_stride=True, **kw)
        ha, st = _decoded(os.path.join(host, 'shape_1')), _decoded(os.path.join(strd, 'shape_1'))
        assert sorted(ha) == sorted(st) == ['0.png', '1.png']
        for n in ha:
            assert ha[n].shape == (2 * 256, 3 * 256, 3) and np.array_equal(ha[n], st[n]), n
            plain, stride = (os.path.getsize(os.path.join(f, 'shape_1', n)) for f in (dev, strd))
            print(f'png-dist find_directions sheet {n}: device {plain} bytes, with the stride {stride} bytes')
            assert stride <= plain, (n, stride, plain)
    finally:
        pipe.close()
