"""The PNG encoder on the GPU (csrc/png_encode.hip, ctrlhair_amd/pngenc.py): every zlib stream inflates to the numpy oracle's filtered
bytes (tests/png_oracle.py) bit for bit, the wrapped file decodes to the pixels, batches and repeats give the same bytes, the ABI
refuses bad arguments, the jobs write the same pixels with png='device' as with png='host', and the stream is about as small as zlib's
run-length strategy over the same chunks makes it.

Measured ratios device / chunked RLE yardstick (deterministic; printed by test_compression_against_the_yardsticks):
label map 1.0025, small contact sheet 1.0000, ramp 1.0000 -> MARGIN = the largest rounded up to the next 0.05."""
import io
import os
import types
import zlib

import numpy as np
import pytest
import torch

from ctrlhair_amd import directions as DS
from ctrlhair_amd import lib as L
from ctrlhair_amd import pngenc as PE
from ctrlhair_amd import procedural as P
from tests import png_oracle as PO

pytestmark = pytest.mark.gpu
ERR_ARG = 1
NGF = 16
MODES = {1: 'L', 3: 'RGB', 4: 'RGBA'}
MARGIN = 1.05


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


@pytest.fixture(scope='module')
def enc(handle):
    return PE.PngEncoder(handle, 'cuda:0')


def _check(enc, imgs: np.ndarray, filt: int = -1):
    """Encode a batch [N,H,W,C] / [N,H,W]; check every stream against the oracle and every file against the pixels.  -> the streams."""
    from PIL import Image
    x = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()
    streams = enc.streams(x, filt)
    N, H, W = imgs.shape[:3]
    C = imgs.shape[3] if imgs.ndim == 4 else 1
    bound = int(enc.handle.lib.ch_png_zlib_bound(H, W, C))
    assert len(streams) == N
    for n, s in enumerate(streams):
        assert len(s) <= bound
        d = zlib.decompressobj()
        got = d.decompress(s)
        assert d.eof and d.unused_data == b'' and d.unconsumed_tail == b''
        want, _ = PO.filtered_stream(imgs[n], filt)
        assert got == want, (imgs.shape, filt, n)
        im = Image.open(io.BytesIO(PE.wrap_png(s, H, W, C)))
        im.load()
        assert im.mode == MODES[C] and np.array_equal(np.asarray(im).reshape(imgs[n].shape), imgs[n])
    return streams


def _shape_for(F: int):
    """(H, W, C) whose filtered stream has exactly F bytes: RGB rows where F factors that way, else grey rows (sides <= 32768)."""
    for rowlen in range(256, 4, -1):
        if F % rowlen == 0 and (rowlen - 1) % 3 == 0:
            return F // rowlen, (rowlen - 1) // 3, 3
    for rowlen in range(min(F, 32769), 1, -1):
        if F % rowlen == 0 and F // rowlen <= 32768:
            return F // rowlen, rowlen - 1, 1
    raise ValueError(f'no image has a filtered stream of {F} bytes')


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (3, 5), (17, 31), (64, 64), (70, 53)])
def test_shapes_and_filters(enc, shape, C):
    H, W = shape
    rng = np.random.default_rng(1000 * H + 10 * W + C)
    noise = rng.integers(0, 256, (1, H, W, C), dtype=np.uint8)
    steps = (rng.integers(0, 4, (1, H, W, C)) * 70).astype(np.uint8)                      # few values: runs and matches at every size
    for filt in (-1, 0, 1, 2, 3, 4):
        _check(enc, np.concatenate([noise, steps]), filt)
    if C == 1:
        _check(enc, noise[..., 0])                                                        # [N,H,W] is C = 1


def test_chunk_boundary_sizes(enc, handle):
    K = int(handle.lib.ch_png_chunk_bytes())
    assert K == enc.chunk and K % 256 == 0
    rng = np.random.default_rng(2)
    for F in (K, 2 * K, K + 1, 2 * K + 37, K - 1):
        H, W, C = _shape_for(F)
        assert H * (1 + W * C) == F
        img = (rng.integers(0, 3, H * W * C) * 100).astype(np.uint8)                       # runs in the first half, noise in the second
        img[img.size // 2:] = rng.integers(0, 256, img.size - img.size // 2, dtype=np.uint8)
        for filt in (-1, 0):
            _check(enc, img.reshape(1, H, W, C), filt)
    assert _shape_for(K)[2] == 3 and _shape_for(2 * K)[2] == 3                            # (128 and 256 rows of 85 RGB pixels at K = 32768)


def _small_sheet(handle):
    cells = PO.smooth_cells(2, 3, 48)
    sheet = DS.ContactSheet(handle, 'cuda:0', 2, 3, 48, margin=4)
    sheet.draw(torch.from_numpy(cells).cuda(), [(i, j) for i in range(2) for j in range(3)])
    return sheet


@pytest.fixture(scope='module')
def contents(handle):
    rng = np.random.default_rng(3)
    return {'zeros': np.zeros((128, 85, 3), np.uint8), 'ones': np.full((140, 85, 3), 255, np.uint8),
            'noise': rng.integers(0, 256, (97, 131, 3), dtype=np.uint8), 'ramp': PO.ramp(70, 300, 3), 'label': PO.label_map(),
            'sheet': _small_sheet(handle).numpy()}


@pytest.mark.parametrize('name', ['zeros', 'ones', 'noise', 'ramp', 'label', 'sheet'])
def test_contents(enc, contents, name):
    img = contents[name]
    K = enc.chunk
    for filt in (-1, 0):
        s = _check(enc, img[None], filt)[0]
        F = len(PO.filtered_stream(img, filt)[0])
        if name == 'noise':                                                               # nothing to gain: a stored block per chunk
            assert len(s) == 2 + F + 5 * ((F + K - 1) // K) + 6
        if name in ('zeros', 'ones'):                                                     # matches of 258 back to back: ~ 1 bit per 129 bytes
            assert len(s) < F // 64


def test_runs_of_every_kind(enc):
    K = enc.chunk
    W = K                                                                                 # rows of K + 1 stream bytes: the type byte, then W
    runs = []
    for k, n in enumerate((1, 2, 3, 4, 257, 258, 259, 260, 516, 517, 518, 775, 1000)):
        runs += [10 + k] * n + [200 + k]                                                  # runs separated by single distinct bytes
    head = np.array(runs, np.uint8)
    # filter 0: stream position p of row 0 holds image byte p - 1.  Row 0 ends in 100 9s, stream positions K - 99 .. K: that run
    # straddles the first chunk boundary; row 1 is [1, 2, 3] and then one run of 5s to the end of the second chunk and beyond
    row0 = np.concatenate([head, np.full(W - 100 - len(head), 7, np.uint8), np.full(100, 9, np.uint8)])
    row1 = np.concatenate([np.array([1, 2, 3], np.uint8), np.full(W - 3, 5, np.uint8)])
    s = _check(enc, np.stack([row0, row1])[None], 0)[0]
    assert len(s) < 500                                                                   # (3 chunks; ~50 bytes for a chunk that is one run)
    zeros = _check(enc, np.zeros((1, 3, W), np.uint8), 0)[0]                               # type bytes included: every chunk one run of zeros
    assert len(zeros) < 250
    # x[j] = j + 1 under the Sub filter: type byte 1, then x - a = 1 everywhere -- the whole stream one run of a non-zero byte, so the
    # second and third chunk are single runs that began in the chunk before and may not reach back into it
    ones = np.broadcast_to(((np.arange(W) + 1) % 256).astype(np.uint8), (1, 3, W))
    assert PO.filtered_stream(ones[0], 1)[0] == b'\x01' * (3 * (W + 1))
    s1 = _check(enc, ones, 1)[0]
    assert len(s1) < 250
    for w in (1, 2, 3, 4, 257, 258, 259, 260):                                            # the whole stream one run: type byte 0 + w zeros
        _check(enc, np.zeros((1, 1, w), np.uint8), 0)


def test_batches_and_repeats_give_the_same_bytes(enc, contents):
    rng = np.random.default_rng(4)
    H, W = 96, 152
    batch = np.stack([contents['sheet'][:H, :W], contents['noise'][:H, :131].repeat(2, axis=1)[:, :W], np.zeros((H, W, 3), np.uint8),
                      PO.ramp(H, W, 3), (rng.integers(0, 5, (H, W, 3)) * 60).astype(np.uint8)])
    assert batch.shape == (5, H, W, 3) and H * (1 + 3 * W) > enc.chunk                    # more than one chunk per image
    together = _check(enc, batch)
    again = _check(enc, batch)
    assert together == again
    for n in range(5):
        assert _check(enc, batch[n:n + 1])[0] == together[n], n
    assert len(set(together)) == 5
    files = enc.encode(torch.from_numpy(batch).cuda())
    assert [f[:8] for f in files] == [PE.PNG_SIGNATURE] * 5


def test_write_and_wrapper_errors(enc, tmp_path):
    from PIL import Image
    lab = np.stack([PO.label_map(64, seed=s) for s in range(3)])
    paths = [str(tmp_path / f'{i}.png') for i in range(3)]
    enc.write(paths, torch.from_numpy(lab).cuda())
    for p, want in zip(paths, lab):
        im = Image.open(p)
        assert im.mode == 'L' and np.array_equal(np.asarray(im), want)
    with pytest.raises(ValueError):
        enc.write(paths[:2], torch.from_numpy(lab).cuda())
    for bad in (torch.zeros(1, 4, 4, 2, dtype=torch.uint8), torch.zeros(1, 4, 4, 3), torch.zeros(4, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            enc.streams(bad.cuda())
    with pytest.raises(ValueError):
        enc.streams(torch.zeros(1, 4, 4, 3, dtype=torch.uint8).cuda(), filter=5)


def test_argument_errors_name_the_function(handle):
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    p = buf.data_ptr()
    lib = handle.lib
    need = int(lib.ch_png_encode_workspace_bytes(1, 4, 4, 3))
    assert 0 < need <= buf.numel() and int(lib.ch_png_zlib_bound(4, 4, 3)) == 2 + 52 + 10 + 2 + 4
    good = dict(img=p, N=1, H=4, W=4, C=3, filter=-1, out=p, sizes=p, ws=p, ws_bytes=need)
    for change in (dict(img=None), dict(out=None), dict(sizes=None), dict(ws=None), dict(C=2), dict(C=0), dict(C=5), dict(filter=-2),
                   dict(filter=5), dict(N=0), dict(N=-1), dict(H=0), dict(W=0), dict(H=32769), dict(W=40000), dict(H=32768, W=32768, C=1),
                   dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        a = dict(good, **change)
        rc = lib.ch_png_encode(handle._h, a['img'], a['N'], a['H'], a['W'], a['C'], a['filter'], a['out'], a['sizes'], a['ws'], a['ws_bytes'],
                               None)
        msg = lib.ch_last_error(handle._h).decode()
        if change == dict(H=32768, W=32768, C=1):                                         # H * W = 2^30 is allowed: here the workspace is what is small
            assert rc == ERR_ARG and 'workspace' in msg
        assert rc == ERR_ARG and 'ch_png_encode' in msg, (change, rc, msg)
    rc = lib.ch_png_encode(handle._h, p, 1, 32768, 32769, 1, -1, p, p, p, need, None)
    assert rc == ERR_ARG and 'ch_png_encode' in lib.ch_last_error(handle._h).decode()
    assert int(lib.ch_png_zlib_bound(4, 4, 2)) == 0 and int(lib.ch_png_encode_workspace_bytes(0, 4, 4, 3)) == 0
    torch.cuda.synchronize()
    assert not bool(buf.any())                                                            # nothing was launched


def test_compression_against_the_yardsticks(enc, contents):
    K = enc.chunk
    size, rle, huff = {}, {}, {}
    for name in ('zeros', 'label', 'sheet', 'ramp'):
        img = contents[name]
        stream = PO.filtered_stream(img)[0]
        size[name] = len(enc.streams(torch.from_numpy(img[None]).cuda())[0])
        rle[name], huff[name] = PO.rle_yardstick(stream, K), PO.huffman_only(stream)
        print(f'png {name}: filtered {len(stream)} device {size[name]} chunked-RLE {rle[name]} huffman-only {huff[name]} '
              f'device/RLE {size[name] / rle[name]:.4f}')
    for name in ('zeros', 'label'):                                                       # the run matching works
        assert size[name] < huff[name], name
    assert MARGIN < huff['label'] / rle['label']                                          # (the margin cannot swallow that condition)
    for name in ('label', 'sheet', 'ramp'):
        assert size[name] <= MARGIN * rle[name], (name, size[name], rle[name])


# ---- wiring ----------------------------------------------------------------------------------------------------------------------------
def _weights():
    from ctrlhair_amd.hair_editor import procedural_weights
    w = procedural_weights(0, 64)
    w['sean'] = P.sean_state_dict(0, NGF)
    return w


def _decoded(folder):
    from PIL import Image
    return {n: np.asarray(Image.open(os.path.join(folder, n))) for n in sorted(os.listdir(folder))}


def test_find_directions_device_writes_the_same_pixels(hip_lib, tmp_path):
    from ctrlhair_amd.pipeline import EditPipeline
    pipe = EditPipeline(_weights(), device=0, img_size=256, max_batch=4)
    try:
        search = DS.DirectionSearch(pipe, torch.from_numpy(P.synthetic_images(1, 256, seed=3)).cuda(), noise_seed=5)
        host, dev = str(tmp_path / 'host'), str(tmp_path / 'dev')
        a = DS.find_directions(search, 'shape', [], host, n=2, values=[-2.5, 2.5], seed=2, png='host')
        b = DS.find_directions(search, 'shape', [], dev, n=2, values=[-2.5, 2.5], seed=2, png='device')
        assert a == b
        ha, de = _decoded(os.path.join(host, 'shape_1')), _decoded(os.path.join(dev, 'shape_1'))
        assert sorted(ha) == sorted(de) == ['0.png', '1.png']
        for n in ha:
            assert ha[n].shape == (2 * 256, 3 * 256, 3) and np.array_equal(ha[n], de[n]), n
        assert not np.array_equal(ha['0.png'], ha['1.png'])
    finally:
        pipe.close()


def test_extract_masks_device_writes_the_same_pixels(handle, tmp_path):
    from PIL import Image
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd.models import FaceParsing
    fp = FaceParsing(handle, torch.device('cuda', 0)).load_state_dict(P.bisenet_state_dict(0), max_batch=2, max_size=512)
    editor = types.SimpleNamespace(face_parsing=fp)
    img_dir = tmp_path / 'images'
    img_dir.mkdir()
    imgs = ((P.synthetic_images(2, 256, seed=21).transpose(0, 2, 3, 1) * 0.5 + 0.5) * 255).astype(np.uint8)
    for i, im in enumerate(imgs):
        Image.fromarray(im).save(img_dir / f'{i:02d}.png')
    assert D.extract_masks(editor, str(img_dir), str(tmp_path / 'host'), batch=2) == ['00.png', '01.png']
    assert D.extract_masks(editor, str(img_dir), str(tmp_path / 'dev'), batch=2, png='device') == ['00.png', '01.png']
    ha, de = _decoded(str(tmp_path / 'host')), _decoded(str(tmp_path / 'dev'))
    assert sorted(ha) == sorted(de) == ['00.png', '01.png']
    for n in ha:
        assert ha[n].shape == (512, 512) and ha[n].dtype == np.uint8 and np.array_equal(ha[n], de[n]), n
        assert Image.open(os.path.join(str(tmp_path / 'dev'), n)).mode == 'L'
