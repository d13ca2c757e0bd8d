"""The PNG decoder on the HIP library (ch_png_decode; ctrlhair_amd/pngdec.py): every corpus file against Pillow and the unfilter oracle,
batch invariance, the malformed set between valid neighbours and guard bytes, the ABI's refusals, the file readers with their Pillow
fallback, the colour-statistics job with decode='device', and the round trip through the project's own encoder.

The status classes of the malformed set are those of tests/png_decode_cases.py, which tests/test_pngdec.py shows to be what the inflate core
gives on the CPU under sanitizers: the streams reach the device only through the code that run has covered."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from ctrlhair_amd import lib as L
from ctrlhair_amd import pngdec, pngenc
from tests import png_decode_cases as PC
from tests import png_unfilter_oracle as UO

pytestmark = pytest.mark.gpu
ERR_ARG = 1
GUARD = 4096


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


@pytest.fixture(scope='module')
def dec(handle):
    return pngdec.PngDecoder(handle, 'cuda:0')


def _pillow(png: bytes) -> np.ndarray:
    from PIL import Image
    im = Image.open(io.BytesIO(png))
    im.load()
    return np.asarray(im)


def test_corpus(dec):
    corpus = PC.corpus()
    tensors, statuses = dec.decode([c.png for c in corpus])
    for c, t, s in zip(corpus, tensors, statuses):
        assert s == 0, (c.name, s)
        got = t.cpu().numpy()
        assert np.array_equal(got, _pillow(c.png)), c.name
        assert np.array_equal(got.reshape(c.H, c.W, c.C), UO.unfilter(c.filtered, c.H, c.W, c.C)), c.name


def _mixed_streams():
    """16 zlib streams of 64 x 64 x 3 images, from some 60 bytes to over 12 KiB."""
    from tests import png_oracle as PO
    rng = np.random.default_rng(5)
    streams, pixels = [], []
    for k in range(16):
        if k % 4 == 0:
            px = np.full((64, 64, 3), 17 * k, np.uint8)
        elif k % 4 == 1:
            px = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
        else:
            px = PC.pixels_for(64, 64, 3, 500 + k)
        filtered, _ = PO.filtered_stream(px, (k % 6) - 1)
        streams.append(PC.VARIANTS[2 if k % 4 == 0 else k % len(PC.VARIANTS)][1](filtered))        # (the flat images at level 9)
        pixels.append(px)
    return streams, pixels


def test_batch_invariance(dec):
    streams, pixels = _mixed_streams()
    assert min(map(len, streams)) * 50 < max(map(len, streams))
    img, status = dec.decode_streams(streams, 64, 64, 3)
    first = img.clone()
    assert status.cpu().tolist() == [0] * 16
    for n in range(16):
        assert np.array_equal(first[n].cpu().numpy(), pixels[n]), n
    again, status = dec.decode_streams(streams, 64, 64, 3)
    assert torch.equal(again, first) and status.cpu().tolist() == [0] * 16
    for n in range(16):
        one, st = dec.decode_streams([streams[n]], 64, 64, 3)
        assert int(st[0]) == 0 and torch.equal(one[0], first[n]), n
    rev, _ = dec.decode_streams(streams[::-1], 64, 64, 3)
    assert torch.equal(rev.flip(0), first)


def test_malformed_between_valid_neighbours_and_guards(handle):
    (H, W, C, px, z), entries = PC.malformed()
    streams, want = [], []
    for name, s, st, _ in entries:
        streams += [z, s]
        want += [0, st]
    streams.append(z)
    want.append(0)
    N = len(streams)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    data = np.frombuffer(b''.join(streams), np.uint8)
    ws_bytes = int(handle.lib.ch_png_decode_workspace_bytes(N, H, W, C))
    assert ws_bytes >= N * H * (1 + W * C)
    pad16 = lambda v: v + (-v) % 16
    img_at = GUARD
    img_bytes = N * H * W * C
    str_at = pad16(img_at + img_bytes + GUARD)
    ws_at = pad16(str_at + data.size + GUARD)
    total = ws_at + ws_bytes + GUARD
    buf = torch.full((total,), 0xA5, dtype=torch.uint8, device='cuda:0')
    buf[str_at:str_at + data.size] = torch.from_numpy(data.copy()).cuda()
    offsets = torch.from_numpy(offs).cuda()
    status = torch.full((N,), -1, dtype=torch.int32, device='cuda:0')
    base = buf.data_ptr()
    assert (base + ws_at) % 16 == 0
    handle.call('ch_png_decode', base + str_at, offsets.data_ptr(), N, H, W, C, base + img_at, status.data_ptr(), base + ws_at, ws_bytes,
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = status.cpu().tolist()
    names = ['valid' if k % 2 == 0 else entries[k // 2][0] for k in range(N)]
    assert got == want, [(n, g, w) for n, g, w in zip(names, got, want) if g != w]
    host = buf.cpu().numpy()
    img = host[img_at:img_at + img_bytes].reshape(N, H, W, C)
    for k in range(0, N, 2):
        assert np.array_equal(img[k], px), k
    for a, b, what in ((0, img_at, 'before img'), (img_at + img_bytes, str_at, 'after img'), (str_at + data.size, ws_at, 'after streams / before workspace'),
                       (ws_at + ws_bytes, total, 'after workspace')):
        assert (host[a:b] == 0xA5).all(), what
    assert np.array_equal(host[str_at:str_at + data.size], data)


def test_abi_refusals(handle):
    lib = handle.lib
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda:0')
    offs = torch.zeros(4, dtype=torch.int64, device='cuda:0')
    st = torch.zeros(4, dtype=torch.int32, device='cuda:0')
    p, big = buf.data_ptr(), ctypes.c_size_t(1 << 40)

    def call(N, H, W, C, ws_bytes=big):
        return lib.ch_png_decode(handle._h, p, offs.data_ptr(), N, H, W, C, p, st.data_ptr(), p, ws_bytes, None)

    assert call(0, 8, 8, 3) == ERR_ARG
    assert call(1, 8, 8, 2) == ERR_ARG
    assert call(1, 32769, 32768, 1) == ERR_ARG
    assert call(1, 0, 8, 3) == ERR_ARG and call(65536, 8, 8, 3) == ERR_ARG
    need = int(lib.ch_png_decode_workspace_bytes(2, 8, 8, 3))
    assert need >= 2 * 8 * 25 and call(2, 8, 8, 3, need - 1) == ERR_ARG
    assert lib.ch_png_decode_workspace_bytes(0, 8, 8, 3) == 0 and lib.ch_png_decode_workspace_bytes(1, 8, 8, 2) == 0
    assert lib.ch_png_decode_workspace_bytes(1, 32768, 32768, 4) == 32768 * (1 + 4 * 32768)
    torch.cuda.synchronize()
    assert int(st.sum()) == 0                                                              # nothing ran


def test_readers_and_fallback(handle, tmp_path):
    from PIL import Image
    from ctrlhair_amd import dataset as D
    rgb, grey, rgba = PC.pixels_for(40, 33, 3, 1), PC.pixels_for(40, 33, 1, 2)[:, :, 0], PC.pixels_for(21, 50, 4, 3)
    Image.fromarray(rgb).save(tmp_path / 'a_rgb.png')
    Image.fromarray(grey).save(tmp_path / 'b_grey.png')
    Image.fromarray(rgba).save(tmp_path / 'c_rgba.PNG')
    Image.fromarray(rgb).convert('P').save(tmp_path / 'd_palette.png')
    Image.fromarray(rgb).save(tmp_path / 'e_photo.jpg')
    # f: a file Pillow still reads although the device refuses its stream: the last three bytes of the Adler-32 are missing (INPUT_END)
    good = (tmp_path / 'a_rgb.png').read_bytes()
    H, W, C, stream = pngdec.parse_png(good)
    (tmp_path / 'f_adler.png').write_bytes(pngenc.wrap_png(stream[:-3], H, W, C))
    paths = [str(tmp_path / n) for n in sorted(os.listdir(tmp_path))]
    dec = pngdec.PngDecoder(handle, 'cuda:0')
    got = dec.read_rgb(paths)
    for p, t in zip(paths, got):
        want = D.read_rgb(p)
        assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and np.array_equal(t.cpu().numpy(), want), p
    assert dec.fallbacks == 3                                                              # palette, .jpg, the stream without its whole Adler-32
    dec.fallbacks = 0
    got = dec.read_gray(paths)
    for p, t in zip(paths, got):
        assert np.array_equal(t.cpu().numpy(), D.read_gray(p)), p
    assert dec.fallbacks == 5                                                              # all but the grey file
    # a corrupt PNG raises what the host path raises
    z = bytearray(stream)
    z[len(z) // 2:] = b''
    bad = str(tmp_path / 'g_cut.png')
    with open(bad, 'wb') as f:
        f.write(pngenc.wrap_png(bytes(z), H, W, C))
    with pytest.raises(Exception) as host_err:
        D.read_rgb(bad)
    with pytest.raises(type(host_err.value)):
        dec.read_rgb([paths[0], bad])


def test_hair_color_stats_decode_device(handle, tmp_path):
    from PIL import Image
    from ctrlhair_amd import colorstats as CS
    from ctrlhair_amd import dataset as D
    from tests import colorstats_ref as R
    img_dir, lab_dir = tmp_path / 'img', tmp_path / 'label'
    img_dir.mkdir()
    lab_dir.mkdir()
    rng = np.random.default_rng(11)
    for i, kind in enumerate(['blob', 'blob', 'all', 'blob', 'few', 'blob']):
        img, lab = R.synth_image_and_labels(rng, 64, 64, kind)
        Image.fromarray(img).save(img_dir / f'{i}.png')
        D.write_label_png(str(lab_dir / f'{i}.png'), lab)
    stats = CS.HairColorStats(handle, torch.device('cuda', 0))
    outs = {}
    for mode in ('host', 'device'):
        root = tmp_path / mode
        res = D.hair_color_stats(stats, str(img_dir), str(lab_dir), str(root), 'ds', jobs=('rgb', 'colorvar'), batch=4, decode=mode)
        assert len(res['rgb']) == 6 and len(res['colorvar']) >= 1
        outs[mode] = {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), 'rb').read()
                      for d, _, fs in os.walk(root) for f in fs}
    assert sorted(outs['host']) == sorted(outs['device']) and len(outs['host']) >= 7
    for k in outs['host']:
        assert outs['host'][k] == outs['device'][k], k
    with pytest.raises(ValueError):
        D.hair_color_stats(stats, str(img_dir), str(lab_dir), str(tmp_path / 'x'), 'ds', decode='gpu')


def test_encoder_round_trip(handle, dec):
    enc = pngenc.PngEncoder(handle, 'cuda:0')
    groups = {}
    for c in PC.corpus():
        groups.setdefault((c.H, c.W, c.C), []).append(c.pixels)
    for (H, W, C), px in groups.items():
        x = torch.from_numpy(np.stack(px)).cuda()
        for distances in ((), (W * C + 1, 3 * C)) if H * (1 + W * C) > 64 else ((),):
            distances = tuple(d for d in dict.fromkeys(distances) if 2 <= d <= 32767)
            tensors, statuses = dec.decode(enc.encode(x if C > 1 else x[:, :, :, 0], -1, distances))
            assert statuses == [0] * len(px), (H, W, C, distances, statuses)
            assert torch.equal(torch.stack(tensors).reshape(x.shape), x), (H, W, C, distances)
