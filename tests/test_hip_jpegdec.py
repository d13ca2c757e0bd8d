"""The JPEG decoder on the HIP library (ch_jpeg_decode; ctrlhair_amd/jpegdec.py): every corpus file against Pillow, the hand-over between
chunks at several `rounds`, batch invariance, the malformed set, the ABI's refusals, the crop and paste-back jobs with decode='device',
and the round trip through the project's own encoder.

The malformed streams reach the device only through the code tests/test_jpegdec.py has run over them on the CPU under sanitizers."""
import ctypes
import io
import os
import warnings

import numpy as np
import pytest
import torch

from ctrlhair_amd import jpegdec, jpegenc
from ctrlhair_amd import lib as L
from tests import jpegdec_cases as JC

pytestmark = pytest.mark.gpu
ERR_ARG = 1


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


@pytest.fixture(scope='module')
def dec(handle):
    return jpegdec.JpegDecoder(handle, 'cuda:0')


def _pillow(jpg: bytes) -> np.ndarray:
    """Pillow's pixels ([H,W] for grey files, [H,W,3] else), with its truncated-file tolerance off."""
    from PIL import Image, ImageFile
    assert not ImageFile.LOAD_TRUNCATED_IMAGES
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        im = Image.open(io.BytesIO(jpg))
        return np.asarray(im.convert('L' if im.mode == 'L' else 'RGB'))


def test_corpus(dec):
    corpus = JC.corpus()
    tensors, statuses = dec.decode([c.jpg for c in corpus])
    for c, t, s in zip(corpus, tensors, statuses):
        assert s == 0, (c.name, s)
        assert tuple(t.shape) == ((c.H, c.W) if c.C == 1 else (c.H, c.W, 3)), c.name
        assert np.array_equal(t.cpu().numpy(), _pillow(c.jpg)), c.name


def test_synchronisation_at_every_rounds(dec):
    """Three streams of three or more chunks.  Whatever `rounds`: OK and Pillow's pixels, or NOT_SYNCED; at the default all are OK."""
    streams = JC.sync_streams()
    want = [_pillow(c.jpg) for c in streams]
    seen = {}
    for rounds in (0, 1, 2, 3):
        tensors, statuses = dec.decode([c.jpg for c in streams], rounds=rounds)
        seen[rounds] = statuses
        for c, t, s, w in zip(streams, tensors, statuses, want):
            assert s in (0, jpegdec.NOT_SYNCED), (c.name, rounds, s)
            if s == 0:
                assert np.array_equal(t.cpu().numpy(), w), (c.name, rounds)
    assert seen[0] == [0, 0, 0], seen
    assert seen[1] == [jpegdec.NOT_SYNCED] * 3, seen                           # one launch hands nothing from chunk to chunk


def test_batch_invariance(dec):
    px = [JC.content(k, 48, 80, 3, 300 + i) for i, k in enumerate(('noise', 'smooth', 'flat', 'noise', 'checker'))]
    blobs = [JC.save(p, quality=q, subsampling=2, optimize=o) for p, q, o in zip(px, (95, 75, 50, 20, 100), (False, True, False, True, False))]
    parsed = [jpegdec.parse_jpeg(b) for b in blobs]
    assert {p[:4] for p in parsed} == {(48, 80, 3, 2)} and min(len(p[5]) for p in parsed) * 20 < max(len(p[5]) for p in parsed)
    streams, tables = [p[5] for p in parsed], [p[4] for p in parsed]
    img, status = dec.decode_streams(streams, tables, 48, 80, 3, 2)
    first = img.clone()
    assert status.cpu().tolist() == [0] * 5
    for n in range(5):
        assert np.array_equal(first[n].cpu().numpy(), _pillow(blobs[n])), n
    again, status = dec.decode_streams(streams, tables, 48, 80, 3, 2)
    assert torch.equal(again, first) and status.cpu().tolist() == [0] * 5
    for n in range(5):
        one, st = dec.decode_streams([streams[n]], [tables[n]], 48, 80, 3, 2)
        assert int(st[0]) == 0 and torch.equal(one[0], first[n]), n
    rev, _ = dec.decode_streams(streams[::-1], tables[::-1], 48, 80, 3, 2)
    assert torch.equal(rev.flip(0), first)


def test_malformed_set(handle, dec, tmp_path):
    """Every status is non-zero, or the pixels are Pillow's; where Pillow raises the status is non-zero.  The readers give what
    dataset.read_rgb gives: the same array or the same exception type."""
    from ctrlhair_amd import dataset as D
    bad = JC.malformed() + [('hostile-checker', JC.hostile('checker', 2)), ('hostile-noise', JC.hostile('noise', 'grey'))]
    host, parsed = {}, []
    for name, jpg in bad:
        try:
            host[name] = _pillow(jpg)
        except Exception as e:
            host[name] = e
        try:
            jpegdec.parse_jpeg(jpg)
            parsed.append((name, jpg))
        except jpegdec.Unsupported:
            pass
    tensors, statuses = dec.decode([j for _, j in parsed])
    nonzero = 0
    for (name, jpg), t, s in zip(parsed, tensors, statuses):
        nonzero += s != 0
        if isinstance(host[name], Exception):
            assert s != 0, name
        elif s == 0:
            assert np.array_equal(t.cpu().numpy(), host[name]), name
    by_name = {n: s for (n, _), s in zip(parsed, statuses)}
    assert by_name['unused-code'] == 1 and by_name['empty-scan'] == 3 and by_name['hostile-checker'] == 8 and by_name['hostile-noise'] == 8
    assert nonzero >= 40
    paths = []
    for k, (name, jpg) in enumerate(bad):
        paths.append(str(tmp_path / f'{k:03d}_{name}.jpg'))
        with open(paths[-1], 'wb') as f:
            f.write(jpg)
    reader = jpegdec.JpegDecoder(handle, 'cuda:0')
    readable = [p for p, (name, _) in zip(paths, bad) if not isinstance(host[name], Exception)]
    for p, t in zip(readable, reader.read_rgb(readable)):
        assert t.dtype == torch.uint8 and t.is_cuda and t.is_contiguous() and np.array_equal(t.cpu().numpy(), D.read_rgb(p)), p
    assert reader.fallbacks == sum(by_name.get(name, 1) != 0 for name, _ in bad if not isinstance(host[name], Exception))
    for p, (name, _) in zip(paths, bad):
        if isinstance(host[name], Exception):
            with pytest.raises(type(host[name])):
                reader.read_rgb([readable[0], p])


def test_abi_refusals(handle):
    lib = handle.lib
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda:0')
    offs = torch.zeros(4, dtype=torch.int64, device='cuda:0')
    st = torch.full((4,), -1, dtype=torch.int32, device='cuda:0')
    p, big = buf.data_ptr(), ctypes.c_size_t(1 << 40)

    def call(N=1, H=8, W=8, C=3, sampling=2, rounds=0, ws_bytes=big, ws=p):
        rc = lib.ch_jpeg_decode(handle._h, p, offs.data_ptr(), p, N, H, W, C, sampling, rounds, p, st.data_ptr(), ws, ws_bytes, None)
        return rc, lib.ch_last_error(handle._h).decode()

    for change, word in ((dict(N=0), 'N outside'), (dict(N=65536), 'N outside'), (dict(H=0), 'too small or too large'),
                         (dict(W=32769), 'too small or too large'), (dict(H=32768, W=32769), 'too small or too large'),
                         (dict(C=2), 'C must be'), (dict(C=4), 'C must be'), (dict(sampling=3), 'sampling'), (dict(sampling=-1), 'sampling'),
                         (dict(C=1, sampling=2), 'sampling'), (dict(rounds=65), 'rounds'), (dict(rounds=-1), 'rounds'),
                         (dict(ws=p + 8), '16-byte aligned')):
        rc, msg = call(**change)
        assert rc == ERR_ARG and msg.startswith('ch_jpeg_decode: ') and word in msg, (change, rc, msg)
    assert lib.ch_jpeg_decode(None, p, offs.data_ptr(), p, 1, 8, 8, 3, 2, 0, p, st.data_ptr(), p, big, None) == ERR_ARG        # a null handle
    assert call(ws_bytes=0)[0] == ERR_ARG and 'null pointer' in call(ws=None)[1]
    need = int(lib.ch_jpeg_decode_workspace_bytes(2, 8, 8, 3, 2))
    assert need >= 2 * 6 * 128
    rc, msg = call(N=2, ws_bytes=need - 1)
    assert rc == ERR_ARG and 'workspace' in msg and 'ch_jpeg_decode_workspace_bytes' in msg, msg
    for args in ((0, 8, 8, 3, 2), (65536, 8, 8, 3, 2), (1, 0, 8, 3, 2), (1, 8, 32769, 3, 2), (1, 32768, 32769, 1, 0), (1, 8, 8, 2, 0),
                 (1, 8, 8, 4, 0), (1, 8, 8, 3, 3), (1, 8, 8, 1, 1)):
        assert int(lib.ch_jpeg_decode_workspace_bytes(*args)) == 0, args
    assert int(lib.ch_jpeg_decode_workspace_bytes(1, 32768, 32768, 3, 0)) > 0
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [-1] * 4 and not bool(buf.any())               # nothing ran


# ---- the jobs --------------------------------------------------------------------------------------------------------------------------
def _files(folder):
    out = {}
    for n in sorted(os.listdir(folder)):
        with open(os.path.join(folder, n), 'rb') as f:
            out[n] = f.read()
    return out


def test_crop_and_uncrop_jobs_decode_device(handle, tmp_path):
    from PIL import Image
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd.alignment import FaceAligner
    from tests import unalign_cases as UC
    c = UC.inputs('a_magnify')
    photos = tmp_path / 'photos'
    photos.mkdir()
    names = ['p0.jpg', 'p1.jpeg', 'p2.png', 'p3.jpg', 'p4.jpg', 'p5.jpg']
    photo = c['photo']
    Image.fromarray(photo).save(photos / names[0])
    Image.fromarray(np.ascontiguousarray(photo[:-3, :-5])).save(photos / names[1], quality=90, subsampling=0, optimize=True)     # odd sides
    Image.fromarray(photo).save(photos / names[2])
    Image.fromarray(photo).save(photos / names[3], progressive=True)
    Image.fromarray(np.ascontiguousarray(photo[:-1])).save(photos / names[4], subsampling=1)
    Image.fromarray(np.ascontiguousarray(photo[:, :, 1])).save(photos / names[5])                                                # a grey file
    lms = {n: c['lm'] for n in names}
    aligner = FaceAligner(handle, torch.device('cuda', 0))
    folder = lambda name: str(tmp_path / name)
    stats = {}
    for mode in ('host', 'device'):
        done, skipped = D.crop_faces(aligner, str(photos), folder(f'crop_{mode}'), 'ds', lms, size=64, decode=mode, stats=stats)
        assert done == names and skipped == []
        assert stats['fallbacks'] == (1 if mode == 'device' else 0)            # the progressive file
    host, dev = _files(folder('crop_host')), _files(folder('crop_device'))
    assert sorted(host) == sorted(dev) == names
    for n in names:
        assert host[n] == dev[n], n
    for mode in ('host', 'device'):
        done, skipped = D.uncrop_faces(aligner, str(photos), folder('crop_host'), folder(f'uncrop_{mode}'), 'ds', lms, decode=mode,
                                       stats=stats)
        assert done == names and skipped == []
        assert stats['fallbacks'] == (1 if mode == 'device' else 0)            # the progressive photo; its crop is a baseline file
    host, dev = _files(folder('uncrop_host')), _files(folder('uncrop_device'))
    assert sorted(host) == sorted(dev) == names
    for n in names:
        assert host[n] == dev[n], n
    for job in (D.crop_faces, D.uncrop_faces):
        with pytest.raises(ValueError):
            job(*((aligner, str(photos), folder('x'), 'ds', lms) if job is D.crop_faces else
                  (aligner, str(photos), folder('crop_host'), folder('x'), 'ds', lms)), decode='gpu')


def test_encoder_round_trip(handle, dec):
    enc = jpegenc.JpegEncoder(handle, 'cuda:0')
    for H, W, C in ((37, 29, 3), (64, 48, 3), (17, 33, 1)):
        x = torch.from_numpy(np.stack([JC.content(k, H, W, C, 40 + i) for i, k in enumerate(('noise', 'smooth', 'checker'))])).cuda()
        for quality, sub in ((75, 2), (95, 0), (10, 2)):
            files = enc.encode(x, quality, sub)
            tensors, statuses = dec.decode(files)
            assert statuses == [0] * 3, (H, W, C, quality, sub, statuses)
            for f, t in zip(files, tensors):
                assert np.array_equal(t.cpu().numpy(), _pillow(f)), (H, W, C, quality, sub)
