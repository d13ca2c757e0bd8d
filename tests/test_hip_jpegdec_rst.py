"""Restart intervals in the JPEG decoder on the HIP library (ch_jpeg_decode_rst; ctrlhair_amd/jpegdec.py): every file of
tests/jpegdec_rst_cases.py against Pillow, at the default and at every `rounds` from 1 to 8, batch invariance over a batch that mixes
restart intervals, the malformed set beside valid neighbours, ch_jpeg_decode_rst with all-zero intervals against ch_jpeg_decode, the ABI's
refusals, and the crop and paste-back jobs over photos written with restart markers.

The malformed streams reach the device only through the code tests/test_jpegdec_rst.py has run over them on the CPU under sanitizers."""
import ctypes
import io
import os
import warnings

import numpy as np
import pytest
import torch

from ctrlhair_amd import jpegdec
from ctrlhair_amd import lib as L
from tests import jpegdec_cases as JC
from tests import jpegdec_rst_cases as RC

pytestmark = pytest.mark.gpu
ERR_ARG = 1
RESTART = 9


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


@pytest.fixture(scope='module')
def dec(handle):
    return jpegdec.JpegDecoder(handle, 'cuda:0')


_want = {}


def _pillow(jpg: bytes) -> np.ndarray:
    """Pillow's pixels ([H,W] for grey files, [H,W,3] else), decoded once per file."""
    if jpg not in _want:
        from PIL import Image, ImageFile
        assert not ImageFile.LOAD_TRUNCATED_IMAGES
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            im = Image.open(io.BytesIO(jpg))
            _want[jpg] = np.asarray(im.convert('L' if im.mode == 'L' else 'RGB'))
    return _want[jpg]


def test_corpus(dec):
    cases = RC.all_cases()
    assert sum(c.ri > 0 for c in cases) > 400
    tensors, statuses = dec.decode([c.jpg for c in cases])
    for c, t, s in zip(cases, tensors, statuses):
        assert s == 0, (c.name, s)
        assert tuple(t.shape) == ((c.H, c.W) if c.C == 1 else (c.H, c.W, 3)), c.name
        assert np.array_equal(t.cpu().numpy(), _pillow(c.jpg)), c.name


@pytest.mark.parametrize('rounds', range(1, 9))
def test_every_rounds(dec, rounds):
    """rounds = 1 .. 8: OK and Pillow's pixels, or NOT_SYNCED; every file is OK at 8, the default."""
    cases = RC.all_cases()
    tensors, statuses = dec.decode([c.jpg for c in cases], rounds=rounds)
    for c, t, s in zip(cases, tensors, statuses):
        assert s in (0, jpegdec.NOT_SYNCED), (c.name, rounds, s)
        if s == 0:
            assert np.array_equal(t.cpu().numpy(), _pillow(c.jpg)), (c.name, rounds)
    if rounds == 8:
        assert statuses == [0] * len(cases)


def test_batch_invariance(dec):
    mixed = RC.mixed_batch()
    H, W, C, sampling = RC.MIXED_SHAPE
    parsed = [jpegdec.parse_jpeg_restart(c.jpg) for c in mixed]
    streams, tables, restart = [p[5] for p in parsed], [p[4] for p in parsed], [p[6] for p in parsed]
    assert restart == [c.ri for c in mixed]
    img, status = dec.decode_streams(streams, tables, H, W, C, sampling, restart=restart)
    first = img.clone()
    assert status.cpu().tolist() == [0] * len(mixed)
    for n, c in enumerate(mixed):
        assert np.array_equal(first[n].cpu().numpy(), _pillow(c.jpg)), c.name
    again, status = dec.decode_streams(streams, tables, H, W, C, sampling, restart=restart)
    assert torch.equal(again, first) and status.cpu().tolist() == [0] * len(mixed)
    for n in range(len(mixed)):
        one, st = dec.decode_streams([streams[n]], [tables[n]], H, W, C, sampling, restart=[restart[n]])
        assert int(st[0]) == 0 and torch.equal(one[0], first[n]), n
    rev, _ = dec.decode_streams(streams[::-1], tables[::-1], H, W, C, sampling, restart=restart[::-1])
    assert torch.equal(rev.flip(0), first)
    # the files without an interval through the entry without one
    plain = [n for n, r in enumerate(restart) if r == 0]
    img0, st0 = dec.decode_streams([streams[n] for n in plain], [tables[n] for n in plain], H, W, C, sampling)
    assert st0.cpu().tolist() == [0] * len(plain) and torch.equal(img0, first[plain])


def test_malformed_set(dec):
    """Every malformed stream has a non-zero status, at the default and at 1 and 64 rounds; the valid streams around it are Pillow's."""
    H, W, C, sampling = RC.MIXED_SHAPE
    base = RC.malformed_base()
    good = [base] + RC.mixed_batch()
    gp = [jpegdec.parse_jpeg_restart(c.jpg) for c in good]
    bad = RC.malformed()
    streams, tables, restart, valid = [], [], [], {}
    for k, (name, scan, ri) in enumerate(bad):                                 # good, bad, good, bad, ..., good
        g = gp[k % len(gp)]
        valid[len(streams)] = good[k % len(gp)]
        streams += [g[5], scan]
        tables += [g[4], gp[0][4]]
        restart += [g[6], ri]
    valid[len(streams)] = good[-1]
    streams.append(gp[-1][5]), tables.append(gp[-1][4]), restart.append(gp[-1][6])
    seen = {}
    for rounds in (0, 1, 64):
        img, status = dec.decode_streams(streams, tables, H, W, C, sampling, rounds=rounds, restart=restart)
        status = status.cpu().tolist()
        for n, c in valid.items():
            assert status[n] == 0 and np.array_equal(img[n].cpu().numpy(), _pillow(c.jpg)), (rounds, n, c.name, status[n])
        seen[rounds] = {name: status[2 * k + 1] for k, (name, _, _) in enumerate(bad)}
        assert all(seen[rounds].values()), (rounds, seen[rounds])
    for name in ('markers-swapped', 'marker-number-changed', 'numbers-from-1', 'dri-1', 'dri-3', 'dri-4', 'marker-doubled',
                 'marker-doubled-next-number', 'marker-after-last-mcu'):
        assert seen[0][name] == RESTART, (name, seen[0][name])
    assert jpegdec.STATUS_NAMES[RESTART] == 'RESTART'


def test_all_zero_restart_is_ch_jpeg_decode(dec):
    """ch_jpeg_decode_rst with restart = 0 for every stream: the images and statuses of ch_jpeg_decode, on the corpus without intervals
    and on its malformed set."""
    groups = {}
    for c in JC.corpus() + JC.sync_streams():
        groups.setdefault((c.H, c.W, c.C, c.sampling), []).append(jpegdec.parse_jpeg(c.jpg))
    bad = []
    for name, jpg in JC.malformed():
        try:
            bad.append(jpegdec.parse_jpeg(jpg))
        except jpegdec.Unsupported:
            pass
    groups[('malformed',) + bad[0][:4]] = bad
    for key, items in groups.items():
        H, W, C, sampling = key[-4:]
        streams, tables = [p[5] for p in items], [p[4] for p in items]
        img, status = dec.decode_streams(streams, tables, H, W, C, sampling)
        img, status = img.clone(), status.clone()
        img0, status0 = dec.decode_streams(streams, tables, H, W, C, sampling, restart=[0] * len(items))
        assert torch.equal(status0, status), key
        ok = status == 0
        assert torch.equal(img0[ok], img[ok]), key
        if key[0] != 'malformed':
            assert bool(ok.all()), key


def test_abi_refusals(handle):
    lib = handle.lib
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda:0')
    offs = torch.zeros(4, dtype=torch.int64, device='cuda:0')
    st = torch.full((4,), -1, dtype=torch.int32, device='cuda:0')
    p, big = buf.data_ptr(), ctypes.c_size_t(1 << 40)

    def call(N=1, H=8, W=8, C=3, sampling=2, rounds=0, ws_bytes=big, ws=p, restart=p):
        rc = lib.ch_jpeg_decode_rst(handle._h, p, offs.data_ptr(), p, restart, N, H, W, C, sampling, rounds, p, st.data_ptr(), ws, ws_bytes, None)
        return rc, lib.ch_last_error(handle._h).decode()

    def sibling(N=1, H=8, W=8, C=3, sampling=2, rounds=0, ws_bytes=big, ws=p):
        rc = lib.ch_jpeg_decode(handle._h, p, offs.data_ptr(), p, N, H, W, C, sampling, rounds, p, st.data_ptr(), ws, ws_bytes, None)
        return rc, lib.ch_last_error(handle._h).decode()

    for change, word in ((dict(N=0), 'N outside'), (dict(N=65536), 'N outside'), (dict(H=0), 'too small or too large'),
                         (dict(W=32769), 'too small or too large'), (dict(H=32768, W=32769), 'too small or too large'),
                         (dict(C=2), 'C must be'), (dict(C=4), 'C must be'), (dict(sampling=3), 'sampling'), (dict(sampling=-1), 'sampling'),
                         (dict(C=1, sampling=2), 'sampling'), (dict(rounds=65), 'rounds'), (dict(rounds=-1), 'rounds'),
                         (dict(ws=p + 8), '16-byte aligned'), (dict(ws=None), 'null pointer'), (dict(ws_bytes=0), 'workspace')):
        rc, msg = call(**change)
        assert rc == ERR_ARG and msg.startswith('ch_jpeg_decode_rst: ') and word in msg, (change, rc, msg)
        rc0, msg0 = sibling(**change)                                          # the sibling entry: the same refusal in the same words
        assert rc0 == rc and msg0 == msg.replace('ch_jpeg_decode_rst: ', 'ch_jpeg_decode: ', 1), (change, msg, msg0)
    rc, msg = call(restart=None)
    assert rc == ERR_ARG and msg == 'ch_jpeg_decode_rst: null pointer'
    assert lib.ch_jpeg_decode_rst(None, p, offs.data_ptr(), p, p, 1, 8, 8, 3, 2, 0, p, st.data_ptr(), p, big, None) == ERR_ARG    # a null handle
    need = int(lib.ch_jpeg_decode_workspace_bytes(2, 8, 8, 3, 2))
    rc, msg = call(N=2, ws_bytes=need - 1)
    assert rc == ERR_ARG and 'workspace' in msg and 'ch_jpeg_decode_workspace_bytes' in msg, msg
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [-1] * 4 and not bool(buf.any())               # nothing ran


# ---- the jobs --------------------------------------------------------------------------------------------------------------------------
def _files(folder):
    out = {}
    for n in sorted(os.listdir(folder)):
        with open(os.path.join(folder, n), 'rb') as f:
            out[n] = f.read()
    return out


def test_crop_and_uncrop_jobs_over_restart_photos(handle, tmp_path):
    from PIL import Image
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd.alignment import FaceAligner
    from tests import unalign_cases as UC
    c = UC.inputs('a_magnify')
    photos = tmp_path / 'photos'
    photos.mkdir()
    names = ['p0.jpg', 'p1.jpeg', 'p2.jpg', 'p3.jpg', 'p4.jpg']
    photo = c['photo']
    Image.fromarray(photo).save(photos / names[0], restart_marker_rows=1)
    Image.fromarray(np.ascontiguousarray(photo[:-3, :-5])).save(photos / names[1], quality=90, subsampling=0, optimize=True, restart_marker_blocks=3)
    Image.fromarray(photo).save(photos / names[2], restart_marker_blocks=1)
    Image.fromarray(np.ascontiguousarray(photo[:-1])).save(photos / names[3], subsampling=1, restart_marker_rows=2)
    Image.fromarray(np.ascontiguousarray(photo[:, :, 1])).save(photos / names[4], restart_marker_blocks=5)                        # a grey file
    for n in names:
        with open(photos / n, 'rb') as f:
            data = f.read()
        assert jpegdec.parse_jpeg_restart(data)[6] > 0 and RC.markers(RC.scan_of(data)), n
    lms = {n: c['lm'] for n in names}
    aligner = FaceAligner(handle, torch.device('cuda', 0))
    folder = lambda name: str(tmp_path / name)
    stats = {}
    for mode in ('host', 'device'):
        done, skipped = D.crop_faces(aligner, str(photos), folder(f'crop_{mode}'), 'ds', lms, size=64, decode=mode, stats=stats)
        assert done == names and skipped == []
        assert stats['fallbacks'] == 0, mode
    host, dev = _files(folder('crop_host')), _files(folder('crop_device'))
    assert sorted(host) == sorted(dev) == names
    for n in names:
        assert host[n] == dev[n], n
    for mode in ('host', 'device'):
        done, skipped = D.uncrop_faces(aligner, str(photos), folder('crop_host'), folder(f'uncrop_{mode}'), 'ds', lms, decode=mode, stats=stats)
        assert done == names and skipped == []
        assert stats['fallbacks'] == 0, mode
    host, dev = _files(folder('uncrop_host')), _files(folder('uncrop_device'))
    assert sorted(host) == sorted(dev) == names
    for n in names:
        assert host[n] == dev[n], n
