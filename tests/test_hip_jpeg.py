"""The JPEG encoder on the GPU (csrc/jpeg_encode.hip, ctrlhair_amd/jpegenc.py): every scan equals the numpy oracle's
(tests/jpeg_oracle.py) and every file the recorded Pillow file (tests/golden/jpeg_golden.npz) byte for byte -- there is no tolerance --,
batches and repeats give the same bytes, the sizes stay under the derived bound, the ABI refuses bad arguments by name, and the crop and
paste-back jobs write with jpeg='device' the files they write with jpeg='host'."""
import os

import numpy as np
import pytest
import torch

from ctrlhair_amd import jpegenc as JE
from ctrlhair_amd import lib as L
from tests import jpeg_cases as JC
from tests import jpeg_oracle as JO

pytestmark = pytest.mark.gpu
ERR_ARG = 1
GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'jpeg_golden.npz')


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


@pytest.fixture(scope='module')
def enc(handle):
    return JE.JpegEncoder(handle, 'cuda:0')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k].tobytes() for k in z.files if k not in ('pillow', 'libjpeg')}


@pytest.fixture(scope='module')
def oracle_scans():
    """case id -> the oracle's scan, computed once."""
    return {JC.case_id(c): JO.scan(JC.case_image(c), c[3], JC.SUBSAMPLING[c[4]]) for c in JC.CASES}


def _first_difference(a: bytes, b: bytes):
    n = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return f'lengths {len(a)} / {len(b)}, first difference at byte {n}'


@pytest.mark.parametrize('case', JC.CASES, ids=JC.case_id)
def test_scan_equals_the_oracle_and_file_equals_pillows(enc, handle, golden, oracle_scans, case):
    H, W, _, q, mode = case
    ss = JC.SUBSAMPLING[mode]
    img = JC.case_image(case)
    x = torch.from_numpy(img[None]).cuda()
    scan = enc.scans(x, q, ss)[0]
    want = oracle_scans[JC.case_id(case)]
    assert scan == want, _first_difference(scan, want)
    assert len(scan) <= int(handle.lib.ch_jpeg_scan_bound(H, W, 1 if mode == 'grey' else 3, ss))
    assert enc.encode(x, q, ss)[0] == golden[JC.case_id(case)]


def test_batches_and_repeats_give_the_same_bytes(enc):
    H, W = 50, 77                                                             # odd: dummy blocks, unaligned rows, images at odd addresses
    batch = np.stack([JC.image(H, W, content, '420', seed=1) for content in JC.CONTENTS])
    x = torch.from_numpy(batch).cuda()
    for q, ss in ((75, 2), (100, 0), (25, 2)):
        together = enc.scans(x, q, ss)
        assert together == enc.scans(x, q, ss)
        assert len(set(together)) == len(JC.CONTENTS)
        for n in range(len(batch)):
            assert enc.scans(x[n:n + 1], q, ss)[0] == together[n] == JO.scan(batch[n], q, ss), (q, ss, n)
    grey = torch.from_numpy(np.stack([JC.image(H, W, content, 'grey', seed=2) for content in JC.CONTENTS])).cuda()
    together = enc.scans(grey, 90)
    for n in range(len(grey)):
        assert enc.scans(grey[n:n + 1], 90)[0] == together[n] == enc.scans(grey[n:n + 1, :, :, None], 90, 0)[0]     # subsampling: ignored for grey


def test_sizes_stay_under_the_bound(enc, handle):
    lib = handle.lib
    # the bound is derived: blocks * 1658 bits, doubled by stuffing, + 2
    assert int(lib.ch_jpeg_scan_bound(8, 8, 1, 0)) == 2 * ((1658 + 7) // 8) + 2
    assert int(lib.ch_jpeg_scan_bound(17, 23, 3, 2)) == 2 * ((2 * 2 * 6 * 1658 + 7) // 8) + 2            # dummy blocks included
    assert int(lib.ch_jpeg_scan_bound(17, 23, 3, 0)) == 2 * ((3 * 3 * 3 * 1658 + 7) // 8) + 2
    for content in ('noise', 'checker', 'cos77'):                              # the largest scans there are: quality 100
        for mode in JC.MODES:
            img = JC.image(40, 56, content, mode, seed=3)
            n = len(enc.scans(torch.from_numpy(img[None]).cuda(), 100, JC.SUBSAMPLING[mode])[0])
            assert 0 < n <= int(lib.ch_jpeg_scan_bound(40, 56, 1 if mode == 'grey' else 3, JC.SUBSAMPLING[mode])), (content, mode, n)


def test_write_and_wrapper_errors(enc, tmp_path):
    imgs = np.stack([JC.image(24, 40, c, '420', seed=4) for c in ('noise', 'smooth')])
    paths = [str(tmp_path / f'{i}.jpg') for i in range(2)]
    enc.write(paths, torch.from_numpy(imgs).cuda(), quality=90, subsampling=0)
    for p, im in zip(paths, imgs):
        with open(p, 'rb') as f:
            assert f.read() == JO.file(im, 90, 0)
    with pytest.raises(ValueError):
        enc.write(paths[:1], torch.from_numpy(imgs).cuda())
    for bad in (torch.zeros(1, 4, 4, 4, dtype=torch.uint8), torch.zeros(1, 4, 4, 2, dtype=torch.uint8), torch.zeros(1, 4, 4, 3),
                torch.zeros(4, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            enc.scans(bad.cuda())
    ok = torch.zeros(1, 4, 4, 3, dtype=torch.uint8).cuda()
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling=1), dict(subsampling='422')):
        with pytest.raises(ValueError):
            enc.scans(ok, **kw)
    assert enc.scans(ok[:0]) == []


def test_argument_errors_name_the_function(handle):
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    p = buf.data_ptr()
    lib = handle.lib
    need = int(lib.ch_jpeg_encode_workspace_bytes(1, 4, 4, 3, 2))
    assert 0 < need <= buf.numel()
    good = dict(img=p, N=1, H=4, W=4, C=3, q=75, ss=2, out=p, sizes=p, ws=p, ws_bytes=need)
    for change in (dict(img=None), dict(out=None), dict(sizes=None), dict(ws=None), dict(C=4), dict(C=2), dict(C=0), dict(q=0), dict(q=101),
                   dict(ss=1), dict(ss=-1), dict(ss=3), dict(N=0), dict(N=-1), dict(N=65536), dict(H=0), dict(W=0), dict(H=32769), dict(W=40000),
                   dict(H=32768, W=32768, C=1), dict(H=32768, W=32769, C=1), dict(ws=p + 4), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        a = dict(good, **change)
        rc = lib.ch_jpeg_encode(handle._h, a['img'], a['N'], a['H'], a['W'], a['C'], a['q'], a['ss'], a['out'], a['sizes'], a['ws'],
                                a['ws_bytes'], None)
        msg = lib.ch_last_error(handle._h).decode()
        assert rc == ERR_ARG and 'ch_jpeg_encode' in msg, (change, rc, msg)
        if change == dict(H=32768, W=32768, C=1):                             # H * W = 2^30 is allowed: here the workspace is what is small
            assert 'workspace' in msg
    for args in ((4, 4, 4, 2), (4, 4, 2, 0), (4, 4, 3, 1), (0, 4, 3, 2), (4, 0, 3, 2), (32769, 4, 3, 2), (32768, 32769, 1, 0)):
        assert int(lib.ch_jpeg_scan_bound(*args)) == 0, args
        assert int(lib.ch_jpeg_encode_workspace_bytes(1, *args)) == 0, args
    assert int(lib.ch_jpeg_encode_workspace_bytes(0, 4, 4, 3, 2)) == 0 and int(lib.ch_jpeg_encode_workspace_bytes(65536, 4, 4, 3, 2)) == 0
    assert int(lib.ch_jpeg_scan_bound(32768, 32768, 3, 0)) > 0 and int(lib.ch_jpeg_encode_workspace_bytes(1, 32768, 32768, 3, 0)) > 0
    assert int(lib.ch_abi_version()) == 1
    torch.cuda.synchronize()
    assert not bool(buf.any())                                                # nothing was launched


# ---- the jobs --------------------------------------------------------------------------------------------------------------------------
def _files(folder):
    out = {}
    for n in sorted(os.listdir(folder)):
        with open(os.path.join(folder, n), 'rb') as f:
            out[n] = f.read()
    return out


def test_crop_and_uncrop_jobs_write_the_host_files(handle, tmp_path):
    from PIL import Image
    from ctrlhair_amd import dataset as D
    from ctrlhair_amd.alignment import FaceAligner
    from tests import unalign_cases as UC
    c = UC.inputs('a_magnify')
    photos = tmp_path / 'photos'
    photos.mkdir()
    names = ['p0.jpg', 'p1.jpeg']
    Image.fromarray(c['photo']).save(photos / names[0])
    Image.fromarray(np.ascontiguousarray(c['photo'][:-3, :-5])).save(photos / names[1])           # odd sides
    lms = {n: c['lm'] for n in names}
    aligner = FaceAligner(handle, torch.device('cuda', 0))
    folder = lambda name: str(tmp_path / name)
    for kw, tag in ((dict(), ''), (dict(jpeg_quality=90, jpeg_subsampling='444'), '_q90')):
        for mode in ('host', 'device'):
            done, skipped = D.crop_faces(aligner, str(photos), folder(f'crop_{mode}{tag}'), 'ds', lms, size=64, jpeg=mode, **kw)
            assert done == names and skipped == []
        host, dev = _files(folder(f'crop_host{tag}')), _files(folder(f'crop_device{tag}'))
        assert sorted(host) == sorted(dev) == names
        for n in names:
            assert host[n] == dev[n], (tag, n)
        for mode in ('host', 'device'):
            done, skipped = D.uncrop_faces(aligner, str(photos), folder(f'crop_host{tag}'), folder(f'uncrop_{mode}{tag}'), 'ds', lms, jpeg=mode,
                                           **kw)
            assert done == names and skipped == []
        host, dev = _files(folder(f'uncrop_host{tag}')), _files(folder(f'uncrop_device{tag}'))
        assert sorted(host) == sorted(dev) == names
        for n in names:
            assert host[n] == dev[n], (tag, n)
            assert Image.open(os.path.join(folder(f'uncrop_device{tag}'), n)).size == Image.open(photos / n).size
    assert _files(folder('crop_host'))['p0.jpg'] != _files(folder('crop_host_q90'))['p0.jpg']
