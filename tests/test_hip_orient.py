"""EXIF orientation on the HIP library (ch_orient_u8; ctrlhair_amd/orient.py): every byte of a ragged batch against the numpy oracle,
batch invariance, the ABI's refusals, and the crop and uncrop jobs with orient / landmark_frame / metadata on the host and on the device
paths.  Equality throughout: the kernel permutes bytes."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

from ctrlhair_amd import dataset as D
from ctrlhair_amd import lib as L
from ctrlhair_amd import orient as O

pytestmark = pytest.mark.gpu
ERR_ARG = 1
DEV = 'cuda:0'
# one pixel, one row, one column, tile edges on both axes, several tiles on both axes (the tile is 64 x 64 pixels)
SIZES = [(1, 1), (1, 7), (7, 1), (63, 65), (64, 64), (65, 127), (129, 130), (300, 500)]


def _c(a):
    """A C-ordered copy (np.ascontiguousarray keeps the negative strides of a flipped view whose sides are 1)."""
    return np.array(a, order='C', copy=True)


@pytest.fixture(scope='module')
def handle(hip_lib):
    return L.Handle(0)


@pytest.fixture(scope='module')
def orienter(handle):
    return O.Orienter(handle, DEV)


@pytest.fixture(scope='module')
def ragged():
    """(stored numpy images, orientations, upright numpy images): 8 sizes x C in {1, 3} x 8 orientations, plus C = 4 and [H,W] inputs."""
    rng = np.random.default_rng(7)
    images, orients = [], []
    for H, W in SIZES:
        for C in (1, 3):
            for o in range(1, 9):
                images.append(rng.integers(0, 256, (H, W, C), dtype=np.uint8))
                orients.append(o)
    for o, (H, W) in zip(range(2, 9), SIZES[1:]):
        images.append(rng.integers(0, 256, (H, W, 4), dtype=np.uint8))
        orients.append(o)
        images.append(rng.integers(0, 256, (H, W), dtype=np.uint8))
        orients.append(o)
    return images, orients, [_c(O.orient_numpy(a, o)) for a, o in zip(images, orients)]


def _views(images, lead):
    """The images as contiguous views of ONE device buffer, packed behind `lead` bytes: odd, unaligned source addresses."""
    flat = np.concatenate([np.zeros(lead, np.uint8)] + [a.ravel() for a in images])
    buf = torch.from_numpy(flat).to(DEV)
    out, cur = [], lead
    for a in images:
        out.append(buf[cur:cur + a.size].view(a.shape))
        cur += a.size
    return out


@pytest.mark.parametrize('lead,align', [(0, 256), (1, 1), (13, 1)])
def test_ragged_batch_equals_the_oracle(orienter, ragged, lead, align):
    images, orients, want = ragged
    src = _views(images, lead)
    got = orienter.apply(src, orients, align=align)
    torch.cuda.synchronize()
    assert len(got) == len(images)
    bad = []
    for n, (g, w, s, o) in enumerate(zip(got, want, src, orients)):
        if o == 1:
            assert g is s
            continue
        assert g.dtype == torch.uint8 and tuple(g.shape) == w.shape and g.is_contiguous() and g.data_ptr() % min(align, 256) == 0
        if not torch.equal(g.cpu(), torch.from_numpy(w)):
            bad.append((n, images[n].shape, o))
    assert not bad, bad[:10]
    for s, a in zip(src, images):                                     # the sources are read only
        assert torch.equal(s.cpu(), torch.from_numpy(a))


def test_image_n_of_a_batch_is_its_own_call(orienter, ragged):
    images, orients, want = ragged
    src = _views(images, 5)
    got = orienter.apply(src, orients, align=1)
    for n in range(len(images)):
        alone = orienter.apply([src[n]], [orients[n]], align=1)[0]
        assert torch.equal(alone, got[n]), (images[n].shape, orients[n])
    torch.cuda.synchronize()


def test_values_that_leave_the_image_alone(orienter):
    t = torch.arange(7 * 5 * 3, dtype=torch.uint8, device=DEV).view(7, 5, 3)
    for o in (1, 0, 9, -6, None, 6.0, True):
        assert orienter.apply([t], [o])[0] is t
    assert orienter.apply([], []) == []
    mixed = orienter.apply([t, t, t], [1, 6, 9])
    assert mixed[0] is t and mixed[2] is t and torch.equal(mixed[1].cpu(), torch.from_numpy(_c(O.orient_numpy(t.cpu().numpy(), 6))))
    for bad in ([t.cpu()], [t.float()], [t[None, None]], [t[:, :, :2]], [t.cpu().numpy()]):
        with pytest.raises(ValueError, match='Orienter.apply'):
            orienter.apply(bad, [6])
    with pytest.raises(ValueError, match='orientations'):
        orienter.apply([t], [6, 6])
    # a non-contiguous input is its contiguous copy
    wide = torch.arange(7 * 10 * 3, dtype=torch.uint8, device=DEV).view(7, 10, 3)[:, ::2]
    assert torch.equal(orienter.apply([wide], [8])[0].cpu(), torch.from_numpy(_c(O.orient_numpy(wide.cpu().numpy(), 8))))


def test_abi_refusals(handle):
    lib = handle.lib
    img = torch.full((8, 6, 3), 9, dtype=torch.uint8, device=DEV)
    dst = torch.full((4096,), 77, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    good, _, total = O.pack_batch([img.data_ptr()], [(8, 6, 3)], [6])
    good = _c(good)
    assert total == 144
    err = lambda: lib.ch_last_error(handle._h).decode()

    def call(blob=good, nbytes=None, N=1, dst_p=dst.data_ptr(), dst_bytes=total, ws_p=ws.data_ptr(), ws_bytes=ws.numel()):
        b = None if blob is None else blob.ctypes.data_as(ctypes.c_void_p)
        rc = lib.ch_orient_u8(handle._h, b, (0 if blob is None else blob.nbytes) if nbytes is None else nbytes, N, dst_p, dst_bytes, ws_p,
                              ws_bytes, None)
        return rc, err()

    def edited(**fields):
        b = good.copy()
        d = b.view(O.DESC)
        for k, v in fields.items():
            d[k][0] = v
        return b

    need = int(lib.ch_orient_workspace_bytes(good.ctypes.data_as(ctypes.c_void_p), good.nbytes, 1, total))
    assert need == 256
    assert lib.ch_orient_u8(None, good.ctypes.data_as(ctypes.c_void_p), good.nbytes, 1, dst.data_ptr(), total, ws.data_ptr(), ws.numel(), None) == ERR_ARG
    for change, word in ((dict(blob=None), 'null pointer'), (dict(dst_p=None), 'null pointer'), (dict(ws_p=None), 'null pointer'),
                         (dict(N=0), 'N outside'), (dict(N=65536), 'N outside'), (dict(N=2), 'not N descriptors long'),
                         (dict(nbytes=16), 'not N descriptors long'), (dict(ws_p=ws.data_ptr() + 16), '256-byte aligned'),
                         (dict(ws_bytes=need - 1), 'ch_orient_workspace_bytes'), (dict(dst_bytes=total - 1), 'image 0: destination offset or extent'),
                         (dict(blob=edited(H=0)), 'image 0: side outside'), (dict(blob=edited(W=32769)), 'image 0: side outside'),
                         (dict(blob=edited(C=2)), 'image 0: C is not 1, 3 or 4'), (dict(blob=edited(orient=0)), 'image 0: orientation outside'),
                         (dict(blob=edited(orient=9)), 'image 0: orientation outside'), (dict(blob=edited(src=0)), 'image 0: null address'),
                         (dict(blob=edited(dst=1)), 'image 0: destination offset or extent'), (dict(blob=edited(dst=-1)), 'image 0: destination offset or extent'),
                         (dict(blob=edited(H=9)), 'image 0: destination offset or extent'),
                         (dict(blob=edited(src=dst.data_ptr() + 100)), 'image 0: source lies inside the destination')):
        rc, msg = call(**change)
        assert rc == ERR_ARG and msg.startswith('ch_orient_u8: ') and word in msg, (change.keys(), msg)
    torch.cuda.synchronize()
    assert bool((dst == 77).all())                                  # nothing ran
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.equal(dst[:total].view(6, 8, 3).cpu(), torch.full((6, 8, 3), 9, dtype=torch.uint8)) and bool((dst[total:] == 77).all())


# ---- the jobs --------------------------------------------------------------------------------------------------------------------------
ICC = np.random.default_rng(5).integers(0, 256, 70000, dtype=np.uint8).tobytes()      # two APP2 segments


def _tagged(a, fmt, o):
    from PIL import Image
    exif = Image.Exif()
    if o is not None:
        exif[0x0112] = o
    exif[0x010F] = 'a camera maker'
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, fmt, exif=exif, icc_profile=ICC)
    return buf.getvalue()


@pytest.fixture(scope='module')
def photos(tmp_path_factory):
    """One upright 160 x 200 photo, per extension as nine files that display identically: u.<ext> untagged, o<k>.<ext> the inversely
    turned pixels plus tag k.  Landmarks for the upright photo, and for the stored pixels of each file; an edited crop per name."""
    from PIL import Image
    from tests import unalign_cases as UC
    c = UC.inputs('a_magnify')
    root = tmp_path_factory.mktemp('orient_photos')
    up, lm = c['photo'], np.asarray(c['lm'], np.float64)
    out = {'up': up, 'lm': lm, 'root': root}
    for ext, fmt in (('png', 'PNG'), ('jpg', 'JPEG')):
        plain, tagged, edits = root / f'plain_{ext}', root / f'tagged_{ext}', root / f'edits_{ext}'
        plain.mkdir(), tagged.mkdir(), edits.mkdir()
        (plain / f'u.{ext}').write_bytes(_tagged(up, fmt, None))
        lms_up, lms_stored = {f'u.{ext}': lm}, {}
        for o in range(1, 9):
            stored = _c(O.orient_numpy(up, O.inverse_orientation(o)))
            n = f'o{o}.{ext}'
            (tagged / n).write_bytes(_tagged(stored, fmt, o))
            lms_up[n] = lm
            lms_stored[n] = O.unorient_points(lm, o, *stored.shape[:2])
        for n in lms_up:
            Image.fromarray(c['edits'][0]).save(edits / n)
        out[ext] = {'plain': str(plain), 'tagged': str(tagged), 'edits': str(edits), 'lms_up': lms_up, 'lms_stored': lms_stored,
                    'names': [f'o{o}.{ext}' for o in range(1, 9)]}
    return out


@pytest.fixture(scope='module')
def aligner(handle):
    from ctrlhair_amd.alignment import FaceAligner
    return FaceAligner(handle, torch.device('cuda', 0))


def _tag_left(name):
    """The orientation tag of an output made upright from o<k>.<ext>: none where the photo was turned; Orientation = 1 turns nothing and
    stays, as after ImageOps.exif_transpose."""
    return 1 if name[1] == '1' else None


def _files(folder):
    out = {}
    for n in sorted(os.listdir(folder)):
        with open(os.path.join(folder, n), 'rb') as f:
            out[n] = f.read()
    return out


def test_crop_job_orients_png_photos(aligner, photos, tmp_path):
    p = photos['png']
    folder = lambda name: str(tmp_path / name)
    D.crop_faces(aligner, p['plain'], folder('want'), 'ds', p['lms_up'], size=32)
    want = _files(folder('want'))['u.png']
    stats = {}
    for mode in ('host', 'device'):
        D.crop_faces(aligner, p['tagged'], folder(f'up_{mode}'), 'ds', p['lms_up'], size=32, decode=mode, orient=True, stats=stats)
        assert stats['fallbacks'] == 0
        D.crop_faces(aligner, p['tagged'], folder(f'st_{mode}'), 'ds', p['lms_stored'], size=32, decode=mode, orient=True, landmark_frame='stored')
        got_up, got_st = _files(folder(f'up_{mode}')), _files(folder(f'st_{mode}'))
        assert sorted(got_up) == sorted(got_st) == p['names']
        for n in p['names']:
            assert got_up[n] == want, (mode, n)
            assert got_st[n] == want, (mode, n, 'stored')
    # without the option nothing changes: the stored pixels are cropped, which is another picture for every turn but 1
    D.crop_faces(aligner, p['tagged'], folder('plain'), 'ds', p['lms_up'], size=32, decode='device')
    plain = _files(folder('plain'))
    assert plain['o1.png'] == want and all(plain[n] != want for n in p['names'][1:])


def test_crop_job_orients_jpeg_photos_device_equals_host(aligner, photos, tmp_path):
    from PIL import Image
    p = photos['jpg']
    folder = lambda name: str(tmp_path / name)
    stats = {}
    for mode in ('host', 'device'):
        D.crop_faces(aligner, p['tagged'], folder(mode), 'ds', p['lms_up'], size=32, decode=mode, jpeg=mode, orient=True, metadata='keep',
                     stats=stats)
        assert stats['fallbacks'] == 0
    host, dev = _files(folder('host')), _files(folder('device'))
    assert sorted(host) == sorted(dev) == p['names']
    for n in p['names']:
        assert host[n] == dev[n], n
        im = Image.open(io.BytesIO(dev[n]))
        assert im.size == (32, 32) and im.info['icc_profile'] == ICC and im.getexif().get(0x0112) == _tag_left(n) and im.getexif()[0x010F] == 'a camera maker'


def test_uncrop_job_orients(aligner, photos, tmp_path):
    from PIL import Image
    p = photos['png']
    folder = lambda name: str(tmp_path / name)
    D.uncrop_faces(aligner, p['plain'], p['edits'], folder('want'), 'ds', p['lms_up'])
    want = _files(folder('want'))['u.png']
    assert Image.open(io.BytesIO(want)).size == (200, 160)
    for mode in ('host', 'device'):
        D.uncrop_faces(aligner, p['tagged'], p['edits'], folder(f'up_{mode}'), 'ds', p['lms_up'], decode=mode, orient=True)
        D.uncrop_faces(aligner, p['tagged'], p['edits'], folder(f'st_{mode}'), 'ds', p['lms_stored'], decode=mode, orient=True,
                       landmark_frame='stored')
        got_up, got_st = _files(folder(f'up_{mode}')), _files(folder(f'st_{mode}'))
        for n in p['names']:
            assert got_up[n] == want, (mode, n)
            assert got_st[n] == want, (mode, n, 'stored')


def test_uncrop_job_keeps_metadata(aligner, photos, tmp_path):
    from PIL import Image
    folder = lambda name: str(tmp_path / name)
    # .jpg names: the device writer's files are the host writer's
    p = photos['jpg']
    for mode in ('host', 'device'):
        D.uncrop_faces(aligner, p['tagged'], p['edits'], folder(f'jpg_{mode}'), 'ds', p['lms_up'], decode=mode, jpeg=mode, orient=True,
                       metadata='keep')
    host, dev = _files(folder('jpg_host')), _files(folder('jpg_device'))
    assert sorted(host) == sorted(dev) == p['names']
    for n in p['names']:
        assert host[n] == dev[n], n
        im = Image.open(io.BytesIO(dev[n]))
        assert im.size == (200, 160) and im.info['icc_profile'] == ICC and im.getexif().get(0x0112) == _tag_left(n) and im.getexif()[0x010F] == 'a camera maker'
        assert dev[n][:4] == b'\xff\xd8\xff\xe0' and dev[n][20:22] == b'\xff\xe1' and dev[n].count(b'ICC_PROFILE\x00') == 2
    D.uncrop_faces(aligner, p['tagged'], p['edits'], folder('jpg_drop'), 'ds', p['lms_up'], decode='device', jpeg='device', orient=True)
    for n, data in _files(folder('jpg_drop')).items():
        im = Image.open(io.BytesIO(data))
        assert 'icc_profile' not in im.info and len(im.getexif()) == 0
        assert np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(dev[n]))))
    # .png names: other file bytes, the same pixels and the same metadata in Pillow's eyes
    p = photos['png']
    for mode in ('host', 'device'):
        D.uncrop_faces(aligner, p['tagged'], p['edits'], folder(f'png_{mode}'), 'ds', p['lms_up'], decode=mode, png=mode, orient=True,
                       metadata='keep')
    host, dev = _files(folder('png_host')), _files(folder('png_device'))
    assert sorted(host) == sorted(dev) == p['names']
    for n in p['names']:
        a, b = Image.open(io.BytesIO(host[n])), Image.open(io.BytesIO(dev[n]))
        assert np.array_equal(np.asarray(a), np.asarray(b)) and a.size == (200, 160)
        assert a.info['icc_profile'] == b.info['icc_profile'] == ICC
        assert a.getexif().tobytes() == b.getexif().tobytes() and a.info['exif'] == b.info['exif']
        assert b.getexif().get(0x0112) == _tag_left(n) and b.getexif()[0x010F] == 'a camera maker'


def test_read_photo_on_the_device(aligner, photos):
    from ctrlhair_amd.alignment import read_photo
    reader = D._PhotoReader(aligner)
    for ext in ('png', 'jpg'):
        p = photos[ext]
        for n in p['names']:
            path = os.path.join(p['tagged'], n)
            host, meta_h = read_photo(path)
            dev, meta_d = read_photo(path, reader=reader)
            assert meta_h == meta_d and meta_d[0] == int(n[1]) and meta_d[2] == ICC
            assert torch.equal(dev.cpu(), torch.from_numpy(_c(host))), n
            assert torch.equal(reader.read_rgb(path).cpu(), torch.from_numpy(D.read_rgb(path)))          # the default: as stored
    turned = D._PhotoReader(aligner, orient=True)
    paths = [os.path.join(photos['png']['tagged'], n) for n in photos['png']['names']]
    for t in turned.read_rgb_many(paths):
        assert torch.equal(t.cpu(), torch.from_numpy(photos['up']))
    assert reader.fallbacks == turned.fallbacks == 0
