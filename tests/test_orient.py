"""Host half of the EXIF orientation and metadata support, CPU only: the numpy oracle of ch_orient_u8 equals Pillow's exif_transpose, the
metadata reader returns what exif_transpose leaves behind, points move with their pixels, the writers' containers are Pillow's (JPEG byte
for byte, PNG up to what Pillow reads back), the host crop jobs take the options, and csrc/orient_batch.h refuses every batch that lies
(as a stand-alone program under AddressSanitizer and UndefinedBehaviorSanitizer)."""
import io
import os
import zlib

import numpy as np
import pytest

from ctrlhair_amd import jpegenc as JE
from ctrlhair_amd import orient as O
from ctrlhair_amd import photometa as PM
from ctrlhair_amd import pngenc as PE

from tests import jpeg_oracle as JO

SIZES = [(1, 1), (1, 7), (7, 1), (33, 65), (64, 64), (65, 63), (100, 131)]           # (H, W)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pixels(H, W, C, seed=0):
    return np.random.default_rng(seed + 1000 * H + W).integers(0, 256, (H, W, C) if C > 1 else (H, W), dtype=np.uint8)


def tagged_file(a, fmt, orientation=None, icc=None, extra=True):
    """A PNG (eXIf chunk) or JPEG (APP1) file of pixels a with the orientation tag (None: no tag; extra: one more tag, so the EXIF block
    survives without it)."""
    from PIL import Image
    exif = Image.Exif()
    if orientation is not None:
        exif[0x0112] = orientation
    if extra:
        exif[0x010F] = 'a camera maker'
    buf = io.BytesIO()
    kw = {'exif': exif} if len(exif) else {}
    if icc is not None:
        kw['icc_profile'] = icc
    Image.fromarray(a).save(buf, fmt, **kw)
    return buf.getvalue()


def profile(n, seed=5):
    """n bytes that stand for an ICC profile: the containers carry them without looking inside."""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.mark.parametrize('size', SIZES, ids=[f'{h}x{w}' for h, w in SIZES])
@pytest.mark.parametrize('fmt,C', [('PNG', 3), ('PNG', 1), ('JPEG', 3), ('JPEG', 1)])
def test_oracle_equals_exif_transpose(size, fmt, C):
    from PIL import Image, ImageOps
    a = pixels(*size, C)
    for o in range(1, 9):
        data = tagged_file(a, fmt, o)
        stored = np.asarray(Image.open(io.BytesIO(data)))
        if fmt == 'PNG':
            assert np.array_equal(stored, a)
        want = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(data))))
        got = O.orient_numpy(stored, o)
        assert got.shape == want.shape == O.upright_shape(*size, o) + ((3,) if C == 3 else ())
        assert np.array_equal(got, want), o
        assert PM.read_metadata(data)[0] == o


def test_missing_tag_zero_and_nine_leave_the_image_alone():
    from PIL import Image, ImageOps
    a = pixels(33, 65, 3)
    for o in (None, 0, 9, 1):
        data = tagged_file(a, 'PNG', o)
        want = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(data))))
        assert np.array_equal(want, a)
        got = PM.read_metadata(data)[0]
        assert got == (1 if o is None else o) and not O.turns(got)
        assert O.orient_numpy(a, got) is a
        assert O.upright_shape(33, 65, got) == (33, 65) and O.inverse_orientation(got) == 1
    for bad in (True, 2.0, '6', None):
        assert not O.turns(bad) and O.orient_numpy(a, bad) is a


def test_inverse_orientation_undoes_the_turn():
    a = pixels(7, 12, 3)
    for o in range(1, 9):
        up = O.orient_numpy(a, o)
        assert np.array_equal(O.orient_numpy(up, O.inverse_orientation(o)), a), o


@pytest.mark.parametrize('fmt', ['PNG', 'JPEG'])
def test_read_metadata_is_what_exif_transpose_leaves_behind(fmt):
    from PIL import Image, ImageOps
    a = pixels(33, 65, 3)
    icc = profile(3000)
    for o in range(2, 9):
        for extra in (True, False):
            data = tagged_file(a, fmt, o, icc=icc, extra=extra)
            im = Image.open(io.BytesIO(data))
            assert im.getexif().get(0x0112) == o and im.info.get('icc_profile') == icc
            up = ImageOps.exif_transpose(im)
            got = PM.read_metadata(data)
            assert got == (o, up.info['exif'], icc), (o, extra)
            back = Image.Exif()
            back.load(got[1])
            assert 0x0112 not in back and (back.get(0x010F) == 'a camera maker') == extra
            # for pixels that stay as stored the tag stays
            kept = Image.Exif()
            kept.load(PM.read_metadata(data, strip=False)[1])
            assert kept.get(0x0112) == o
    # 1, 0 and 9 turn nothing: exif_transpose leaves the file's block as it is, tag included, and so does read_metadata
    for o in (1, 0, 9):
        data = tagged_file(a, fmt, o, icc=icc)
        im = Image.open(io.BytesIO(data))
        up = ImageOps.exif_transpose(im)
        got = PM.read_metadata(data)
        assert got == (o, up.info['exif'], icc) and got[1] == im.info['exif'], o
        kept = Image.Exif()
        kept.load(got[1])
        assert kept.get(0x0112) == o
        assert PM.read_metadata(data, strip=False) == got
    # no EXIF at all: nothing to carry; no profile: None
    assert PM.read_metadata(tagged_file(a, fmt, None, extra=False)) == (1, None, None)
    assert PM.read_metadata(tagged_file(a, fmt, None, icc=icc, extra=False)) == (1, None, icc)


def test_read_metadata_takes_a_path(tmp_path):
    data = tagged_file(pixels(33, 65, 3), 'JPEG', 6, icc=profile(500))
    p = tmp_path / 'a.jpg'
    p.write_bytes(data)
    assert PM.read_metadata(str(p)) == PM.read_metadata(p) == PM.read_metadata(data) and PM.read_metadata(data)[0] == 6
    assert PM.read_metadata(str(tmp_path / 'missing.jpg')) == PM.NONE
    assert PM.turns(6) and not PM.turns(1) and not PM.turns(9) and not PM.turns(True) and not PM.turns(None)


def test_read_metadata_never_raises():
    a = pixels(33, 65, 3)
    for fmt in ('PNG', 'JPEG'):
        data = tagged_file(a, fmt, 6, icc=profile(500))
        for cut in (0, 1, 3, 8, 11):
            assert PM.read_metadata(data[:cut]) == PM.NONE, (fmt, cut)
    for junk in (b'', b'not an image at all', bytes(range(256)) * 8, None, 7):
        assert PM.read_metadata(junk) == (1, None, None)
    # a file cut inside its pixel data still opens lazily: the headers are all this reads
    data = tagged_file(pixels(100, 131, 3), 'JPEG', 6)
    assert PM.read_metadata(data[:len(data) - 200])[0] == 6


def test_image_metadata_leaves_the_image_usable_for_exif_transpose():
    from PIL import Image, ImageOps
    a = pixels(7, 12, 3)
    im = Image.open(io.BytesIO(tagged_file(a, 'PNG', 6)))
    assert PM.image_metadata(im)[0] == 6
    assert np.array_equal(np.asarray(ImageOps.exif_transpose(im)), O.orient_numpy(a, 6))


@pytest.mark.parametrize('o', range(1, 9))
def test_points_move_with_their_pixels(o):
    H, W = 5, 9
    a = np.arange(H * W, dtype=np.int64).reshape(H, W)                # every pixel its own value
    up = O.orient_numpy(a, o)
    ys, xs = np.mgrid[0:H, 0:W]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)    # (x, y)
    moved = O.orient_points(pts, o, H, W)
    assert moved.shape == pts.shape
    mx, my = moved[:, 0].astype(int), moved[:, 1].astype(int)
    assert np.array_equal(moved, np.stack([mx, my], 1))               # integer pixels stay integer pixels
    assert np.array_equal(up[my, mx], a[ys.ravel(), xs.ravel()])
    assert np.array_equal(O.unorient_points(moved, o, H, W), pts)
    frac = pts[:7] + [0.25, -0.5]
    assert np.allclose(O.unorient_points(O.orient_points(frac, o, H, W), o, H, W), frac, atol=0, rtol=0)
    assert O.orient_points(pts.reshape(H, W, 2), o, H, W).shape == (H, W, 2)
    assert pts[3, 0] == 3.0                                            # the input is not written to


def _pillow_jpeg(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', **kw)
    return buf.getvalue()


def _exif_block(n_extra=0):
    from PIL import Image
    exif = Image.Exif()
    exif[0x010F] = 'a camera maker'
    exif[0x0132] = '2024:05:06 07:08:09'
    if n_extra:
        exif[0x9286] = 'x' * n_extra
    return exif.tobytes()


@pytest.mark.parametrize('icc_len', [None, 100, 65519, 65520, 200000])
@pytest.mark.parametrize('with_exif', [False, True])
def test_wrap_jpeg_with_metadata_is_pillows_file(icc_len, with_exif):
    img = pixels(33, 65, 3)
    scan = JO.scan(img, 75, 2)
    kw = {}
    if with_exif:
        kw['exif'] = _exif_block()
    if icc_len is not None:
        kw['icc_profile'] = profile(icc_len)
    want = _pillow_jpeg(img, **kw)
    got = JE.wrap_jpeg(scan, 33, 65, 3, 75, 2, **kw)
    assert got == want
    if not kw:
        assert got == JE.wrap_jpeg(scan, 33, 65, 3) == JE.wrap_jpeg(scan, 33, 65, 3, exif=b'', icc_profile=b'')
    # the layout the issue names: APP0, APP1 Exif, APP2 ICC_PROFILE chunks of at most 65519 profile bytes, then DQT
    at = got.index(b'\xff\xe0') + 18
    if with_exif:
        assert got[at:at + 2] == b'\xff\xe1' and got[at + 4:at + 10] == b'Exif\x00\x00'
        at += 2 + int.from_bytes(got[at + 2:at + 4], 'big')
    if icc_len:
        chunks = -(-icc_len // 65519)
        for i in range(chunks):
            assert got[at:at + 2] == b'\xff\xe2' and got[at + 4:at + 16] == b'ICC_PROFILE\x00' and got[at + 16] == i + 1 and got[at + 17] == chunks
            at += 2 + int.from_bytes(got[at + 2:at + 4], 'big')
    assert got[at:at + 2] == b'\xff\xdb'


def test_exif_too_long_for_one_segment():
    """Pillow's save() raises at 65534 bytes; wrap_jpeg says the same, and the jobs drop the block with a warning before either."""
    img = pixels(8, 8, 3)
    block = _exif_block()                                             # save() writes the bytes it is given: pad a real block to the length
    fits, too_long = block + b'\x00' * (JE.EXIF_MAX - len(block)), block + b'\x00' * (JE.EXIF_MAX + 1 - len(block))
    assert len(fits) == JE.EXIF_MAX == PM.EXIF_MAX and len(too_long) == JE.EXIF_MAX + 1
    assert JE.wrap_jpeg(JO.scan(img, 75, 2), 8, 8, 3, exif=fits) == _pillow_jpeg(img, exif=fits)
    with pytest.raises(ValueError, match='EXIF data is too long'):
        _pillow_jpeg(img, exif=too_long)
    with pytest.raises(ValueError, match='EXIF data is too long'):
        JE.wrap_jpeg(JO.scan(img, 75, 2), 8, 8, 3, exif=too_long)
    assert PM.droppable(fits) is fits and PM.droppable(None) is None


def test_droppable_warns(capsys):
    assert PM.droppable(b'E' * (PM.EXIF_MAX + 1), 'a.jpg') is None
    assert 'a.jpg' in capsys.readouterr().out


@pytest.mark.parametrize('C', [1, 3, 4])
def test_wrap_png_metadata_reads_back_in_pillow(C):
    from PIL import Image
    a = pixels(33, 65, C)
    rows = a.reshape(33, -1)
    stream = zlib.compress(b''.join(b'\x00' + r.tobytes() for r in rows))
    exif, icc = _exif_block(), profile(70000)
    plain = PE.wrap_png(stream, 33, 65, C)
    assert plain == PE.wrap_png(stream, 33, 65, C, None, None) == PE.wrap_png(stream, 33, 65, C, b'', b'')
    for kw in (dict(exif=exif), dict(icc_profile=icc), dict(exif=exif, icc_profile=icc)):
        im = Image.open(io.BytesIO(PE.wrap_png(stream, 33, 65, C, **kw)))
        im.load()
        assert np.array_equal(np.asarray(im), a)
        assert im.info.get('icc_profile') == kw.get('icc_profile')
        assert (im.getexif().tobytes() if 'exif' in kw else None) == kw.get('exif')
        assert im.info.get('exif') == (kw['exif'] if 'exif' in kw else None)
    both = PE.wrap_png(stream, 33, 65, C, exif=exif, icc_profile=icc)
    assert both.index(b'IHDR') < both.index(b'iCCP') < both.index(b'eXIf') < both.index(b'IDAT')
    # Pillow writes the same two chunks for the same arguments
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, 'PNG', exif=exif, icc_profile=icc)
    theirs = Image.open(io.BytesIO(buf.getvalue()))
    assert theirs.info['icc_profile'] == icc and theirs.getexif().tobytes() == exif


def test_per_image_metadata_lists():
    assert JE.per_image(None, 3, 'exif') == [None] * 3
    assert JE.per_image([b'a', None], 2, 'exif') == [b'a', None]
    for bad in (b'abc', [b'a'], []):
        with pytest.raises(ValueError, match='exif'):
            JE.per_image(bad, 3, 'exif')


# ---- the readers and the host jobs ------------------------------------------------------------------------------------------------------
def test_read_rgb_orient_and_metadata(tmp_path):
    from PIL import Image
    from ctrlhair_amd import alignment as AL
    from ctrlhair_amd import dataset as D
    a = pixels(33, 65, 3)
    icc = profile(400)
    for o in (None, 1, 3, 6, 9):
        p = str(tmp_path / f'o{o}.png')
        with open(p, 'wb') as f:
            f.write(tagged_file(a, 'PNG', o, icc=icc))
        assert np.array_equal(D.read_rgb(p), a)                                       # the default: the stored pixels
        up = D.read_rgb(p, orient=True)
        assert np.array_equal(up, O.orient_numpy(a, o))
        px, meta = D.read_rgb(p, orient=True, metadata=True)
        assert np.array_equal(px, up) and meta == PM.read_metadata(open(p, 'rb').read()) and meta[2] == icc
        px, meta = D.read_rgb(p, metadata=True)
        assert np.array_equal(px, a) and meta == PM.read_metadata(open(p, 'rb').read(), strip=False)
        px2, meta2 = AL.read_photo(p)
        assert np.array_equal(px2, up) and meta2 == PM.read_metadata(open(p, 'rb').read())
        assert np.array_equal(AL.read_photo(p, orient=False)[0], a)
    grey = str(tmp_path / 'grey.jpg')
    with open(grey, 'wb') as f:
        f.write(tagged_file(pixels(20, 31, 1), 'JPEG', 8))
    stored = np.asarray(Image.open(grey).convert('RGB'))
    assert np.array_equal(D.read_rgb(grey, orient=True), O.orient_numpy(stored, 8))


class _WindowAligner:
    """Stands for FaceAligner in the host jobs: the 'crop' is the 8 x 8 window of the photo whose corner is the first landmark, the
    paste-back puts the edit there -- enough to see which pixels and which landmarks a job hands over."""
    handle = device = None

    def align(self, photo, lm, size):
        x, y = int(lm[0][0]), int(lm[0][1])
        return np.ascontiguousarray(np.asarray(photo)[y:y + size, x:x + size]), None

    def paste_back(self, photo, edit, plan):
        import torch
        out = np.array(photo)
        out[plan[1]:plan[1] + edit.shape[0], plan[0]:plan[0] + edit.shape[1]] = edit
        return torch.from_numpy(out)[None]


def _eight(tmp_path, ext, icc=None):
    """One upright photo as nine files that display identically: untagged, and for each orientation the inversely turned pixels plus
    the tag.  -> (folder of the untagged file, folder of the eight, the upright pixels, upright landmarks per name, stored landmarks)."""
    from PIL import Image
    up = pixels(40, 56, 3, seed=3)
    plain, tagged = tmp_path / 'plain', tmp_path / 'tagged'
    plain.mkdir(), tagged.mkdir()
    fmt = 'PNG' if ext == 'png' else 'JPEG'
    lm = np.zeros((68, 2))
    lm[:] = [13.0, 9.0]
    (plain / f'u.{ext}').write_bytes(tagged_file(up, fmt, None, icc=icc))
    lms_up, lms_stored = {f'u.{ext}': lm}, {}
    for o in range(1, 9):
        stored = np.ascontiguousarray(O.orient_numpy(up, O.inverse_orientation(o)))
        assert np.array_equal(O.orient_numpy(stored, o), up)
        (tagged / f'o{o}.{ext}').write_bytes(tagged_file(stored, fmt, o, icc=icc))
        lms_up[f'o{o}.{ext}'] = lm
        lms_stored[f'o{o}.{ext}'] = O.unorient_points(lm, o, *stored.shape[:2])
    return plain, tagged, up, lms_up, lms_stored


def test_host_crop_job_orients(tmp_path):
    from PIL import Image
    from ctrlhair_amd import dataset as D
    plain, tagged, up, lms_up, lms_stored = _eight(tmp_path, 'png', icc=profile(300))
    al = _WindowAligner()
    D.crop_faces(al, str(plain), str(tmp_path / 'want'), 'ds', lms_up, size=8)
    want = (tmp_path / 'want' / 'u.png').read_bytes()
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(want))), up[9:17, 13:21])
    D.crop_faces(al, str(tagged), str(tmp_path / 'a'), 'ds', lms_up, size=8, orient=True)
    D.crop_faces(al, str(tagged), str(tmp_path / 'b'), 'ds', lms_stored, size=8, orient=True, landmark_frame='stored')
    D.crop_faces(al, str(tagged), str(tmp_path / 'c'), 'ds', lms_up, size=8)            # the default: the stored pixels, as before
    D.crop_faces(al, str(tagged), str(tmp_path / 'k'), 'ds', lms_up, size=8, orient=True, metadata='keep')
    differ = 0
    for o in range(1, 9):
        n = f'o{o}.png'
        assert (tmp_path / 'a' / n).read_bytes() == (tmp_path / 'b' / n).read_bytes() == want, o
        differ += (tmp_path / 'c' / n).read_bytes() != want
        kept = Image.open(tmp_path / 'k' / n)
        assert np.array_equal(np.asarray(kept), up[9:17, 13:21]) and kept.info['icc_profile'] == profile(300)
        assert kept.getexif().get(0x0112) == (1 if o == 1 else None) and kept.getexif().get(0x010F) == 'a camera maker'
        assert 'icc_profile' not in Image.open(tmp_path / 'a' / n).info
    assert differ >= 6
    for bad in (dict(landmark_frame='sideways'), dict(metadata='some')):
        with pytest.raises(ValueError):
            D.crop_faces(al, str(tagged), str(tmp_path / 'x'), 'ds', lms_up, size=8, **bad)


def test_host_uncrop_job_orients_and_keeps_metadata(tmp_path, monkeypatch):
    from PIL import Image
    from ctrlhair_amd import alignment as AL
    from ctrlhair_amd import dataset as D
    monkeypatch.setattr(AL, 'align_plan', lambda lm, H, W, S: (int(lm[0][0]), int(lm[0][1]), H, W))
    icc = profile(300)
    plain, tagged, up, lms_up, lms_stored = _eight(tmp_path, 'png', icc=icc)
    edits = tmp_path / 'edits'
    edits.mkdir()
    edit = pixels(8, 8, 3, seed=9)
    for n in list(lms_up):
        Image.fromarray(edit).save(edits / n)
    al = _WindowAligner()
    D.uncrop_faces(al, str(plain), str(edits), str(tmp_path / 'want'), 'ds', lms_up)
    want = (tmp_path / 'want' / 'u.png').read_bytes()
    expect = up.copy()
    expect[9:17, 13:21] = edit
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(want))), expect)
    D.uncrop_faces(al, str(tagged), str(edits), str(tmp_path / 'a'), 'ds', lms_up, orient=True)
    D.uncrop_faces(al, str(tagged), str(edits), str(tmp_path / 'b'), 'ds', lms_stored, orient=True, landmark_frame='stored')
    D.uncrop_faces(al, str(tagged), str(edits), str(tmp_path / 'k'), 'ds', lms_up, orient=True, metadata='keep')
    D.uncrop_faces(al, str(tagged), str(edits), str(tmp_path / 's'), 'ds', lms_up, metadata='keep')
    for o in range(1, 9):
        n = f'o{o}.png'
        assert (tmp_path / 'a' / n).read_bytes() == (tmp_path / 'b' / n).read_bytes() == want, o
        kept = Image.open(tmp_path / 'k' / n)
        assert np.array_equal(np.asarray(kept), expect) and kept.info['icc_profile'] == icc and kept.getexif().get(0x0112) == (1 if o == 1 else None)
        # without orient the pixels stay the stored ones, and so does the tag that says how to show them
        stored = Image.open(tmp_path / 's' / n)
        assert stored.getexif().get(0x0112) == o and stored.info['icc_profile'] == icc
        assert stored.size == Image.open(tagged / n).size


def test_command_line_has_the_options():
    from ctrlhair_amd import dataset as D
    assert '--orient' in D.__doc__ and '--landmark-frame upright|stored' in D.__doc__ and '--metadata drop|keep' in D.__doc__
    for main in (D._main_crop, D._main_uncrop):
        with pytest.raises(SystemExit):
            main(['a', 'b', 'c', '--landmarks', 'x', '--landmark-frame', 'sideways'])
        with pytest.raises(SystemExit):
            main(['a', 'b', 'c', '--landmarks', 'x', '--metadata', 'some'])


# ---- the batch and its host-side check ----------------------------------------------------------------------------------------------------
def test_batch_packing():
    blob, offs, total = O.pack_batch([4096, 8192, 12288], [(5, 7, 3), (64, 64, 1), (3, 2, 4)], [6, 3, 8])
    assert blob.dtype == np.uint8 and blob.size == 3 * O.DESC.itemsize == 96
    d = blob.view(O.DESC)
    assert [tuple(int(v) for v in r) for r in d] == [(4096, 0, 5, 7, 3, 6), (8192, 256, 64, 64, 1, 3), (12288, 4352, 3, 2, 4, 8)]
    assert offs == [0, 256, 4352] and total == 4352 + 24
    _, offs, total = O.pack_batch([4096, 8192], [(5, 7, 3), (2, 2, 1)], [6, 2], align=1)
    assert offs == [0, 105] and total == 109
    for bad in (dict(shapes=[(0, 4, 3)]), dict(shapes=[(4, 32769, 3)]), dict(shapes=[(4, 4, 2)]), dict(orientations=[0]),
                dict(orientations=[9]), dict(orientations=[True]), dict(addresses=[], shapes=[], orientations=[]), dict(align=0)):
        args = dict(addresses=[4096], shapes=[(4, 4, 3)], orientations=[6])
        args.update(bad)
        with pytest.raises(ValueError):
            O.pack_batch(**args)


DST = 1 << 32            # a destination address for the aliasing test; the sources of the cases lie below it


def hostile_batches():
    """(case, blob, N, dst address, dst bytes, accepted) for the library's host-side check of a batch: good ones, each documented
    refusal, and a good batch with single words overwritten (accepted = None: either answer, but no read outside the blob and no run
    outside the destination)."""
    shapes = [(5, 7, 3), (64, 64, 1), (130, 67, 4), (1, 1, 3)]
    good, _, total = O.pack_batch([4096, 1 << 20, 2 << 20, 3 << 20], shapes, [6, 3, 8, 2], align=1)
    yield 'good', good, 4, DST, total, True
    yield 'good, fewer images than descriptors said', good[:64], 2, DST, total, True
    yield 'good, a larger buffer', good, 4, DST, total + 1000, True
    yield 'good, destination address unknown', good, 4, 0, total, True
    every, _, t8 = O.pack_batch([4096 + (i << 20) for i in range(8)], [(65, 127, 3)] * 8, list(range(1, 9)))
    yield 'every orientation', every, 8, DST, t8, True
    big, _, tb = O.pack_batch([4096], [(2048, 1025, 4)], [5])
    yield 'many tiles', big, 1, DST, tb, True
    yield 'N 0', good, 0, DST, total, False
    yield 'N 65536', good, 65536, DST, total, False
    yield 'N larger than the batch', good, 5, DST, total, False
    yield 'N smaller than the batch', good, 3, DST, total, False
    yield 'cut inside a descriptor', good[:100], 4, DST, total, False
    yield 'buffer one byte short', good, 4, DST, total - 1, False
    yield 'empty buffer', good, 4, DST, 0, False
    yield 'buffer wraps', good, 4, (1 << 64) - 16, total, False

    def edited(n, **fields):
        b = good.copy()
        d = b.view(O.DESC)
        for k, v in fields.items():
            d[k][n] = v
        return b

    for case, b in (('H 0', edited(0, H=0)), ('W 32769', edited(1, W=32769)), ('H negative', edited(1, H=-64)),
                    ('C 2', edited(0, C=2)), ('C 0', edited(0, C=0)), ('C 5', edited(2, C=5)), ('orientation 0', edited(0, orient=0)),
                    ('orientation 9', edited(3, orient=9)), ('orientation negative', edited(1, orient=-6)),
                    ('null address', edited(2, src=0)), ('offset past the end', edited(3, dst=total)),
                    ('offset far past the end', edited(3, dst=1 << 62)), ('offset negative', edited(0, dst=-1)),
                    ('extent past the end', edited(3, dst=total - 2)), ('offsets descend', edited(1, dst=0)),
                    ('overlaps the image before', edited(2, dst=int(good.view(O.DESC)['dst'][2]) - 1)),
                    ('a larger image than its slot', edited(1, H=65)),
                    ('H * W * C past the buffer', edited(3, H=32768, W=32768, C=4)),
                    ('source inside the destination', edited(1, src=DST + 5)),
                    ('source ends inside the destination', edited(1, src=DST - 10)),
                    ('source wraps', edited(1, src=(1 << 64) - 5))):
        yield case, b, 4, DST, total, False
    rng = np.random.default_rng(11)
    for i in range(300):
        b = good.copy()
        w = b.view(np.int32)
        at = int(rng.integers(0, w.size))
        w[at] = int(rng.choice([-1, 0, 1, 2, 5, 9, 2 ** 31 - 1, -2 ** 31, 65537, int(rng.integers(-2 ** 31, 2 ** 31))]))
        yield f'word {at} overwritten ({i})', b, 4, DST, total, None


def test_workspace_query_checks_the_batch():
    """ch_orient_workspace_bytes is the entry's own check, and host code: every hostile batch whose lie does not need the destination's
    address gets the documented answer here, without a GPU (tools/orient_check_host.cpp runs all of them under sanitizers)."""
    import ctypes
    from ctrlhair_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    query = lib.load().ch_orient_workspace_bytes
    for case, blob, N, dst, dst_bytes, accepted in hostile_batches():
        blob = np.ascontiguousarray(blob)
        need = int(query(blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, N, dst_bytes))
        if accepted is not None and 'destination' not in case and 'wraps' not in case:
            assert (need > 0) == accepted, case
        if need:
            assert need % 256 == 0 and need >= blob.nbytes, case
    assert int(query(None, 0, 1, 4)) == 0


def test_batch_check_under_sanitizers(tmp_path):
    """csrc/orient_batch.h as a stand-alone CPU program under AddressSanitizer and UndefinedBehaviorSanitizer: the same cases; each batch
    is malloc'ed at its size, and for every batch that passes the program repeats the kernel's tile walk and checks every run."""
    import shutil
    import subprocess
    clang = next((p for p in ('/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++') if os.path.exists(p)), None) or shutil.which('clang++')
    assert clang, 'no ROCm clang++ to build tools/orient_check_host.cpp with'
    exe = str(tmp_path / 'orient_check_host')
    r = subprocess.run([clang, '-O1', '-g', '-std=c++17', '-Wall', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                        os.path.join(ROOT, 'tools', 'orient_check_host.cpp'), '-o', exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    cases = list(hostile_batches())
    lines = []
    for i, (case, blob, N, dst, dst_bytes, accepted) in enumerate(cases):
        path = str(tmp_path / f'{i:03d}.bin')
        np.ascontiguousarray(blob).tofile(path)
        lines.append(f'{path} {N} {dst} {dst_bytes}')
    (tmp_path / 'list.txt').write_text('\n'.join(lines) + '\n')
    r = subprocess.run([exe, str(tmp_path / 'list.txt')], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, f'sanitizer report or failure (exit {r.returncode}):\n{r.stderr[-4000:]}'
    rows = r.stdout.splitlines()
    assert len(rows) == len(cases)
    for (case, blob, N, dst, dst_bytes, accepted), row in zip(cases, rows):
        need, msg = row.split(' ', 1)
        assert (int(need) > 0) == (msg == 'ok'), (case, row)
        if accepted is not None:
            assert (msg == 'ok') == accepted, (case, row)
    said = {row.split(' ', 1)[1].split(': ')[-1] for row in rows}
    assert len(said) >= 10, said                                  # the cases reach most of the refusals


def test_importing_the_host_half_needs_no_torch():
    import subprocess
    import sys
    code = ('import sys; sys.modules["torch"] = None\n'
            'import numpy as np\n'
            'from ctrlhair_amd import orient as O, photometa as PM\n'
            'O.pack_batch([4096], [(5, 7, 3)], [6]); O.orient_numpy(np.zeros((2, 3, 3), np.uint8), 6); PM.read_metadata(b"x"); print("ok")')
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr[-2000:]
