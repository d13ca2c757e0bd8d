"""The JPEG encoder's host side and its checker, without a GPU: the numpy oracle (tests/jpeg_oracle.py) writes Pillow's files byte for
byte -- the recorded ones (tests/golden/jpeg_golden.npz; tools/jpeg_golden.py) and, where this Pillow has a JPEG codec, live ones --, the
case set reaches every branch of the entropy coder, ctrlhair_amd.jpegenc writes the same container, and the crop jobs' jpeg options do
with jpeg='host' what the jobs did before there was an option."""
import io
import os

import numpy as np
import pytest

from ctrlhair_amd import jpegenc as JE
from tests import jpeg_cases as JC
from tests import jpeg_oracle as JO

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'jpeg_golden.npz')


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k].tobytes() for k in z.files if k not in ('pillow', 'libjpeg')}


@pytest.fixture(scope='module')
def oracle_files():
    """case id -> the oracle's file; the coverage counters of the whole set on the side."""
    JO.reset_counters()
    files = {JC.case_id(c): JO.file(JC.case_image(c), c[3], JC.SUBSAMPLING[c[4]]) for c in JC.CASES}
    return files, dict(JO.COUNTERS)


def _pillow_jpeg():
    try:
        from PIL import features
        return bool(features.check('jpg'))
    except Exception:
        return False


def _pillow_bytes(img, **options):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', **options)
    return buf.getvalue()


def test_case_list_is_what_the_issue_asks_for(golden):
    ids = [JC.case_id(c) for c in JC.CASES]
    assert len(set(ids)) == len(ids) and sorted(golden) == sorted(ids)
    sizes = {(c[0], c[1]) for c in JC.CASES}
    assert sizes >= {(1, 1), (7, 9), (8, 8), (16, 16), (17, 23), (33, 130), (64, 80), (264, 520), (424, 424)}
    for key, want in ((2, set(JC.CONTENTS)), (3, set(JC.QUALITIES)), (4, set(JC.MODES))):
        assert {c[key] for c in JC.CASES} == want
    assert {(c[2], c[3]) for c in JC.CASES} >= {(x, q) for x in JC.CONTENTS for q in JC.QUALITIES}
    assert {(c[2], c[4]) for c in JC.CASES} >= {(x, m) for x in JC.CONTENTS for m in JC.MODES}
    # the sizes that cross the device code's rounds: a scan over 64 KiB (more than 256 stuffing segments of 256 bytes) and more than
    # 8192 blocks (256 groups of 32 in one round of the bit-offset scan)
    big = JC.case_image((264, 520, 'noise', 75, '420'))
    assert len(JO.scan(big, 75, 2)) > 65536
    assert len(JO.scan_blocks(JC.case_image((424, 424, 'checker', 1, '444')), 1, 0)[0]) > 8192


def test_oracle_files_equal_the_recorded_pillow_files(oracle_files, golden):
    files, _ = oracle_files
    for cid, want in golden.items():
        assert files[cid] == want, cid


@pytest.mark.skipif(not _pillow_jpeg(), reason='this Pillow has no JPEG codec')
def test_oracle_files_equal_live_pillow():
    for c in JC.CASES[::3] + JC.CASES[-6:]:
        img = JC.case_image(c)
        assert JO.file(img, c[3], JC.SUBSAMPLING[c[4]]) == _pillow_bytes(img, quality=c[3], subsampling=JC.SUBSAMPLING[c[4]]), JC.case_id(c)


@pytest.mark.skipif(not _pillow_jpeg(), reason='this Pillow has no JPEG codec')
def test_save_without_options_is_quality_75_at_420():
    img = JC.image(33, 130, 'noise', '420')
    assert _pillow_bytes(img) == JO.file(img, 75, 2) == JE.wrap_jpeg(JO.scan(img, 75, 2), 33, 130, 3)
    assert _pillow_bytes(img) != JO.file(img, 75, 0)


def test_case_set_reaches_every_branch(oracle_files):
    _, counters = oracle_files
    print(counters)
    for name in ('zrl', 'eob', 'no_eob', 'stuffed', 'dummy'):
        assert counters[name] > 0, name
    assert counters['max_ac_size'] == 10 and counters['max_dc_cat'] >= 10


def test_wrap_jpeg_is_the_oracles_container(golden):
    for c in JC.CASES[::5]:
        img = JC.case_image(c)
        H, W, _, q, mode = c
        ss = JC.SUBSAMPLING[mode]
        assert JE.wrap_jpeg(JO.scan(img, q, ss), H, W, 1 if mode == 'grey' else 3, q, ss) == golden[JC.case_id(c)], JC.case_id(c)
    f = JE.wrap_jpeg(b'\x00', 2, 3, 3)
    assert f[:4] == b'\xff\xd8\xff\xe0' and f[-3:] == b'\x00\xff\xd9'
    assert JE.wrap_jpeg(b'\x00', 2, 3, 3, subsampling='444') == JE.wrap_jpeg(b'\x00', 2, 3, 3, subsampling=0) != f


def test_quant_tables():
    for q in (1, 10, 25, 49, 50, 51, 75, 90, 99, 100):
        for got, want in zip(JE.quant_tables(q), JO.quant_tables(q)):
            assert got.dtype == np.uint8 and got.shape == (64,) and np.array_equal(got, want), q
    assert set(JE.quant_tables(100)[0]) == {1} and JE.quant_tables(1)[0].max() == 255
    assert tuple(JE.quant_tables(50)[0]) == JE.BASE_LUMA and tuple(JE.quant_tables(50)[1]) == JE.BASE_CHROMA
    assert JE.ZIGZAG == tuple(JO.ZIGZAG)


def test_errors():
    for bad in (0, 101, -1, 75.0, True, None, '75'):
        with pytest.raises(ValueError, match='quality'):
            JE.quant_tables(bad)
        with pytest.raises(ValueError, match='quality'):
            JE.wrap_jpeg(b'', 8, 8, 3, quality=bad)
    for bad in (1, 3, -1, '422', None, 2.0, True):
        with pytest.raises(ValueError, match='subsampling'):
            JE.wrap_jpeg(b'', 8, 8, 3, subsampling=bad)
    for C in (0, 2, 4):
        with pytest.raises(ValueError, match='C must be'):
            JE.wrap_jpeg(b'', 8, 8, C)
    for H, W in ((0, 8), (8, 0), (65536, 8)):
        with pytest.raises(ValueError, match='H and W'):
            JE.wrap_jpeg(b'', H, W, 3)
    for bad in ('bogus', None, 'Device', ''):
        with pytest.raises(ValueError, match='jpeg'):
            JE.check_jpeg_mode(bad)
    assert JE.check_jpeg_mode('host') == 'host' and JE.check_jpeg_mode('device') == 'device'
    assert JE.check_jpeg_params(75, '420') == (75, 2) and JE.check_jpeg_params(np.int64(1), 0) == (1, 0)


# ---- the jobs' options, with stub aligners --------------------------------------------------------------------------------------------
class _StubAligner:
    """No handle and no device: jpeg='host' must not need either."""

    def __init__(self, crop):
        self.crop = crop

    def align(self, photo, lm, size):
        return self.crop, None

    def paste_back(self, photo, edit, plan):
        import torch
        return torch.from_numpy(np.array(photo))[None]


def _photos(tmp_path, names):
    from PIL import Image
    src = tmp_path / 'src'
    src.mkdir()
    photo = JC.image(48, 72, 'smooth', '420')
    for n in names:
        Image.fromarray(photo).save(src / n)
    lm = np.stack([np.linspace(10, 60, 68), np.linspace(8, 40, 68)], axis=1)
    return src, {n: lm for n in names}


def _read(folder, n):
    with open(os.path.join(str(folder), n), 'rb') as f:
        return f.read()


@pytest.mark.skipif(not _pillow_jpeg(), reason='this Pillow has no JPEG codec')
def test_crop_job_jpeg_host_writes_what_it_wrote_before(tmp_path):
    from PIL import Image
    from ctrlhair_amd import dataset as D
    names = ['a.jpg', 'b.jpeg', 'c.png', 'd.bmp', 'E.JPG']
    src, lms = _photos(tmp_path, names)
    crop = JC.image(32, 32, 'noise', '420')
    stub = _StubAligner(crop)
    done, _ = D.crop_faces(stub, str(src), str(tmp_path / 'plain'), 'ds', lms, size=32)
    assert sorted(done) == sorted(names)
    done, _ = D.crop_faces(stub, str(src), str(tmp_path / 'host'), 'ds', lms, size=32, jpeg='host', jpeg_quality=75, jpeg_subsampling=2)
    assert sorted(done) == sorted(names)
    want = {}
    for n in names:
        buf = io.BytesIO()
        Image.fromarray(crop).save(buf, {'png': 'PNG', 'bmp': 'BMP'}.get(n.rsplit('.', 1)[1].lower(), 'JPEG'))
        want[n] = buf.getvalue()
        assert _read(tmp_path / 'plain', n) == _read(tmp_path / 'host', n) == want[n], n
    assert want['a.jpg'] == JO.file(crop, 75, 2)
    # the two options reach Pillow for the JPEG names alone
    D.crop_faces(stub, str(src), str(tmp_path / 'q'), 'ds', lms, size=32, jpeg_quality=90, jpeg_subsampling='444')
    for n in names:
        got = _read(tmp_path / 'q', n)
        assert got == (JO.file(crop, 90, 0) if D._is_jpeg(n) else want[n]), n
    with pytest.raises(ValueError, match='jpeg'):
        D.crop_faces(stub, str(src), str(tmp_path / 'x'), 'ds', lms, jpeg='bogus')
    with pytest.raises(ValueError, match='quality'):
        D.crop_faces(stub, str(src), str(tmp_path / 'x'), 'ds', lms, jpeg_quality=0)
    with pytest.raises(ValueError, match='subsampling'):
        D.crop_faces(stub, str(src), str(tmp_path / 'x'), 'ds', lms, jpeg_subsampling=1)


@pytest.mark.skipif(not _pillow_jpeg(), reason='this Pillow has no JPEG codec')
def test_uncrop_job_jpeg_host_writes_what_it_wrote_before(tmp_path, monkeypatch):
    from PIL import Image
    from ctrlhair_amd import alignment as AL
    from ctrlhair_amd import dataset as D
    monkeypatch.setattr(AL, 'align_plan', lambda *a, **k: None)
    names = ['a.jpg', 'c.png']
    src, lms = _photos(tmp_path, names)
    edits = tmp_path / 'edits'
    edits.mkdir()
    for n in names:
        Image.fromarray(JC.image(16, 16, 'flat', '420')).save(edits / n)
    stub = _StubAligner(None)
    for folder, kw in (('plain', {}), ('host', dict(jpeg='host', jpeg_quality=75, jpeg_subsampling='420')), ('q', dict(jpeg_quality=25))):
        done, skipped = D.uncrop_faces(stub, str(src), str(edits), str(tmp_path / folder), 'ds', lms, **kw)
        assert sorted(done) == names and skipped == []
    photo = D.read_rgb(str(src / 'a.jpg'))                                  # what the stub pastes back: the decoded photo itself
    assert _read(tmp_path / 'plain', 'a.jpg') == _read(tmp_path / 'host', 'a.jpg') == JO.file(photo, 75, 2)
    assert _read(tmp_path / 'q', 'a.jpg') == JO.file(photo, 25, 2)
    assert _read(tmp_path / 'plain', 'c.png') == _read(tmp_path / 'host', 'c.png') == _read(tmp_path / 'q', 'c.png')
    with pytest.raises(ValueError, match='jpeg'):
        D.uncrop_faces(stub, str(src), str(edits), str(tmp_path / 'x'), 'ds', lms, jpeg='gpu')


def test_command_line_has_the_options():
    from ctrlhair_amd import dataset as D
    for job in ('crop', 'uncrop'):
        assert '--jpeg host|device' in D.__doc__
    for main in (D._main_crop, D._main_uncrop):
        with pytest.raises(SystemExit):
            main(['a', 'b', 'c', '--landmarks', 'x', '--jpeg', 'bogus'])
        with pytest.raises(SystemExit):
            main(['a', 'b', 'c', '--landmarks', 'x', '--jpeg-subsampling', '422'])
        with pytest.raises(SystemExit):
            main(['a', 'b', 'c', '--landmarks', 'x', '--jpeg-quality', '0'])
