"""Face alignment, host side: the oracle (Pillow / numpy / scipy themselves driven by align_plan) against the crops the reference
produced (tests/golden/align_golden.npz, made by tests/golden/make_align_golden.py), the plan against the recorded landmarks and
branches, crop_face's unchanged behaviour without landmarks, and the dataset crop job's sharding and skip report."""
import os

import numpy as np
import pytest

from ctrlhair_amd import alignment as A
from tests import align_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'align_golden.npz')
WINDOW = 256


@pytest.fixture(scope='module')
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check_crop(golden, name, crop):
    """`crop` against everything the fixture records for the case: the full crop or its centre window, and the SHA-256."""
    crop = np.asarray(crop)
    S = O.CASES[name][6]
    assert crop.shape == (S, S, 3) and crop.dtype == np.uint8
    if f'{name}/crop' in golden:
        want, got = golden[f'{name}/crop'], crop
    else:
        o = (S - WINDOW) // 2
        want, got = golden[f'{name}/window'], crop[o:o + WINDOW, o:o + WINDOW]
    diff = np.abs(want.astype(int) - got.astype(int))
    print(f'{name}: {int((diff > 0).sum())} differing values, max {int(diff.max())}')
    assert np.array_equal(want, got)
    assert O.sha256(crop) == str(golden[f'{name}/crop_sha256'])


def plan_of(name):
    photo, lm, S, T = O.case_inputs(name)
    return photo, lm, A.align_plan(lm, photo.shape[0], photo.shape[1], S, T)


@pytest.mark.parametrize('name', list(O.CASES))
def test_inputs_are_the_recorded_ones(golden, name):
    photo, lm, _, _ = O.case_inputs(name)
    assert O.sha256(photo) == str(golden[f'{name}/photo_sha256'])
    assert O.sha256(lm) == str(golden[f'{name}/lm_sha256'])


@pytest.mark.parametrize('name', list(O.CASES))
def test_plan_equals_the_recorded_landmarks_and_branches(golden, name):
    photo, lm, plan = plan_of(name)
    assert plan['landmarks'].dtype == np.int32 and np.array_equal(plan['landmarks'], golden[f'{name}/landmarks'])
    assert (plan['shrink'] > 1, plan['cropped'], plan['padded']) == tuple(bool(v) for v in golden[f'{name}/branches'])
    # geometry that follows from the definitions
    w, h = plan['resized']
    if plan['shrink'] > 1:
        assert (w, h) == (int(np.rint(photo.shape[1] / plan['shrink'])), int(np.rint(photo.shape[0] / plan['shrink'])))
    else:
        assert (w, h) == (photo.shape[1], photo.shape[0])
    x0, y0, x1, y1 = plan['crop']
    assert 0 <= x0 < x1 <= w and 0 <= y0 < y1 <= h
    assert plan['blur'] == pytest.approx(0.02 * plan['qsize'])
    side = np.hypot(*(plan['quad'][3] - plan['quad'][0]))
    assert side == pytest.approx(plan['qsize'], rel=1e-12)
    if plan['padded']:
        assert min(plan['pad']) >= int(np.rint(plan['qsize'] * 0.3)) and plan['gauss_radius'] == int(4 * plan['blur'] + 0.5)
        assert plan['gauss_w'].shape == (2 * plan['gauss_radius'] + 1,) and plan['gauss_w'].sum() == pytest.approx(1.0)
        assert plan['image_size'] == (x1 - x0 + plan['pad'][0] + plan['pad'][2], y1 - y0 + plan['pad'][1] + plan['pad'][3])
    else:
        assert plan['pad'] == (0, 0, 0, 0) and plan['image_size'] == (x1 - x0, y1 - y0)
    # Pillow's quad coefficients: pixel centres of the grid corners land on the quad's corners (+ 0.5)
    a, T = plan['coef'], plan['transform_size']
    for (gx, gy), corner in zip(((0, 0), (0, T), (T, T), (T, 0)), plan['quad'] + 0.5):
        assert a[0] + a[1] * gx + a[2] * gy + a[3] * gx * gy == pytest.approx(corner[0], abs=1e-6)
        assert a[4] + a[5] * gx + a[6] * gy + a[7] * gx * gy == pytest.approx(corner[1], abs=1e-6)
    packed = A.pack_plan(plan)
    assert packed.shape == (A.PLAN_LEN,) and packed.dtype == np.float64 and np.array_equal(packed[12:20], a)


@pytest.mark.parametrize('name', list(O.CASES))
def test_oracle_equals_the_reference_crop(golden, name):
    photo, lm, plan = plan_of(name)
    check_crop(golden, name, O.run_plan(photo, plan))


def test_cases_take_every_branch_and_size(golden):
    br = np.array([golden[f'{n}/branches'] for n in O.CASES], bool)
    assert br.any(0).all() and (~br).any(0).all()
    assert {O.CASES[n][6] for n in O.CASES} >= {256, 512, 1024}


def test_plan_accepts_81_points_and_rejects_bad_input():
    photo, lm, S, T = O.case_inputs('plain_256')
    lm81 = np.concatenate([lm, np.zeros((13, 2))])
    a, b = A.align_plan(lm, 900, 800, S, T), A.align_plan(lm81, 900, 800, S, T)
    assert np.array_equal(a['coef'], b['coef']) and np.array_equal(a['landmarks'], b['landmarks'])
    with pytest.raises(ValueError):
        A.align_plan(lm[:60], 900, 800, S)
    with pytest.raises(ValueError):
        A.align_plan(lm, 900, 800, 512, transform_size=256)
    bad = lm.copy()
    bad[40, 0] = np.nan
    with pytest.raises(ValueError):
        A.align_plan(bad, 900, 800, S)
    off = A.align_plan(lm, 900, 800, S, T, enable_padding=False)
    assert not off['padded']


def test_perspective_matrix_maps_the_corners():
    src = np.array([[10.5, 20.25], [8.0, 220.0], [230.0, 240.5], [215.0, 12.0]])
    dst = np.array([[0, 0], [0, 1], [1, 1], [1, 0]], np.float64)
    M = A.perspective_matrix(src, dst)
    h = M @ np.concatenate([src, np.ones((4, 1))], 1).T
    assert np.allclose((h[:2] / h[2]).T, dst, atol=1e-9)


def _bare_editor(models=None, landmarker=None):
    from ctrlhair_amd.hair_editor import HairEditor
    he = HairEditor.__new__(HairEditor)          # crop_face touches only models / img_size / landmarker
    he.models, he.img_size = models, 256
    if landmarker is not None:
        he.landmarker = landmarker
    return he


def test_crop_face_without_landmarks_still_raises_not_implemented():
    he = _bare_editor(models=object())
    with pytest.raises(NotImplementedError, match='dlib'):
        he.crop_face(np.zeros((64, 64, 3), np.uint8))


def test_crop_face_with_landmarks_needs_the_hip_models():
    photo, lm, _, _ = O.case_inputs('plain_256')
    with pytest.raises(RuntimeError, match='HipModels.aligner'):
        _bare_editor(models=object()).crop_face(photo, landmarks=lm)


class FakeAligner:
    """Stands in for alignment.FaceAligner: the host oracle."""

    def __init__(self):
        self.calls = []

    def align(self, img, lm, output_size, transform_size=4096, enable_padding=True):
        self.calls.append(tuple(img.shape))
        plan = A.align_plan(lm, img.shape[0], img.shape[1], output_size, 512)        # small grid: the job is under test, not the crop
        return O.run_plan(img, plan), plan['landmarks']


class FakeModels:
    def __init__(self):
        self.aligner = FakeAligner()


def test_crop_face_routes_landmarks_and_landmarker_and_saves(tmp_path):
    from PIL import Image
    photo, lm, _, _ = O.case_inputs('plain_256')
    he = _bare_editor(models=FakeModels())
    out = he.crop_face(photo, save_path=str(tmp_path / 'a.png'), landmarks=np.concatenate([lm, np.ones((13, 2))]))
    assert out.shape == (256, 256, 3) and out.dtype == np.uint8
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'a.png')), out)
    he2 = _bare_editor(models=FakeModels(), landmarker=lambda img: np.concatenate([lm, np.ones((13, 2))]))
    assert np.array_equal(he2.crop_face(photo), out)
    with pytest.raises(ValueError):
        he.crop_face(photo, landmarks=lm[:10])


def test_crop_job_shards_and_reports_missing_landmarks(tmp_path, capsys):
    from PIL import Image
    from ctrlhair_amd import dataset as D
    src = tmp_path / 'src'
    src.mkdir()
    photo, lm, _, _ = O.case_inputs('plain_256')
    small, lm_small = photo[::2, ::2], lm / 2
    names = [f'p{i}.png' for i in range(5)]
    for n in names:
        Image.fromarray(small).save(src / n)
    # three key layouts; p3 has no entry
    marks = {'p0.png': lm_small, 'p1': lm_small, D.code_key('ds', 'p2.png'): lm_small, 'p4.png': lm_small}
    np.savez(tmp_path / 'lm.npz', **marks)
    loaded = D.load_landmarks(str(tmp_path / 'lm.npz'))
    assert set(loaded) == set(marks)
    import pickle
    with open(tmp_path / 'lm.pkl', 'wb') as f:
        pickle.dump(marks, f)
    assert set(D.load_landmarks(str(tmp_path / 'lm.pkl'))) == set(marks)
    done_all, skipped_all = [], []
    for rank in range(2):
        fake = FakeAligner()
        done, skipped = D.crop_faces(fake, str(src), str(tmp_path / 'out'), 'ds', loaded, size=64, rank=rank, world=2)
        assert len(fake.calls) == len(done)
        assert set(done) | set(skipped) == set(names[rank::2])
        done_all += done
        skipped_all += skipped
    assert sorted(done_all) == ['p0.png', 'p1.png', 'p2.png', 'p4.png'] and skipped_all == ['p3.png']
    assert 'no landmarks for p3.png' in capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / 'out')) == sorted(done_all)
    want = O.run_plan(small, A.align_plan(lm_small, small.shape[0], small.shape[1], 64, 512))
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'out' / 'p2.png')), want)
