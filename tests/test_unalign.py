"""The paste-back geometry (ctrlhair_amd.alignment.unalign_plan) and its host oracle (tests/unalign_oracle.py).  No GPU."""
import numpy as np
import pytest

from ctrlhair_amd import alignment as AL
from tests import align_oracle as AO
from tests import unalign_cases as UC
from tests import unalign_oracle as UO

# plans without shrink, with a sub-window crop, with padding, with shrink, with shrink and padding, without a crop
PLAN_CASES = sorted(AO.CASES)


def _plan(name):
    photo, lm, S, T = AO.case_inputs(name)
    plan = AL.align_plan(lm, photo.shape[0], photo.shape[1], S, T)
    return photo, lm, plan, AL.unalign_plan(plan, photo.shape[0], photo.shape[1])


def test_cases_cover_every_plan_branch():
    plans = [_plan(n)[2] for n in PLAN_CASES]
    assert any(p['shrink'] > 1 for p in plans) and any(p['shrink'] <= 1 for p in plans)
    assert any(p['cropped'] for p in plans) and any(not p['cropped'] for p in plans)
    assert any(p['padded'] for p in plans) and any(not p['padded'] for p in plans)
    assert any(p['shrink'] > 1 and p['padded'] for p in plans)


@pytest.mark.parametrize('name', PLAN_CASES)
def test_landmarks_map_to_the_plans(name):
    """A applied to the photo's landmarks gives the aligned landmarks align_plan reports.  Cap: 2 aligned pixels -- the plan rounds
    to integers (0.5), maps through float32 corners, and under a shrink divides by the factor where the edge-to-edge map multiplies
    by resized / size.  Measured maximum over the six fixture plans: 0.499 pixels (pad_right_1024): the integer rounding alone."""
    _, lm, plan, pu = _plan(name)
    got = lm[:68] @ pu['A'][:, :2].T + pu['A'][:, 2]
    err = np.abs(got - plan['landmarks']).max()
    print(f'{name}: max |A lm - plan landmarks| = {err:.3f} px')
    assert err <= 2.0


@pytest.mark.parametrize('name', PLAN_CASES)
def test_round_trip_and_corners(name):
    photo, _, plan, pu = _plan(name)
    S = plan['output_size']
    A3 = np.vstack([pu['A'], [0, 0, 1]])
    B3 = np.vstack([pu['Ainv'], [0, 0, 1]])
    assert np.abs(B3 @ A3 - np.eye(3)).max() <= 1e-9 and np.abs(A3 @ B3 - np.eye(3)).max() <= 1e-9
    # the quad's corners (NW, SW, SE, NE of the frame the transform read), taken to the photo by hand, land on the crop's corners
    zoom = np.array([photo.shape[1] / plan['resized'][0], photo.shape[0] / plan['resized'][1]])
    corners = (plan['quad'] + 0.5 - np.array(plan['pad'][:2]) + np.array(plan['crop'][:2])) * zoom
    got = corners @ pu['A'][:, :2].T + pu['A'][:, 2]
    assert np.abs(got - np.array([[0, 0], [0, S], [S, S], [S, 0]])).max() <= 1e-9 * max(S, 1) * 16
    assert pu['output_size'] == S
    assert abs(np.hypot(*pu['A'][:, 0]) - np.hypot(*pu['A'][:, 1])) <= 1e-2 * pu['scale']      # a rotated square (up to resized's rounding)
    x0, y0, x1, y1 = pu['bbox']
    assert 0 <= x0 < x1 <= photo.shape[1] and 0 <= y0 < y1 <= photo.shape[0]


def test_pack_unalign_layout():
    _, _, _, pu = _plan('plain_256')
    v = AL.pack_unalign(pu)
    assert v.shape == (AL.UNALIGN_PLAN_LEN,) and v.dtype == np.float64
    assert np.array_equal(v[:6].reshape(2, 3), pu['A']) and tuple(v[6:10]) == pu['bbox'] and v[10] == pu['scale'] and v[11] == 256
    assert not v[12:].any()


def test_errors():
    photo, lm, plan, _ = _plan('plain_256')
    H, W = photo.shape[:2]
    away = dict(plan, quad=plan['quad'] - 10000.0)
    with pytest.raises(ValueError, match='outside the photo'):
        AL.unalign_plan(away, H, W)
    with pytest.raises(ValueError, match='not made for|was made for'):
        AL.unalign_plan(plan, H + 7, W)
    tiny = AO.make_landmarks(5, (100.0, 80.0), 9.0, 0.0)             # a 37-px quad asked for at 1024: 27 crop pixels per photo pixel
    with pytest.raises(ValueError, match='at most 16'):
        AL.unalign_plan(AL.align_plan(tiny, 160, 200, 1024, 1024), 160, 200)
    skew = dict(plan, quad=plan['quad'] + np.array([[0, 0], [0, 0], [9.0, 0], [0, 0]]))
    with pytest.raises(ValueError, match='not affine'):
        AL.unalign_plan(skew, H, W)


def test_hair_editor_paste_back_errors():
    from ctrlhair_amd.hair_editor import HairEditor
    he = HairEditor.__new__(HairEditor)                                  # no models: both errors come before any device work
    with pytest.raises(RuntimeError, match='crop_face'):
        he.paste_back(np.zeros((256, 256, 3), np.uint8))
    photo, _, plan, _ = _plan('plain_256')
    he.last_alignment = {'photo': photo, 'plan': plan}
    with pytest.raises(ValueError, match='output_size is 256'):
        he.paste_back(np.zeros((128, 128, 3), np.uint8))
    with pytest.raises(ValueError, match='output_size is 256'):
        he.paste_back(np.zeros((2, 256, 128, 3), np.uint8))


def test_oracle_round_trip_beats_half_pixel_shift():
    """Align a smooth photo with the host oracle of the alignment (Pillow), paste the crop back with the paste-back oracle (hard
    edge) and compare with the photo inside the eroded quad.  The same with the oracle's map displaced by half a photo pixel gives the
    error a geometry slip of that size produces; the correct map must stay at or below a quarter of it.  Measured mean absolute
    differences: 0.478 grey levels (correct map) against 3.062 (shifted)."""
    H = W = 300
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    photo = np.stack([127.5 + 100 * np.sin(xx / 11.0 + yy / 23.0), 127.5 + 100 * np.cos(yy / 9.0 - xx / 31.0),
                      127.5 + 60 * np.sin(xx / 14.0) + 50 * np.cos(yy / 12.0)], axis=-1)
    photo = np.clip(np.rint(photo), 0, 255).astype(np.uint8)
    lm = AO.make_landmarks(3, (150.0, 135.0), 30.0, 12.0)
    plan = AL.align_plan(lm, H, W, 128, 512)
    assert plan['shrink'] <= 1 and not plan['padded']
    pu = AL.unalign_plan(plan, H, W)
    crop = AO.run_plan(photo, plan)
    back, alpha = UO.paste_back(photo, crop, pu, feather_px=0.0, return_alpha=True)
    x, y = UO.crop_coordinates(pu['A'], *np.meshgrid(np.arange(W), np.arange(H)))
    inner = np.minimum(np.minimum(x, 128 - x), np.minimum(y, 128 - y)) > 8                   # the quad eroded by 8 crop pixels
    assert inner.sum() > 5000 and (alpha[inner] == 1).all()
    shifted = UO.paste_back(photo, crop, pu, feather_px=0.0, shift=(0.5 * pu['scale'], 0.5 * pu['scale']))
    err = np.abs(back[0].astype(np.float64) - photo)[inner].mean()
    err_shift = np.abs(shifted[0].astype(np.float64) - photo)[inner].mean()
    print(f'round trip: mean |back - photo| = {err:.3f}, with a half-pixel shift {err_shift:.3f}')
    assert err <= 0.25 * err_shift


@pytest.mark.parametrize('name', sorted(UC.CASES))
def test_float32_emulation_stays_under_half_the_cap(name):
    """The GPU test allows 2 % of the pixels inside bbox to differ from the float64 oracle (by one grey level).  The oracle's own
    per-pixel arithmetic in float32 on the very inputs of the GPU test must stay under half of that, or the inputs are badly chosen.
    Measured shares: 0 on every case but e_batch_feather, 0.004 % there; no pixel differs by more than one grey level."""
    c = UC.inputs(name)
    got = UO.paste_back(c['photo'], c['edits'], c['plan_u'], c['weight'], c['feather'], dtype=np.float32)
    r = UC.compare(name, got)
    print(f'{name}: float32 emulation vs float64: max {r["max"]}, share {100 * r["share"]:.4f} %')
    assert r['max'] <= 1 and r['share'] <= 0.01 and r['photo_kept']


def test_gpu_cases_reach_their_branches():
    u = {n: UC.inputs(n) for n in UC.CASES}
    assert u['a_magnify']['plan_u']['scale'] < 1 and not u['a_magnify']['plan']['padded']
    assert 2.5 < u['b_minify']['plan_u']['scale'] < 4
    assert u['c_padded']['plan']['padded'] and u['c_padded']['plan_u']['bbox'][:2] == (0, 0)
    assert u['d_shrink']['plan']['shrink'] >= 2
    assert u['e_batch_hard']['edits'].shape[0] == 3 and u['e_batch_hard']['feather'] == 0 and u['e_batch_feather']['feather'] == 2.0
    x0, y0, x1, y1 = u['f_origin']['plan_u']['bbox']
    assert (x0, y0) == (0, 0) and (x1 - x0) % 32 and (y1 - y0) % 8
    assert 6 * u['h_lds']['plan_u']['scale'] * 256 * 4 > 65536


def test_uncrop_job_shards_names_and_skips(tmp_path, capsys):
    """dataset.uncrop_faces with the oracle standing in for the aligner: same landmark file, sharding and file names as the crop job."""
    from PIL import Image
    from ctrlhair_amd import dataset as D

    class OracleAligner:
        def paste_back(self, photo, edits, plan):
            import torch
            return torch.from_numpy(UO.paste_back(photo, edits, AL.unalign_plan(plan, photo.shape[0], photo.shape[1])))

    c = UC.inputs('a_magnify')
    photos, edits = tmp_path / 'photos', tmp_path / 'edits'
    photos.mkdir(), edits.mkdir()
    for n in ('p0.png', 'p1.png', 'p2.png', 'p3.png'):
        Image.fromarray(c['photo']).save(photos / n)
        if n != 'p2.png':
            Image.fromarray(c['edits'][0]).save(edits / n)
    lms = {'p0.png': c['lm'], 'p1': c['lm'], 'ds___p2': c['lm']}                  # p3 has no landmarks, p2 no edit
    done_all, skipped_all = [], []
    for rank in range(2):
        done, skipped = D.uncrop_faces(OracleAligner(), str(photos), str(edits), str(tmp_path / 'out'), 'ds', lms, rank=rank, world=2)
        done_all += done
        skipped_all += skipped
    assert sorted(done_all) == ['p0.png', 'p1.png'] and sorted(skipped_all) == ['p2.png', 'p3.png']
    out = capsys.readouterr().out
    assert 'no edit for p2.png' in out and 'no landmarks for p3.png' in out
    assert np.array_equal(np.asarray(Image.open(tmp_path / 'out' / 'p1.png')), UC.oracle('a_magnify')[0][0])
    with pytest.raises(ValueError, match='expected a 64 x 64 crop'):
        D.uncrop_faces(OracleAligner(), str(photos), str(edits), str(tmp_path / 'out'), 'ds', lms, size=64)
