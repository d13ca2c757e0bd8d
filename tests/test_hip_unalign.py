"""Paste-back on the HIP library (csrc/face_unalign.hip) against the float64 oracle of tests/unalign_oracle.py, on the cases of
tests/unalign_cases.py.  The kernel's coordinates are float64 and fixed operation by operation, so its alpha == 0 set is the
oracle's; its tap sums are float32, so a value within about 1e-2 grey levels of a rounding boundary may land on the other side:
every pixel within one grey level, at most 2 % of the pixels inside bbox different."""
import numpy as np
import pytest
import torch

from tests import unalign_cases as UC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def aligner():
    from ctrlhair_amd.alignment import FaceAligner
    return FaceAligner(device='cuda:0')


def _run(aligner, name, **over):
    c = dict(UC.inputs(name), **over)
    out = aligner.paste_back(c['photo'], c['edits'], c['plan_u'], weight=c['weight'], feather=c['feather'])
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize('name', sorted(UC.CASES))
def test_against_oracle(aligner, name):
    c = UC.inputs(name)
    got = _run(aligner, name)
    assert got.shape == (c['edits'].shape[0],) + c['photo'].shape and got.dtype == np.uint8
    r = UC.compare(name, got)
    print(f'{name}: max {r["max"]}, share of differing pixels inside bbox {100 * r["share"]:.4f} %')
    assert r['photo_kept'], 'a pixel outside bbox or with alpha == 0 differs from the photo'
    assert r['max'] <= 1
    assert r['share'] <= 0.02
    assert (got != c['photo'][None]).any(), 'nothing was pasted'


@pytest.mark.parametrize('name', ['e_batch_hard', 'e_batch_feather', 'f_origin'])
def test_batch_equals_single_calls(aligner, name):
    c = UC.inputs(name)
    got = _run(aligner, name)
    for n in range(c['edits'].shape[0]):
        one = _run(aligner, name, edits=c['edits'][n])
        assert one.shape[0] == 1 and np.array_equal(one[0], got[n]), f'image {n} of the batch differs from its N = 1 call'


def test_align_plan_dict_and_device_inputs(aligner):
    """paste_back takes align_plan's dict as well as unalign_plan's, and device tensors as well as numpy."""
    c = UC.inputs('a_magnify')
    dev = aligner.device
    got = aligner.paste_back(torch.from_numpy(c['photo']).to(dev), torch.from_numpy(c['edits']).to(dev), c['plan'])
    assert np.array_equal(got.cpu().numpy(), _run(aligner, 'a_magnify'))
    crop, plan = aligner.align(c['photo'], c['lm'], 32, 128, return_plan=True)
    assert plan['output_size'] == 32 and np.array_equal(plan['quad'], c['plan']['quad'])
    crop2, lms = aligner.align(c['photo'], c['lm'], 32, 128)
    assert np.array_equal(crop.cpu().numpy(), crop2.cpu().numpy()) and np.array_equal(lms, plan['landmarks'])


def test_rejects_bad_arguments(aligner):
    c = UC.inputs('a_magnify')
    with pytest.raises(ValueError, match='output_size is 32'):
        aligner.paste_back(c['photo'], np.zeros((64, 64, 3), np.uint8), c['plan_u'])
    with pytest.raises(ValueError, match='weight map'):
        aligner.paste_back(c['photo'], c['edits'], c['plan_u'], weight=np.zeros((8, 8), np.uint8))
    with pytest.raises(ValueError, match='does not fit'):
        aligner.paste_back(c['photo'][:100], c['edits'], c['plan_u'])
    bad = dict(c['plan_u'], A=c['plan_u']['A'] * np.nan)
    with pytest.raises(RuntimeError, match='ch_face_unalign'):
        aligner.paste_back(c['photo'], c['edits'], bad)


def test_backend_outputs_in_photo_hair_region():
    """Backend.outputs_in_photo(region='hair') on procedural weights equals outputs() followed by paste_back with the same weight,
    bit for bit; crop_face returns what it returned before and remembers the photo and the plan."""
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.hair_editor import procedural_weights
    from ctrlhair_amd.ui.backend import Backend
    from tests import align_oracle as AO
    ngf = 16                                       # a tiny SEAN generator; the other networks are full size
    w = procedural_weights(0, 64)
    w['sean'] = P.sean_state_dict(0, ngf)
    torch.manual_seed(0)
    be = Backend(2.5, blending=False, weights=w, device=0, max_batch=2)
    with pytest.raises(RuntimeError, match='crop_face'):
        be.paste_back(np.zeros((256, 256, 3), np.uint8))
    photo = AO.make_photo(41, 420, 380)
    lm = AO.make_landmarks(141, (190.0, 180.0), 50.0, 9.0)
    crop = be.crop_face(photo, landmarks=lm)
    assert crop.shape == (256, 256, 3) and be.last_alignment['plan']['output_size'] == 256
    assert np.array_equal(crop, be.models.aligner.align(photo, lm, 256)[0].cpu().numpy())
    be.noise = torch.from_numpy(P.noise_planes(1, 256, ngf, seed=77)).cuda()
    be.set_input_img(crop)
    lat = [be.copy_latent(), be.copy_latent()]
    lat[1].curliness = lat[1].curliness + 0.7
    got, masks = be.outputs_in_photo(lat, region='hair')
    imgs, masks2 = be.outputs(lat)
    weight = be._region_weight('hair', masks2)
    assert weight.shape == (256, 256) and weight.dtype == torch.uint8 and set(np.unique(weight.cpu().numpy())) <= {0, 255}
    want = be.paste_back(np.stack(imgs), weight=weight)
    assert got.shape == (2, 420, 380, 3) and np.array_equal(masks, masks2)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    whole = be.outputs_in_photo(lat, region='crop')[0]
    assert np.array_equal(whole.cpu().numpy(), be.paste_back(np.stack(imgs)).cpu().numpy())
    one = be.output_in_photo(region='crop')
    assert one.shape == (420, 380, 3) and np.array_equal(one.cpu().numpy(), be.paste_back(be.output())[0].cpu().numpy())
    with pytest.raises(ValueError, match="'crop' or 'hair'"):
        be.outputs_in_photo(lat, region='face')
