"""Backend.transfer_latent_representation('shape') with the built-in GPU warper, and EditPipeline.transfer_shape."""
import numpy as np
import pytest
import torch

from ctrlhair_amd import procedural as P
from tests.test_backend import NGF, portrait, weights
from tests.warp_cases import cases


def _landmarks():
    c = cases()
    return c[0]['face_lm'], c[0]['hair_lm']


def test_without_warper_or_landmarks_the_transfer_raises():
    from ctrlhair_amd.ui.backend import Backend
    from tests.oracle_models import OracleModels
    be = Backend(2.5, blending=False, models=OracleModels(weights(), NGF))
    be.set_input_img(portrait(3))
    be.set_target_img(portrait(4))
    with pytest.raises(RuntimeError, match='set_landmarks'):
        be.transfer_latent_representation('shape')


def test_injected_warper_takes_precedence_and_keeps_its_arguments():
    from ctrlhair_amd.ui.backend import Backend
    from tests.oracle_models import OracleModels
    calls = []

    def warper(hair_img, face_img, wrap_temp_folder=None, need_crop=True):
        calls.append((hair_img, face_img, wrap_temp_folder, need_crop))
        out = np.zeros((512, 512), int)
        out[100:300, 150:350] = 13
        return out, {'hair_mask': (out == 13).astype('uint8')}
    be = Backend(2.5, blending=False, models=OracleModels(weights(), NGF), warper=warper, landmarker=lambda img: 1 / 0)
    be.set_input_img(portrait(3))
    be.set_target_img(portrait(4))
    be.set_landmarks(*_landmarks())
    be.transfer_latent_representation('shape')
    assert len(calls) == 1
    assert calls[0][0] is be.target_img and calls[0][1] is be.input_img and calls[0][2] == be.temp_path and calls[0][3] is False
    assert (be.warp_target == 13).sum() == 200 * 200 // 4
    assert torch.equal(be.cur_latent.shape, be.target_latent.shape)


@pytest.mark.gpu
def test_builtin_shape_transfer_on_the_gpu(hip_lib):
    from ctrlhair_amd.ui.backend import Backend
    be = Backend(2.5, blending=False, weights=weights(), device=0)
    be.set_input_img(portrait(3))
    be.set_target_img(portrait(4))
    before_mask, before_shape = be.cur_mask.copy(), be.cur_latent.shape.clone()
    with pytest.raises(RuntimeError, match='set_landmarks'):
        be.transfer_latent_representation('shape')
    be.set_landmarks(*_landmarks())
    be.transfer_latent_representation('shape')
    assert be.warp_target.shape == (256, 256) and be.warp_target.dtype == np.uint8
    assert torch.equal(be.cur_latent.shape, be.target_latent.shape) and be.cur_latent.shape is not be.target_latent.shape
    hc, _ = be.mask_generator.encode_labels(torch.tensor(be.warp_target[None], dtype=torch.uint8, device=be.device))
    assert torch.equal(hc, be.cur_latent.shape)
    decoded = be.mask_generator.decode_labels(be.cur_latent.shape, be.cur_latent.face)[0].cpu().numpy()
    assert np.array_equal(be.cur_mask, decoded)
    print('shape latent moved by', float((be.cur_latent.shape - before_shape).abs().max()), '; mask pixels changed:',
          int((be.cur_mask != before_mask).sum()))
    # the landmarker route gives the same warp: pixels of the 256 x 256 images the Backend keeps
    lm_in, lm_tg = _landmarks()
    seen = []

    def landmarker(img):
        seen.append(img)
        return (lm_tg if img is be2.target_img else lm_in) * np.asarray(img).shape[1]
    be2 = Backend(2.5, blending=False, models=be.models, landmarker=landmarker)
    be2.set_input_img(portrait(3))
    be2.set_target_img(portrait(4))
    be2.transfer_latent_representation('shape')
    assert len(seen) == 2 and np.array_equal(be2.warp_target, be.warp_target)
    out = be.output()
    assert out.shape == (256, 256, 3) and out.dtype == np.uint8


def _u8(x):
    return (x * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).cpu().numpy()


def _same(a, b):
    """The batch-composition bound of tests/test_backend.py::test_batched_outputs_sweep_and_grid."""
    d = np.abs(a.astype(np.int32) - b.astype(np.int32))
    print(f'max level difference {int(d.max())}, pixels differing {int((d > 0).sum())} of {d.size}')
    return d.max() <= 1 and (d > 0).mean() < 1e-3


@pytest.mark.gpu
def test_pipeline_transfer_shape_equals_four_backend_transfers(hip_lib):
    """EditPipeline.transfer_shape at B = 4 against four runs of the Backend API (set_input_img, set_target_img, set_landmarks,
    transfer_latent_representation('shape'), output()) on the same photos, landmarks and noise.  The pipeline gets the
    Backend's own 512 x 512 parsings (labels512=), as tests/test_pipeline.py hands the Backend's labels to edit()."""
    from ctrlhair_amd.pipeline import EditPipeline
    from ctrlhair_amd.ui.backend import Backend
    B = 4
    be = Backend(2.5, blending=False, weights=weights(), device=0, max_batch=8)
    pipe = EditPipeline(models=be.models, img_size=256)
    cs = cases()
    lm, dlm = np.stack([c['face_lm'] for c in cs]), np.stack([c['hair_lm'] for c in cs])
    noise = torch.from_numpy(P.noise_planes(B, 256, NGF, seed=9)).to(be.device)
    faces, donors = [portrait(10 + i) for i in range(B)], [portrait(20 + i) for i in range(B)]
    outs, targets, masks, lab_face, lab_donor = [], [], [], [], []
    for i in range(B):
        be.noise = noise[i:i + 1]
        be.set_input_img(faces[i])
        be.set_target_img(donors[i])
        be.set_landmarks(lm[i], dlm[i])
        be.transfer_latent_representation('shape')
        outs.append(be.output())
        targets.append(be.warp_target.copy())
        masks.append(be.cur_mask.copy())
        lab_face.append(be._parse512(be.input_img))
        lab_donor.append(be._parse512(be.target_img))
    to_t = lambda imgs: torch.from_numpy(np.concatenate([be.preprocess_img(im) for im in imgs]).astype(np.float32)).to(be.device)
    st = {}
    out = pipe.transfer_shape(to_t(faces), to_t(donors), lm, dlm, sliders={}, noise=noise, stages=st,
                              labels512=torch.stack(lab_face + lab_donor))
    got = _u8(out)
    for i in range(B):
        assert np.array_equal(st['warp_target'][i, ::2, ::2].cpu().numpy(), targets[i]), f'pair {i}: warp target differs'
        assert np.array_equal(st['mask'][i].cpu().numpy(), masks[i]), f'pair {i}: decoded mask differs'
        assert _same(got[i], outs[i]), f'pair {i}: image differs'
    assert len({t.tobytes() for t in targets}) == B


@pytest.mark.gpu
def test_direction_of_the_transfer_against_the_host_oracle(hip_lib):
    """Which image gives the hair and which the face, and which landmark set goes with which, pinned independently of the code
    under test: with the fixture parsings in place of the parser, Backend.warp_target and EditPipeline's warp target must be the
    host oracle's label map for (donor = target image, face = input image), up to 2 % of the oracle's boundary band."""
    from ctrlhair_amd.pipeline import EditPipeline
    from ctrlhair_amd.ui.backend import Backend
    from tests.warp_cases import boundary_band, oracle
    c = cases()[1]
    want = oracle(1)[0]
    band = boundary_band(want == 13)
    be = Backend(2.5, blending=False, weights=weights(), device=0)
    be.set_input_img(portrait(3))
    be.set_target_img(portrait(4))
    be.set_landmarks(c['face_lm'], c['hair_lm'])                 # (input = face, target = donor of the hair)
    dev = lambda a: torch.from_numpy(a).to(be.device)
    be._parse512 = lambda img: dev(c['hair']) if img is be.target_img else dev(c['face'])
    be.transfer_latent_representation('shape')
    diff = be.warp_target != want[::2, ::2]
    print(f'Backend: {int(diff.sum())} pixels differ from the oracle, band {int(band[::2, ::2].sum())} pixels (at 256)')
    assert not (diff & ~band[::2, ::2]).any() and diff.sum() <= 0.02 * band[::2, ::2].sum()
    pipe = EditPipeline(models=be.models, img_size=256)
    img = torch.from_numpy(P.synthetic_images(1, 256, seed=5)).to(be.device)
    st = {}
    pipe.transfer_shape(img, img, c['face_lm'][None], c['hair_lm'][None], sliders={}, stages=st,
                        labels512=torch.stack([dev(c['face']), dev(c['hair'])]))
    diff = st['warp_target'][0].cpu().numpy() != want
    print(f'EditPipeline: {int(diff.sum())} pixels differ from the oracle, band {int(band.sum())} pixels')
    assert not (diff & ~band).any() and diff.sum() <= 0.02 * band.sum()
    # swapping the roles is a different label map: the check above can tell the directions apart
    swapped = pipe.warper.warp_batch(dev(c['face'])[None], dev(c['hair'])[None], c['face_lm'][None], c['hair_lm'][None])
    assert (swapped[0].cpu().numpy() != want).sum() > band.sum()
    # landmarks belong to the photo: loading another one forgets them
    be.set_target_img(portrait(5))
    with pytest.raises(RuntimeError, match='set_landmarks'):
        be.transfer_latent_representation('shape')
