"""Blending in the batched surface: Backend.outputs() with blending on equals the per-image postprocess_blending loop bit
for bit, and EditPipeline.edit_blended() equals the single-image PoissonBlender (bit for bit) and the CPU oracle (+-1 grey
level) on the pieces Backend.output() composes."""
import numpy as np
import pytest
import torch

from ctrlhair_amd import procedural as P
from oracle import poisson_oracle as PO

pytestmark = pytest.mark.gpu


def test_outputs_with_blending_equals_the_per_image_loop(hip_lib):
    from tests.test_backend import NGF, portrait, weights
    from ctrlhair_amd.ui.backend import Backend
    torch.manual_seed(0)
    be = Backend(2.5, blending=False, weights=weights(), device=0, max_batch=4)
    be.noise = torch.from_numpy(P.noise_planes(1, 256, NGF, seed=77)).cuda()
    be.set_input_img(portrait(3))
    values = [-1.5, 0.0, 1.5]
    plain, masks = be.sweep('shape', 0, values)
    assert len(plain) == 3 and plain[0].dtype == np.uint8 and plain[0].shape == (256, 256, 3)
    loop = [be.postprocess_blending(be.input_img, plain[i], be.input_mask, masks[i])[0] for i in range(3)]      # the old loop
    be.blending = True
    got, masks_b = be.sweep('shape', 0, values)
    assert np.array_equal(masks, masks_b) and len(got) == 3
    for i in range(3):
        d = int((got[i] != loop[i]).sum())
        print(f'image {i}: {d} bytes differ from the per-image loop; {int((got[i] != plain[i]).sum())} from the unblended image')
        assert got[i].dtype == np.uint8 and np.array_equal(got[i], loop[i]), i
        assert not np.array_equal(got[i], plain[i])
    assert isinstance(be.models.blender.last_iters, list) and len(be.models.blender.last_iters) == 3
    # an injected callable blender keeps the per-image loop
    calls = []

    def injected(face, res, mask, with_gamma=True):
        calls.append(res.shape)
        return res
    be.blender = injected
    try:
        be.sweep('shape', 0, values)
    except RuntimeError:                     # without cv2 the injected path cannot dilate: it raises, it does not batch
        pass
    else:
        assert len(calls) == 3
    be.models.generator.handle.close()


def test_edit_blended_256(hip_lib):
    from ctrlhair_amd.hair_editor import procedural_weights
    from ctrlhair_amd.pipeline import EditPipeline
    B, S, ngf = 2, 256, 16
    pipe = EditPipeline(weights=procedural_weights(0, ngf), device=0, img_size=S, max_batch=B)
    img = torch.from_numpy(P.synthetic_images(B, S, seed=21)).to(pipe.device)
    nz = torch.from_numpy(P.noise_planes(B, S, ngf, seed=22)).to(pipe.device)
    st = {}
    out = pipe.edit_blended(img, noise=nz, stages=st)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (B, S, S, 3)
    out = out.cpu().numpy()
    u8 = lambda x: (x * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().cpu().numpy()
    src, tgt = u8(img), u8(st['image'])
    labels, mask = st['labels'].cpu().numpy(), st['mask'].cpu().numpy()
    assert labels.shape == mask.shape == (B, S, S)
    blender = pipe.models.blender
    iters = list(blender.last_iters)
    for i in range(B):
        keep = blender.blend_mask(mask[i], labels[i]).cpu().numpy()
        assert np.array_equal(keep, PO.blend_mask(mask[i], labels[i]))
        one = blender(src[i], tgt[i], 1 - keep)
        assert np.array_equal(out[i], one) and blender.last_iters == iters[i], i
        ref = PO.poisson_blending(src[i], tgt[i], 1 - keep, with_gamma=True)
        d = np.abs(out[i].astype(np.int32) - ref.astype(np.int32))
        print(f'image {i}: {iters[i]} iterations, max level difference vs oracle {int(d.max())}, kept fraction {keep.mean():.3f}')
        assert d.max() <= 1, i
        assert not np.array_equal(out[i], tgt[i])
    pipe.close()
