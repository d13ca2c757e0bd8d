"""Matte paste-back on the HIP library (csrc/face_matte.hip, ch_face_unalign_matte) against the float64 oracle of
tests/matte_oracle.py, on the cases of tests/matte_cases.py.

alpha: the 13 window moments are exact integers on both sides and the solve is float64 on both sides, so the two differ by float64
rounding amplified by the 3 x 3 system's condition number (<= 0.25 / eps) and by one float32 rounding of a, b and m: the CPU
prototype of that arithmetic is within 2e-6 of float64.  The condition is half a grey level of alpha, 1 / 510.
Composite: the resample is ch_face_unalign's float32 one, so its bound holds: every pixel within one grey level, at most 2 % of the
pixels inside bbox different."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import matte_cases as MC
from tests import unalign_cases as UC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def aligner():
    from ctrlhair_amd.alignment import FaceAligner
    return FaceAligner(device='cuda:0')


def _run(aligner, name, **over):
    c = dict(MC.inputs(name), **over)
    out, alpha = aligner.paste_back(c['photo'], c['edits'], c['plan_u'], weight=c['weight'], feather=c['feather'],
                                    matte={'radius': c['radius'], 'eps': c['eps']}, return_alpha=True)
    torch.cuda.synchronize()
    return out.cpu().numpy(), alpha.cpu().numpy()


@pytest.mark.parametrize('name', sorted(MC.CASES))
def test_against_oracle(aligner, name):
    c = MC.inputs(name)
    got, alpha = _run(aligner, name)
    x0, y0, x1, y1 = c['plan_u']['bbox']
    assert got.shape == (c['edits'].shape[0],) + c['photo'].shape and got.dtype == np.uint8
    assert alpha.shape == (y1 - y0, x1 - x0) and alpha.dtype == np.float32
    r = MC.compare(name, got, alpha)
    print(f'{name}: max |alpha - oracle| {r["alpha_max"]:.3e}, composite max {r["max"]}, share of differing pixels inside bbox '
          f'{100 * r["share"]:.4f} %')
    assert r['alpha_max'] <= 1.0 / 510.0
    assert r['zero_set_equal'], 'alpha == 0 on a different set than the oracle'
    assert r['photo_kept'], 'a pixel outside bbox or with alpha == 0 differs from the photo'
    assert r['max'] <= 1
    assert r['share'] <= 0.02
    assert (got != c['photo'][None]).any(), 'nothing was pasted'
    assert 0.0 <= alpha.min() and alpha.max() <= 1.0


@pytest.mark.parametrize('name', ['e_batch_feather-r3-eps0.0001', 'e_batch_feather-r64-eps0.0001', 'f_origin-r8-eps0.01'])
def test_batch_equals_single_calls_and_runs_repeat(aligner, name):
    c = MC.inputs(name)
    got, alpha = _run(aligner, name)
    again, alpha_again = _run(aligner, name)
    assert np.array_equal(got, again) and np.array_equal(alpha, alpha_again), 'two runs of one call differ'
    for n in range(c['edits'].shape[0]):
        one, alpha_one = _run(aligner, name, edits=c['edits'][n])
        assert one.shape[0] == 1 and np.array_equal(one[0], got[n]), f'image {n} of the batch differs from its N = 1 call'
        assert np.array_equal(alpha_one, alpha)


@pytest.mark.parametrize('S,scale,side', [(32, 0.4, 80), (80, 2.0, 40), (64, 0.25, 256)])
def test_full_weight_hard_edge_equals_plain_paste_back(aligner, S, scale, side):
    """Weight all 255, feather <= 0: m == 1 exactly (a constant weight is reproduced exactly), alpha = ramp = 1, and the output is
    ch_face_unalign's with the same weight, byte for byte.  The premise needs p8 = 255 on all of D, so the plan is an axis-aligned
    quad on whole photo pixels (every pixel centre of bbox inside the quad); in the rotated plans of matte_cases the corners of
    bbox lie outside the quad, where p8 = 0 by the specification.  side = 256 takes more than one strip and segment."""
    from tests import align_oracle as AO
    ox, oy = 11, 6
    photo = AO.make_photo(51, side + 23, side + 30)
    edits = np.stack([AO.make_photo(52 + n, S, S) for n in range(2)])
    A = np.array([[scale, 0.0, -scale * ox], [0.0, scale, -scale * oy]])
    pu = {'A': A, 'bbox': (ox, oy, ox + side, oy + side), 'scale': scale, 'output_size': S}
    assert S == scale * side
    w = np.full((S, S), 255, np.uint8)
    for r in (1, 5, 64):
        got, alpha = aligner.paste_back(photo, edits, pu, weight=w, feather=0.0, matte={'radius': r, 'eps': 1e-4}, return_alpha=True)
        plain = aligner.paste_back(photo, edits, pu, weight=w, feather=0.0)
        torch.cuda.synchronize()
        assert (alpha.cpu().numpy() == 1.0).all()
        assert np.array_equal(got.cpu().numpy(), plain.cpu().numpy())


def test_matte_none_is_the_plain_call(aligner):
    from ctrlhair_amd import alignment as AL
    for name in ('e_batch_feather', 'f_origin'):
        c = UC.inputs(name)
        got = aligner.paste_back(c['photo'], c['edits'], c['plan_u'], weight=c['weight'], feather=c['feather'], matte=None)
        dp, de = torch.from_numpy(c['photo']).cuda(), torch.from_numpy(c['edits']).cuda()
        dw = None if c['weight'] is None else torch.from_numpy(c['weight']).cuda()
        H, W = c['photo'].shape[:2]
        out = torch.empty(de.shape[0], H, W, 3, dtype=torch.uint8, device='cuda')
        pv, pp = aligner._f64(AL.pack_unalign(c['plan_u']))
        aligner.handle.call('ch_face_unalign', dp.data_ptr(), H, W, de.data_ptr(), int(de.shape[0]), None if dw is None else dw.data_ptr(),
                            pp, float(c['feather']), out.data_ptr(), aligner._stream())
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), out.cpu().numpy())
        assert np.array_equal(got.cpu().numpy(), aligner.paste_back(c['photo'], c['edits'], c['plan_u'], weight=c['weight'],
                                                                    feather=c['feather']).cpu().numpy())
    with pytest.raises(ValueError, match='weight'):
        aligner.paste_back(c['photo'], c['edits'], c['plan_u'], matte=True)


def test_abi_rejects_bad_arguments(aligner):
    """radius 0 and 65, eps 0 and NaN, a null weight and a workspace one byte short return CH_ERR_ARG with a message naming the
    entry, and nothing is launched: out and alpha keep their sentinel bytes."""
    from ctrlhair_amd import alignment as AL
    c = MC.inputs('e_batch_feather-r3-eps0.0001')
    H, W = c['photo'].shape[:2]
    x0, y0, x1, y1 = c['plan_u']['bbox']
    dp, de, dw = (torch.from_numpy(c[k]).cuda() for k in ('photo', 'edits', 'weight'))
    N = int(de.shape[0])
    pv, pp = aligner._f64(AL.pack_unalign(c['plan_u']))
    lib, h = aligner.handle.lib, aligner.handle._h
    need = int(lib.ch_face_unalign_matte_workspace_bytes(H, W, pp, 3))
    assert need >= 21 * (x1 - x0) * (y1 - y0) and need % 256 == 0
    assert lib.ch_face_unalign_matte_workspace_bytes(H, W, pp, 0) == 0 and lib.ch_face_unalign_matte_workspace_bytes(H, W, pp, 65) == 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    out = torch.full((N, H, W, 3), 7, dtype=torch.uint8, device='cuda')
    alpha = torch.full((y1 - y0, x1 - x0), -3.0, dtype=torch.float32, device='cuda')

    def call(radius=3, eps=1e-4, weight=dw.data_ptr(), ws_ptr=ws.data_ptr(), ws_bytes=need):
        return lib.ch_face_unalign_matte(h, dp.data_ptr(), H, W, de.data_ptr(), N, weight, pp, float(c['feather']), radius, eps,
                                         out.data_ptr(), alpha.data_ptr(), ws_ptr, ws_bytes, aligner._stream())

    bad = [dict(radius=0), dict(radius=65), dict(eps=0.0), dict(eps=float('nan')), dict(eps=float('inf')), dict(eps=-1e-4),
           dict(weight=None), dict(ws_bytes=need - 1), dict(ws_ptr=None), dict(ws_ptr=ws.data_ptr() + 16)]
    for kw in bad:
        assert call(**kw) == 1, kw                   # CH_ERR_ARG
        assert b'ch_face_unalign_matte' in lib.ch_last_error(h), kw
    torch.cuda.synchronize()
    assert (out == 7).all() and (alpha == -3.0).all(), 'a rejected call launched something'
    assert call() == 0
    torch.cuda.synchronize()
    ref, ref_alpha = _run(aligner, 'e_batch_feather-r3-eps0.0001')
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(alpha.cpu().numpy(), ref_alpha)
    with pytest.raises(ValueError):
        aligner.paste_back(c['photo'], c['edits'], c['plan_u'], weight=c['weight'], matte={'radius': 65})


def test_backend_outputs_in_photo_hair_matte():
    """Backend.outputs_in_photo(region='hair', matte=True) on procedural weights equals outputs() followed by paste_back with the
    undilated hair union and matte=True, bit for bit; region='crop' with a matte raises."""
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.hair_editor import procedural_weights
    from ctrlhair_amd.hostutil import HAIR_IDX
    from ctrlhair_amd.ui.backend import Backend
    from tests import align_oracle as AO
    ngf = 16                                       # a tiny SEAN generator; the other networks are full size
    w = procedural_weights(0, 64)
    w['sean'] = P.sean_state_dict(0, ngf)
    torch.manual_seed(0)
    be = Backend(2.5, blending=False, weights=w, device=0, max_batch=2)
    photo = AO.make_photo(41, 420, 380)
    lm = AO.make_landmarks(141, (190.0, 180.0), 50.0, 9.0)
    crop = be.crop_face(photo, landmarks=lm)
    be.noise = torch.from_numpy(P.noise_planes(1, 256, ngf, seed=77)).cuda()
    be.set_input_img(crop)
    lat = [be.copy_latent(), be.copy_latent()]
    lat[1].curliness = lat[1].curliness + 0.7
    got, masks = be.outputs_in_photo(lat, region='hair', matte=True)
    imgs, masks2 = be.outputs(lat)
    union = (np.asarray(masks2) == HAIR_IDX).any(axis=0) | (np.asarray(be.input_mask).reshape(256, 256) == HAIR_IDX)
    weight = be._region_weight('hair', masks2, True)
    assert weight.shape == (256, 256) and weight.dtype == torch.uint8 and weight.is_cuda
    assert np.array_equal(weight.cpu().numpy(), union.astype(np.uint8) * 255), 'the matte weight is the undilated hair union'
    dilated = be._region_weight('hair', masks2).cpu().numpy()
    assert (dilated >= weight.cpu().numpy()).all()
    want = be.paste_back(np.stack(imgs), weight=weight, matte=True)
    assert got.shape == (2, 420, 380, 3) and np.array_equal(masks, masks2)
    assert np.array_equal(got.cpu().numpy(), want.cpu().numpy())
    one = be.output_in_photo(region='hair', matte={'radius': 2})
    assert one.shape == (420, 380, 3)
    with pytest.raises(ValueError, match="region='hair'"):
        be.outputs_in_photo(lat, region='crop', matte=True)
    with pytest.raises(ValueError, match="region='hair'"):
        be.output_in_photo(region='crop', matte=True)
    with pytest.raises(ValueError, match="'crop' or 'hair'"):
        be.outputs_in_photo(lat, region='face', matte=True)
