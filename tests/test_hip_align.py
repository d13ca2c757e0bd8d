"""Face alignment on the HIP library (csrc/face_align.hip): every stage bit-exact against Pillow / numpy / scipy (tests/align_oracle.py),
the composite call against the crops the reference recorded (tests/golden/align_golden.npz), the public paths, the ABI's argument
errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from ctrlhair_amd import alignment as A
from tests import align_oracle as O
from tests.test_alignment import check_crop, golden, plan_of      # noqa: F401  (golden is a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def aligner(hip_lib):
    from ctrlhair_amd import lib
    return A.FaceAligner(lib.Handle(0), torch.device('cuda', 0))


def same(name, got, want):
    got = got.cpu().numpy() if hasattr(got, 'cpu') else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    diff = np.abs(got.astype(int) - want.astype(int))
    print(f'{name}: {int((diff > 0).sum())} of {diff.size} values differ, max {int(diff.max())}')
    assert np.array_equal(got, want)


@pytest.mark.parametrize('src,dst,ch', [((64, 64), (16, 16), 3), ((301, 517), (97, 211), 3), ((517, 301), (512, 40), 3),
                                        ((128, 96), (300, 200), 3), ((4096, 48), (256, 48), 3), ((40, 4096), (40, 256), 3),
                                        ((233, 177), (100, 59), 1), ((120, 131), (57, 64), 4), ((2400, 1800), (1200, 900), 3)])
def test_resample_equals_pillow(aligner, src, dst, ch):
    """(H, W) -> (h, w): down, up, mixed, one axis unchanged, 97 taps (4096 -> 256), non-square, 1 / 3 / 4 channels."""
    rng = np.random.default_rng(src[0] * 7 + dst[1])
    img = rng.integers(0, 256, (src[0], src[1], ch), dtype=np.uint8)
    if ch == 4:          # four plain channels: CMYK (an RGBA image would be resized with premultiplied alpha)
        from PIL import Image
        pil = Image.frombytes('CMYK', (src[1], src[0]), img.tobytes())
        want = np.asarray(pil.resize((dst[1], dst[0]), Image.LANCZOS))
    else:
        want = O.resize(img[..., 0] if ch == 1 else img, (dst[1], dst[0])).reshape(dst[0], dst[1], ch)
    same(f'resample {src}->{dst}x{ch}', aligner.resample(img, (dst[1], dst[0])), want)


def test_resample_extremes_clip(aligner):
    """A checkerboard of 0 / 255 overshoots on both sides: the 8-bit clip."""
    img = np.zeros((90, 120, 3), np.uint8)
    img[::2, 1::2] = 255
    img[1::2, ::2] = 255
    img[30:60, 40:80] = 255
    same('clip', aligner.resample(img, (77, 41)), O.resize(img, (77, 41)))


@pytest.mark.parametrize('name', list(O.CASES))
def test_quad_warp_equals_pillow_on_the_fixture_quads(aligner, name):
    photo, lm, plan = plan_of(name)
    stages = {}
    want = O.run_plan(photo, plan, stages)
    same(f'quad {name}', aligner.quad_warp(stages['source'], plan['quad'] + 0.5, plan['transform_size'], plan['output_size']), want)


def test_quad_warp_zero_fill_and_direct_output(aligner):
    """A quad that leaves the source on two sides (zero fill, clipped neighbours, the last-row rule), reduced and at
    output_size == transform_size."""
    photo = O.make_photo(21, 300, 260)
    corners = np.array([[-40.3, -25.7], [-12.0, 330.2], [250.5, 290.0], [215.25, 10.5]])
    for T, S in ((1024, 256), (512, 512), (768, 100)):
        want = O.quad_warp(photo, corners, T, S)
        assert (want[0, 0] == 0).all()                     # the NW corner lies outside
        same(f'zero fill {T}->{S}', aligner.quad_warp(photo, corners, T, S), want)


@pytest.mark.parametrize('name', [n for n in O.CASES if 'pad' in n])
def test_padding_branch_equals_the_oracle(aligner, name):
    photo, lm, plan = plan_of(name)
    stages = {}
    O.run_plan(photo, plan, stages)
    src = stages.get('cropped', stages.get('shrunk', photo))
    same(f'pad {name}', aligner.pad_feather(src, plan['pad'], plan['blur']), stages['padded'])


def test_padding_branch_odd_pixel_count(aligner):
    """An odd pixel count: the median is one element, not the mean of two."""
    photo = O.make_photo(22, 41, 37)
    assert ((41 + 9 + 11) * (37 + 8 + 12)) % 2 == 1
    qsize = 125.0
    same('pad odd', aligner.pad_feather(photo, (8, 9, 12, 11), qsize * 0.02), O.pad_feather(photo, (8, 9, 12, 11), qsize))


@pytest.mark.parametrize('name', list(O.CASES))
def test_composite_equals_the_reference_crop(aligner, golden, name):      # noqa: F811
    photo, lm, S, T = O.case_inputs(name)
    crop, pts = aligner.align(photo, lm, S, transform_size=T)
    assert crop.is_cuda and crop.dtype == torch.uint8
    check_crop(golden, name, crop.cpu().numpy())
    assert pts.dtype == np.int32 and np.array_equal(pts, golden[f'{name}/landmarks'])
    again, _ = aligner.align(torch.from_numpy(photo).cuda(), lm, S, transform_size=T)
    assert torch.equal(crop, again)


def test_crop_face_and_backend_landmarker(aligner, golden):      # noqa: F811
    from ctrlhair_amd.ui.backend import Backend
    from tests.test_backend import weights
    photo, lm, S, T = O.case_inputs('plain_256')
    be = Backend(2.5, blending=False, weights=weights(), device=0)
    assert isinstance(be.models.aligner, A.FaceAligner)
    with pytest.raises(NotImplementedError):
        be.crop_face(photo)
    out = be.crop_face(photo, landmarks=lm)
    check_crop(golden, 'plain_256', out)
    seen = []

    def landmarker(img):
        seen.append(img.shape)
        return np.concatenate([lm, np.zeros((13, 2))])
    be2 = Backend(2.5, blending=False, models=be.models, landmarker=landmarker)
    check_crop(golden, 'plain_256', be2.crop_face(photo))
    assert seen == [photo.shape]


def test_crop_job_writes_the_reference_crop(tmp_path, golden):      # noqa: F811
    from PIL import Image
    photo, lm, S, T = O.case_inputs('pad_topleft_512')
    src = tmp_path / 'src'
    src.mkdir()
    Image.fromarray(photo).save(src / 'a.png')
    Image.fromarray(photo).save(src / 'b.png')
    np.savez(tmp_path / 'lm.npz', **{'a.png': lm})
    r = subprocess.run([sys.executable, '-m', 'ctrlhair_amd.dataset', 'crop', str(src), str(tmp_path), 'ds', '--landmarks',
                        str(tmp_path / 'lm.npz'), '--size', '256'], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert 'no landmarks for b.png' in r.stdout and '1 files, 1 without landmarks' in r.stdout
    out_dir = tmp_path / 'ds' / 'images_256'
    assert os.listdir(out_dir) == ['a.png']
    plan = A.align_plan(lm, photo.shape[0], photo.shape[1], 256)
    assert np.array_equal(np.asarray(Image.open(out_dir / 'a.png')), O.run_plan(photo, plan))


def test_abi_argument_errors(aligner):
    h = aligner.handle
    lib, hp = h.lib, h._h
    img = torch.zeros(32, 32, 3, dtype=torch.uint8, device='cuda')
    out = torch.zeros(64, 64, 3, dtype=torch.uint8, device='cuda')
    ws = torch.zeros(32 << 20, dtype=torch.uint8, device='cuda')
    coef = np.array([0, 1, 0, 0, 0, 0, 1, 0], np.float64)
    cp = coef.ctypes.data_as(C.c_void_p)

    def err():
        return lib.ch_last_error(hp).decode()
    # resample: null pointer, non-positive size, channel count, small workspace
    assert lib.ch_resample_lanczos_u8(hp, None, 32, 32, 3, out.data_ptr(), 16, 16, ws.data_ptr(), ws.numel(), None) != 0
    assert 'ch_resample_lanczos_u8' in err()
    assert lib.ch_resample_lanczos_u8(hp, img.data_ptr(), 32, 0, 3, out.data_ptr(), 16, 16, ws.data_ptr(), ws.numel(), None) != 0
    assert lib.ch_resample_lanczos_u8(hp, img.data_ptr(), 32, 32, 5, out.data_ptr(), 16, 16, ws.data_ptr(), ws.numel(), None) != 0
    assert lib.ch_resample_lanczos_u8(hp, img.data_ptr(), 32, 32, 3, out.data_ptr(), 16, 16, ws.data_ptr(), 16, None) != 0
    assert 'workspace' in err()
    assert lib.ch_resample_lanczos_workspace_bytes(32, 32, 3, 0, 16) == 0
    # quad warp
    assert lib.ch_quad_warp_resample_u8(hp, img.data_ptr(), 32, 32, None, 64, 64, out.data_ptr(), ws.data_ptr(), ws.numel(), None) != 0
    assert lib.ch_quad_warp_resample_u8(hp, img.data_ptr(), 32, 32, cp, 64, 128, out.data_ptr(), ws.data_ptr(), ws.numel(), None) != 0
    assert lib.ch_quad_warp_resample_u8(hp, img.data_ptr(), 32, 32, cp, 1 << 20, 64, out.data_ptr(), ws.data_ptr(), ws.numel(), None) != 0
    assert lib.ch_quad_warp_resample_u8(hp, img.data_ptr(), 32, 32, cp, 128, 64, out.data_ptr(), ws.data_ptr(), 8, None) != 0
    assert 'workspace' in err()
    nan = np.array([np.nan] * 8)
    assert lib.ch_quad_warp_resample_u8(hp, img.data_ptr(), 32, 32, nan.ctypes.data_as(C.c_void_p), 128, 64, out.data_ptr(), ws.data_ptr(),
                                        ws.numel(), None) != 0
    assert 'finite' in err()
    # pad / feather
    w, r = A.gaussian_weights(1.0)
    wp = w.ctypes.data_as(C.c_void_p)
    pads = np.array([4, 4, 4, 4], np.int32)
    zero = np.array([4, 0, 4, 4], np.int32)
    big = torch.zeros(40, 40, 3, dtype=torch.uint8, device='cuda')
    assert lib.ch_align_pad_feather_u8(hp, img.data_ptr(), 32, 32, zero.ctypes.data_as(C.c_void_p), wp, r, big.data_ptr(), ws.data_ptr(),
                                       ws.numel(), None) != 0
    assert lib.ch_align_pad_feather_u8(hp, img.data_ptr(), 32, 32, pads.ctypes.data_as(C.c_void_p), None, r, big.data_ptr(), ws.data_ptr(),
                                       ws.numel(), None) != 0
    assert lib.ch_align_pad_feather_u8(hp, img.data_ptr(), 32, 32, pads.ctypes.data_as(C.c_void_p), wp, r, big.data_ptr(), ws.data_ptr(),
                                       64, None) != 0
    assert 'workspace' in err()
    # composite: inconsistent plans
    photo, lm, S, T = O.case_inputs('plain_256')
    plan = A.pack_plan(A.align_plan(lm, 900, 800, 64, 256))
    src = torch.zeros(900, 800, 3, dtype=torch.uint8, device='cuda')

    def run(p, H=900, W=800, wsn=None, s=src.data_ptr()):
        p = np.ascontiguousarray(p, np.float64)
        return lib.ch_face_align(hp, s, H, W, p.ctypes.data_as(C.c_void_p), None, 0, out.data_ptr(), ws.data_ptr(),
                                 ws.numel() if wsn is None else wsn, None)
    need = lib.ch_face_align_workspace_bytes(900, 800, plan.ctypes.data_as(C.c_void_p), 0)
    assert 0 < need <= ws.numel()
    assert run(plan) == 0, err()
    assert run(plan, s=None) != 0
    assert run(plan, H=0) != 0
    assert run(plan, wsn=128) != 0 and 'workspace' in err()
    for idx, val in ((5, 801.0), (3, -1.0), (21, 512.0), (20, 1e7), (12, np.inf), (4, 0.5), (1, 799.0)):
        bad = plan.copy()
        bad[idx] = val
        assert run(bad) != 0, idx
        assert 'ch_face_align' in err()
    padded = plan.copy()
    padded[7:12] = (1, 5, 5, 5, 5)
    assert run(padded) != 0 and 'gauss_w' in err()
    torch.cuda.synchronize()
