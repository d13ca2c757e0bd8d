"""Batched, device-resident Poisson blending (ch_poisson_blend_batch / ch_blend_mask_batch, PoissonBlender.blend_batch).

CPU: the oracle against a reference-made fixture of four stacked 64x64 cases (tests/golden/make_poisson_batch_golden.py).
GPU: the batch against that fixture (+-1 grey level, the bar of tests/test_poisson.py) and -- the main check -- against the
single-image solve: image i of a batch is BIT-IDENTICAL to PoissonBlender.__call__ on image i, iteration count included, for
ragged convergence, at 128 and 512 px, and however the batch is chunked."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

from oracle import poisson_oracle as O
from tests.test_poisson import _blender, _inputs, close_u8


def fixture():
    return np.load(os.path.join(os.path.dirname(__file__), 'golden', 'poisson_batch_golden.npz'))


def batch_inputs(S, B, seed, zero=1):
    """B seeded images (tests/test_poisson.py::_inputs) with a different ellipse each; image `zero` gets an all-zero mask.
    Returns src, tgt [B,S,S,3] and the SOLVE masks [B,S,S] (non-zero = solve) as uint8."""
    ys, xs = np.mgrid[0:S, 0:S]
    src, tgt, mask = [], [], []
    for i in range(B):
        s, t, _ = _inputs(S, seed + i)
        cy, cx, ry, rx = (0.3 + 0.08 * i) * S, (0.5 - 0.05 * i) * S, (0.28 - 0.03 * i) * S, (0.33 - 0.04 * i) * S
        hair = ((ys - cy) ** 2 / ry ** 2 + (xs - cx) ** 2 / rx ** 2 <= 1).astype(np.uint8)
        src.append(s)
        tgt.append(t)
        mask.append(np.zeros((S, S), np.uint8) if i == zero else 1 - hair)
    return np.stack(src), np.stack(tgt), np.stack(mask)


def test_fixture_shape_and_oracle_agreement():
    z = fixture()
    assert z['src'].shape == z['tgt'].shape == z['out'].shape == (4, 64, 64, 3) and z['mask'].shape == (4, 64, 64)
    names = [str(n) for n in z['names']]
    assert not z['mask'][names.index('all_zero')].any()                       # ragged convergence
    m = z['mask'][names.index('touches_border')]
    assert m[0].any() and m[:, 0].any() and not m.all()                       # solve region reaches the border
    for i, name in enumerate(names):
        out = O.poisson_blending(z['src'][i], z['tgt'][i], z['mask'][i], with_gamma=True)
        assert close_u8(out, z['out'][i], frac=0.05), name                    # same solver, same pow: near-identical


@pytest.fixture(scope='module')
def blender(hip_lib):
    return _blender()


@pytest.mark.gpu
def test_batch_matches_reference_fixture(blender):
    z = fixture()
    out = blender.blend_batch(z['src'], z['tgt'], z['mask'])
    assert out.is_cuda and out.dtype.is_floating_point is False and tuple(out.shape) == (4, 64, 64, 3)
    out = out.cpu().numpy()
    for i, name in enumerate(z['names']):
        d = np.abs(out[i].astype(int) - z['out'][i].astype(int)).max()
        print(f'{name}: max level difference {d}, iterations {blender.last_iters[i]}')
        assert close_u8(out[i], z['out'][i]), (str(name), d)
    assert all(blender.last_converged) and len(set(blender.last_iters)) > 1


def _check_bit_identity(S, B, seed, chunks=None):
    import torch
    single, batch = _blender(), _blender()
    src, tgt, mask = batch_inputs(S, B, seed)
    if chunks is not None:
        per = batch.workspace_bytes(S, S)
        batch.max_workspace_bytes = -(-B // chunks) * per + per // 2      # room for ceil(B / chunks) images, not one more
    dev = torch.device('cuda', 0)
    out = batch.blend_batch(torch.from_numpy(src).to(dev), torch.from_numpy(tgt).to(dev), torch.from_numpy(mask).to(dev))
    assert out.is_cuda and tuple(out.shape) == (B, S, S, 3)
    out = out.cpu().numpy()
    its = []
    for i in range(B):
        one = single(src[i], tgt[i], mask[i])
        its.append(single.last_iters)
        print(f'S={S} image {i}: single {single.last_iters} iterations, batch {batch.last_iters[i]}, '
              f'{int((one != out[i]).sum())} differing bytes')
        assert np.array_equal(out[i], one), i
        assert batch.last_iters[i] == single.last_iters and batch.last_converged[i] == single.last_converged, i
    assert len(set(its)) >= 2, its                                          # ragged convergence was exercised
    assert all(batch.last_converged)
    return its


@pytest.mark.gpu
def test_batch_is_bit_identical_to_single_solves_128(hip_lib):
    _check_bit_identity(128, 5, 40)


@pytest.mark.gpu
def test_batch_is_bit_identical_to_single_solves_512(hip_lib):
    _check_bit_identity(512, 2, 70)


@pytest.mark.gpu
def test_batch_is_bit_identical_when_split_into_two_chunks(hip_lib):
    _check_bit_identity(128, 5, 40, chunks=2)


@pytest.mark.gpu
def test_source_broadcast_and_numpy_inputs(blender):
    """One [H,W,3] source for the whole batch (Backend.outputs blends every render into the same photo)."""
    src, tgt, mask = batch_inputs(64, 3, 11)
    a = blender.blend_batch(src[0], tgt, mask).cpu().numpy()
    b = blender.blend_batch(np.stack([src[0]] * 3), tgt, mask[..., None]).cpu().numpy()
    assert np.array_equal(a, b)
    assert np.array_equal(a[2], blender(src[0], tgt[2], mask[2]))


@pytest.mark.gpu
def test_unconverged_images_are_reported_per_image(hip_lib):
    """max_iters = 8: image 0 (source == target, constant, everything solved: r0 = 0) is converged at once, image 1 (the
    inputs of tests/test_poisson.py::test_unconverged_solve_is_reported) is not."""
    S = 64
    ys, xs = np.mgrid[0:S, 0:S]
    disc = ((ys - 32) ** 2 + (xs - 32) ** 2 <= 20 ** 2).astype(np.uint8)
    hard_src = np.full((S, S, 3), 120, np.uint8)
    hard_src[::2] = 40
    flat = np.full((S, S, 3), 90, np.uint8)
    src, tgt = np.stack([flat, hard_src]), np.stack([flat, np.full((S, S, 3), 200, np.uint8)])
    mask = np.stack([np.ones((S, S), np.uint8), disc])
    single, batch = _blender(max_iters=8), _blender(max_iters=8)
    want_iters, want_conv, want_out = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for i in range(2):
            want_out.append(single(src[i], tgt[i], mask[i]))
            want_iters.append(single.last_iters)
            want_conv.append(single.last_converged)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        out = batch.blend_batch(src, tgt, mask).cpu().numpy()
    print('iterations', batch.last_iters, 'converged', batch.last_converged)
    assert batch.last_converged == [True, False] and want_conv == [True, False]
    assert batch.last_iters == want_iters and batch.last_iters[1] == 8
    rw = [x for x in w if issubclass(x.category, RuntimeWarning)]
    assert len(rw) == 1 and '[1]' in str(rw[0].message)
    assert np.array_equal(out[0], want_out[0]) and np.array_equal(out[1], want_out[1])


@pytest.mark.gpu
def test_blend_mask_batch_bit_exact(blender):
    rng = np.random.default_rng(3)
    for S in (64, 256):
        tps, fps = [], []
        for i in range(3):               # image 0: the inputs of tests/test_poisson.py::test_hip_blend_mask_bit_exact
            tp = rng.integers(0, 19, (S, S)).astype(np.uint8)
            tp[rng.random((S, S)) < 0.9] = 0
            fp = np.zeros((S, S), np.uint8)
            _, _, hair = _inputs(S, 9 + i)
            hair = np.roll(hair, i * S // 7, axis=0)
            tp[hair == 1] = 13
            fp[np.roll(hair, S // 10, axis=1) == 1] = 13
            tp[:, :3] = 4
            tps.append(tp)
            fps.append(fp)
        tps, fps = np.stack(tps), np.stack(fps)
        got = blender.blend_mask(tps, fps)
        assert got.is_cuda and tuple(got.shape) == (3, S, S)
        got = got.cpu().numpy()
        one = blender.blend_mask(tps, fps[1]).cpu().numpy()             # one face parsing for the whole batch
        for i in range(3):
            assert np.array_equal(got[i], O.blend_mask(tps[i], fps[i])), (S, i)
            assert np.array_equal(one[i], O.blend_mask(tps[i], fps[1])), (S, i)


@pytest.mark.gpu
def test_batch_abi_argument_errors(hip_lib):
    """Argument checks only (nothing is launched): null pointer, B = 0 and H = 2 give CH_ERR_ARG with a message and leave
    the handle usable."""
    import torch
    from ctrlhair_amd import lib as L
    ERR_ARG = 1
    h = L.Handle(0)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    p = buf.data_ptr()

    def raw(fn, *args):
        rc = getattr(h.lib, fn)(h._h, *args)
        return rc, h.lib.ch_last_error(h._h).decode()
    it = (C.c_int * 2)()
    for args in ((None, p, p, p, 2, 8, 8, 1, 10, 1e-7, it, None), (p, p, None, p, 2, 8, 8, 1, 10, 1e-7, it, None),
                 (p, p, p, None, 2, 8, 8, 1, 10, 1e-7, it, None),
                 (p, p, p, p, 0, 8, 8, 1, 10, 1e-7, it, None), (p, p, p, p, 2, 2, 8, 1, 10, 1e-7, it, None),
                 (p, p, p, p, 2, 8, 2, 1, 10, 1e-7, it, None)):
        rc, msg = raw('ch_poisson_blend_batch', *args)
        assert rc == ERR_ARG and 'ch_poisson_blend' in msg, args
    for args in ((None, p, p, 2, 8, 8, None), (p, None, p, 2, 8, 8, None), (p, p, None, 2, 8, 8, None), (p, p, p, 0, 8, 8, None)):
        rc, msg = raw('ch_blend_mask_batch', *args)
        assert rc == ERR_ARG and 'ch_blend_mask' in msg, args
    rc, _ = raw('ch_blend_mask_batch', p, p, p + 4096, 2, 8, 8, None)           # still healthy
    assert rc == 0
    torch.cuda.synchronize()
