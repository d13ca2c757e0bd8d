"""GPU tests of the ACE prologue (option sean.prologue, ctrlhair_amd/csrc/sean_model.cpp Runner::prologue, run where SeanModel::chunk_mode
says so, over the routes of Runner::plan_aces): on handles beyond the run-ahead sizes the label / code-only products of the ACEs -- hidden planes of the F(4x4)-route ACEs, gamma / beta tables, column / row sums and style
images of the gather-route ACEs -- come from grouped launches at the start of a chunk, into per-ACE buffers.  The prologue reorders launches
and moves buffers; it changes no arithmetic, so every case asserts torch.equal(sean.prologue = 1, sean.prologue = 0).

The handles are built with sean.ahead = 0: at these small sizes a default handle is an interactive one (everything runs ahead on the side
stream) and never takes the prologue.  Handles with max_batch = 3 build their style LUTs per ACE, inline, so only the label-only products and
the unstyled ACEs join the prologue there; the max_batch = 4 handles build the LUTs with the grouped GEMM at the start of the chunk and so
cover the LUT-dependent groups too (calls with B = 4: more than 64 (sample, label) columns)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NGF = 64

_handles = {}


def _pair(mb, ms, extra=()):
    """(generator with the prologue, generator without) for one handle geometry, built once per module"""
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.sean.generator import SeanGenerator
    key = (mb, ms, tuple(extra))
    if key not in _handles:
        if 'sd' not in _handles:
            _handles['sd'] = P.sean_state_dict(0, NGF)
        gens = []
        for on in (1, 0):
            opts = {'sean.ahead': 0, 'sean.prologue': on}
            opts.update(dict(extra))
            gens.append(SeanGenerator(0, f16x3=0, options=opts).load_state_dict(_handles['sd'], max_batch=mb, max_size=ms))
        _handles[key] = tuple(gens)
    return _handles[key]


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for key, v in _handles.items():
        if key != 'sd':
            for g in v:
                g.handle.close()
    _handles.clear()


def _run(gen, labels, codes, noise):
    dev = gen.device
    out = gen.generate(torch.from_numpy(labels).to(dev), torch.from_numpy(codes).to(dev), torch.from_numpy(noise).to(dev))
    torch.cuda.synchronize()
    return out


def _inputs(B, S, labels=None, seed=0):
    from ctrlhair_amd import procedural as P
    if labels is None:
        labels = P.blocky_labels(B, S, grid=8, seed=1234 + seed)
    return labels, P.style_codes(B, seed=2024 + seed), P.noise_planes(B, S, NGF, seed=7 + seed)


def _check(pair, labels, codes, noise, what):
    on, off = pair
    a, b = _run(on, labels, codes, noise), _run(off, labels, codes, noise)
    assert torch.isfinite(a).all(), what
    assert torch.equal(a, b), f'{what}: max |prologue - inline| = {float((a - b).abs().max()):.3e}'
    return a


def _face(B, S):
    from ctrlhair_amd import procedural as P
    return np.stack([P.face_like_labels(S, 40 + b) for b in range(B)])


@pytest.mark.parametrize('labels', ['blocky', 'face'])
def test_routes_at_small_size(hip_lib, labels):
    """S = 128: a gather-route level (128 pixels) above the F(4x4) levels (32 / 64 pixels)"""
    B, S = 3, 128
    lab = _face(B, S) if labels == 'face' else None
    _check(_pair(3, 128), *_inputs(B, S, lab), labels)


@pytest.mark.parametrize('labels', ['blocky', 'face'])
def test_lut_groups_and_forced_f4_route(hip_lib, labels):
    """B = 4 on a max_batch = 4 handle: the style LUTs come from the grouped GEMM, so the styled gather-route ACEs join the table and
    style-image groups; sean.wino4_force keeps the 32 / 64-pixel ACEs on the F(4x4) route whatever the task count"""
    B, S = 4, 128
    lab = _face(B, S) if labels == 'face' else None
    _check(_pair(4, 128, (('sean.wino4_force', 1),)), *_inputs(B, S, lab), labels)


def test_two_sparse_levels(hip_lib):
    B, S = 2, 256
    _check(_pair(2, 256), *_inputs(B, S), 'blocky 256')


def test_two_sparse_levels_with_grouped_luts(hip_lib):
    """the 128- and 256-pixel levels' styled ACEs in one table group and one style-image group"""
    B, S = 4, 256
    _check(_pair(4, 256), *_inputs(B, S), 'blocky 256, B = 4')


@pytest.mark.parametrize('kind', ['uniform', 'checkerboard'])
def test_empty_and_dense_extremes(hip_lib, kind):
    """uniform map: empty quad lists; 1-pixel checkerboard of two labels: every quad is a boundary quad, the patch source is off"""
    B, S = 3, 128
    if kind == 'uniform':
        lab = np.full((B, S, S), 13, np.uint8)
    else:
        lab = np.where(np.add.outer(np.arange(S), np.arange(S)) % 2 == 0, 3, 11).astype(np.uint8)
        lab = np.repeat(lab[None], B, 0)
    for pair in (_pair(3, 128), _pair(4, 128, (('sean.wino4_force', 1),))):
        _check(pair, *_inputs(B, S, lab), kind)


def test_stale_state(hip_lib):
    """two calls on one handle with different labels and codes, then the first pair again: the third result equals the first"""
    B, S = 4, 128
    pair = _pair(4, 128, (('sean.wino4_force', 1),))
    first = _inputs(B, S, seed=0)
    second = _inputs(B, S, _face(B, S), seed=5)
    r1 = _check(pair, *first, 'first').clone()
    r2 = _check(pair, *second, 'second')
    assert not torch.equal(r1, r2)
    r3 = _check(pair, *first, 'first again')
    assert torch.equal(r1, r3)


def test_handle_larger_than_the_call(hip_lib):
    """max_batch = 4, max_size = 256 called with B = 3, S = 128: every ACE sits one level below the one its buffers were sized for"""
    _check(_pair(4, 256), *_inputs(3, 128), 'B = 3, S = 128 on a 4 x 256 handle')
    _check(_pair(4, 256), *_inputs(4, 128), 'B = 4, S = 128 on a 4 x 256 handle')


def test_call_split_into_two_chunks(hip_lib):
    """Btot = 5 on a max_batch = 3 handle: chunks of 3 and 2 samples"""
    _check(_pair(3, 128), *_inputs(5, 128), 'Btot = 5')
    _check(_pair(4, 128, (('sean.wino4_force', 1),)), *_inputs(7, 128), 'Btot = 7 on max_batch = 4')


def test_absent_regions(hip_lib):
    """label maps that lack most of the 19 regions: the styled ACEs' LUT rows of absent labels"""
    B, S = 4, 128
    lab = _inputs(B, S)[0] % 4
    lab[1] = 18
    for pair, b in ((_pair(3, 128), 3), (_pair(4, 128, (('sean.wino4_force', 1),)), 4)):
        _check(pair, *_inputs(b, S, lab[:b].copy()), 'absent regions')
