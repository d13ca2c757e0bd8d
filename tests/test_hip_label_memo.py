"""GPU tests of the label memo (option sean.label_memo, ctrlhair_amd/csrc/sean_model.h SeanModel::memo_state): on handles with the ACE
prologue a call of one chunk compares its label maps with the handle's copy on the device, and the launches that build label-only products
return at once when the maps, the shapes and the options are those of the chunk before.  The memo skips work; it changes no arithmetic, so
every output is compared with np.array_equal against a second handle built with sean.label_memo = 0 and fed the same calls, and the
(calls, hits) counters of the memo handle are asserted call by call.

ngf = 16, max_batch = 3, max_size = 128, sean.ahead = 0 (small chunks in prologue mode, as tools/level_plan_digest.py builds them): the
128-pixel level takes the unstyled gather route, 64 and 32 pixels the F(4x4) route, 16 pixels and below the head block.  One case runs at
max_size = 256, B = 2 (a styled gather level).  The handles are shared by the module, so every test brings label maps no test before it
used (its own seeds) and counts from the counters it finds.

The option-change case toggles sean.sparse, not sean.edge: sean.edge is frozen by ch_finalize (tests/test_abi_errors.py), sean.sparse
is the live key that changes a label-derived product (without it every quad of a gather level is a boundary quad)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NGF = 16
_handles = {}


def _pair(mb=3, ms=128):
    """(generator with the memo, reference generator without) for one handle geometry, built once per module"""
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.sean.generator import SeanGenerator
    key = (mb, ms)
    if key not in _handles:
        sd = P.sean_state_dict(0, NGF)
        _handles[key] = tuple(SeanGenerator(0, f16x3=0, options={'sean.ahead': 0, 'sean.label_memo': on}).load_state_dict(sd, max_batch=mb, max_size=ms)
                              for on in (1, 0))
    return _handles[key]


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for v in _handles.values():
        for g in v:
            g.handle.close()
    _handles.clear()


def _labels(kind, B, S, seed):
    from ctrlhair_amd import procedural as P
    if kind == 'dense':          # one label per pixel: the boundary quads overflow the patch buffer, the level runs in plane mode
        return np.random.default_rng(seed).integers(0, 19, size=(B, S, S), dtype=np.uint8)
    lab = P.blocky_labels(B, S, grid=8, seed=seed)      # cells of S / 8 pixels: few boundary quads, pre-gathered patches
    if kind == 'uniform':        # one sample without a boundary quad
        lab[1] = 5
    return lab


def _inputs(B, S, seed):
    from ctrlhair_amd import procedural as P
    return P.style_codes(B, seed=2024 + seed), P.noise_planes(B, S, NGF, seed=7 + seed)


def _dev(gen, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gen.device) for a in arrays]


def _call(pair, labels, seed, what):
    """one generate() on both handles from host arrays; asserts equal images; returns whether the memo handle counted a hit"""
    memo, ref = pair
    B, S = labels.shape[0], labels.shape[-1]
    codes, noise = _inputs(B, S, seed)
    c0, h0 = memo.handle.sean_label_memo_stats()
    a = memo.generate(*_dev(memo, labels, codes, noise))
    b = ref.generate(*_dev(ref, labels, codes, noise))
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.isfinite(a).all(), what
    assert np.array_equal(a, b), f'{what}: max |memo - reference| = {float(np.abs(a - b).max()):.3e}'
    c1, h1 = memo.handle.sean_label_memo_stats()
    assert ref.handle.sean_label_memo_stats() == (0, 0), 'the reference handle has no memo'
    return c1 - c0, h1 - h0


@pytest.mark.parametrize('kind', ['blocky', 'dense', 'uniform'])
def test_repeat(hip_lib, kind):
    """labels L with codes c1, c2, c3: the second and third call hit"""
    pair = _pair()
    L = _labels(kind, 3, 128, {'blocky': 11, 'dense': 12, 'uniform': 13}[kind])
    got = [_call(pair, L, seed, f'{kind}, call {seed}') for seed in (1, 2, 3)]
    assert got == [(1, 0), (1, 1), (1, 1)], got


def test_repeat_256(hip_lib):
    """B = 2 at 256 pixels: a styled gather level (128 pixels) below the unstyled one"""
    pair = _pair(2, 256)
    L = _labels('blocky', 2, 256, 21)
    got = [_call(pair, L, seed, f'256, call {seed}') for seed in (1, 2, 3)]
    assert got == [(1, 0), (1, 1), (1, 1)], got


@pytest.mark.parametrize('where', ['middle', 'border'])
def test_change_and_return(hip_lib, where):
    """L, L', L, L', L' with L' = L but for one pixel of the last sample: only the last call hits (the copy follows every change)"""
    pair = _pair()
    L = _labels('blocky', 3, 128, 31 if where == 'middle' else 32)
    y, x = (8, 8) if where == 'middle' else (15, 40)      # cells of 16 pixels: the middle of a cell / its last row, above another cell
    L2 = L.copy()
    L2[2, y, x] = (L[2, y, x] + 1) % 19
    got = [_call(pair, lab, seed, f'{where}, call {seed}') for seed, lab in enumerate((L, L2, L, L2, L2))]
    assert got == [(1, 0)] * 4 + [(1, 1)], got


def test_in_place(hip_lib):
    """one label tensor, overwritten between the calls: no hit"""
    memo, ref = pair = _pair()
    L, L2 = _labels('blocky', 3, 128, 41), _labels('blocky', 3, 128, 42)
    codes, noise = _inputs(3, 128, 4)
    outs = []
    for g in pair:
        lab, c, n = _dev(g, L, codes, noise)
        h0 = g.handle.sean_label_memo_stats()[1]
        o = [g.generate(lab, c, n).cpu().numpy()]
        lab.copy_(torch.from_numpy(L2).to(g.device))
        o.append(g.generate(lab, c, n).cpu().numpy())
        o.append(g.generate(lab, c, n).cpu().numpy())
        outs.append(o)
        if g is memo:
            assert g.handle.sean_label_memo_stats()[1] - h0 == 1      # (the third call only)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert not np.array_equal(outs[0][0], outs[0][1])


def test_shape(hip_lib):
    """B = 3, 2, 3 and S = 128, 64, 128 on one handle: no hit across a change of shape, a hit on the repeat that follows"""
    pair = _pair()
    L = _labels('blocky', 3, 128, 51)
    L64 = np.ascontiguousarray(L[:, ::2, ::2])
    seq = [(L, 0), (L[:2], 0), (L, 0), (L, 1), (L64, 0), (L64, 1), (L, 0), (L, 1)]
    for i, (lab, hit) in enumerate(seq):
        assert _call(pair, lab, i, f'shape, call {i}') == (1, hit), i


def test_two_chunks(hip_lib):
    """Btot = 4 on the max_batch = 3 handle goes in two chunks and is not memoized; the call of its first three samples that follows misses"""
    pair = _pair()
    L = _labels('blocky', 4, 128, 61)
    assert _call(pair, L[:3], 0, 'three samples') == (1, 0)
    assert _call(pair, L, 1, 'four samples') == (0, 0)
    assert _call(pair, L[:3], 2, 'three samples again') == (1, 0)
    assert _call(pair, L[:3], 3, 'and again') == (1, 1)


def test_option_change(hip_lib):
    """ch_set_option between two calls with equal labels: no hit, the output follows the option (the reference handle takes the same key)"""
    pair = _pair()
    L = _labels('blocky', 3, 128, 71)
    try:
        assert _call(pair, L, 0, 'before') == (1, 0)
        for g in pair:
            g.handle.set_option('sean.sparse', 0)
        assert _call(pair, L, 1, 'sean.sparse = 0') == (1, 0)
        assert _call(pair, L, 2, 'sean.sparse = 0, repeat') == (1, 1)
    finally:
        for g in pair:
            g.handle.set_option('sean.sparse', 1)
    assert _call(pair, L, 3, 'sean.sparse = 1 again') == (1, 0)
    assert _call(pair, L, 4, 'repeat') == (1, 1)


def test_interleaved_encode(hip_lib):
    """encode() between two equal generate() calls writes none of the memoized buffers: the second call hits"""
    pair = _pair()
    from ctrlhair_amd import procedural as P
    L = _labels('blocky', 3, 128, 81)
    assert _call(pair, L, 0, 'before encode') == (1, 0)
    img = P.synthetic_images(3, 128)
    codes = [g.encode(*_dev(g, img, L)).cpu().numpy() for g in pair]
    assert np.array_equal(*codes)
    got = _call(pair, L, 1, 'after encode')
    print('hits of the call after encode():', got[1])
    assert got == (1, 1)


def test_graph(hip_lib):
    """capture once (warm-up call + capture), replay with the captured labels, with other labels refilled in place, and once more"""
    memo, ref = _pair()
    L, L2 = _labels('blocky', 3, 128, 91), _labels('uniform', 3, 128, 92)
    codes, noise = _inputs(3, 128, 9)
    lab, c, n = _dev(memo, L, codes, noise)
    c0, h0 = memo.handle.sean_label_memo_stats()
    g, out = memo.capture(lab, c, n)
    got = []
    for labels in (L, L2, L2):
        lab.copy_(torch.from_numpy(labels).to(memo.device))
        g.replay()
        torch.cuda.synchronize()
        got.append(out.cpu().numpy())
    c1, h1 = memo.handle.sean_label_memo_stats()
    assert (c1 - c0, h1 - h0) == (4, 2)      # warm-up: miss; replays: hit, miss, hit
    for labels, a in zip((L, L2, L2), got):
        b = ref.generate(*_dev(ref, labels, codes, noise)).cpu().numpy()
        assert np.array_equal(a, b)
    del g


def test_off_switch(hip_lib):
    """sean.label_memo = 0: nothing is counted"""
    _, ref = _pair()
    L = _labels('blocky', 3, 128, 95)
    codes, noise = _inputs(3, 128, 0)
    for _ in range(2):
        ref.generate(*_dev(ref, L, codes, noise))
    assert ref.handle.sean_label_memo_stats() == (0, 0)
