"""GPU tests of the SPADE memo (option sean.spade_memo, ctrlhair_amd/csrc/sean_model.h SeanModel::memo_acc, conv_wino4v.h): the styled
ACEs on the F(4x4) V route keep the Winograd-domain accumulators of every task after the 32 hidden k-steps; the label memo's decision
kernel sets the mode of a call -- PLAIN on a label miss, STORE on the first hit of a label set, LOAD from the second hit on.  Every
accumulator receives the same MFMAs in the same order in all three, so every output is compared with np.array_equal against a second
handle built with sean.label_memo = 0 and fed the same calls, and the (stores, loads) counters and the label memo's (calls, hits) are
asserted call by call.

ngf = 32, max_batch = 2, max_size = 256, sean.ahead = 0: the smallest geometry with V-route styled ACEs at both level sizes -- up_0 at
32 pixels (C = 512 / 512 / 256, one spatial tile per sample) and up_1 at 64 pixels (C = 256 / 256: 512 GEMM rows, two spatial tiles per
side).  Both handles also take sean.wino4_force = 1: with two samples these launches have fewer tasks than the device has CUs, where
SeanModel::ace_route hands an F(4x4) ACE to the gather kernel, and the memo would never run; the key forces the F(4x4) kernels wherever
the shape allows, on the reference handle as well.  The handles are shared by the module, so every test brings label maps no test
before it used and counts from the counters it finds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NGF = 32
PLAIN, STORE, LOAD = (1, 0, 0, 0), (1, 1, 1, 0), (1, 1, 0, 1)      # (calls, hits, stores, loads) one call adds
_handles = {}


def _build(ngf, mb, ms, **opts):
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.sean.generator import SeanGenerator
    options = {'sean.ahead': 0, 'sean.wino4_force': 1}
    options.update(opts)
    # (the committed calibration table holds ngf = 16 and 64 only: ngf = 32 runs with the identity running statistics)
    sd = P.sean_state_dict(0, ngf, calibrated=ngf != NGF)
    return SeanGenerator(0, f16x3=0, options=options).load_state_dict(sd, max_batch=mb, max_size=ms)


def _pair():
    """(generator with both memos, reference generator without the label memo), built once per module"""
    if 'pair' not in _handles:
        _handles['pair'] = (_build(NGF, 2, 256), _build(NGF, 2, 256, **{'sean.label_memo': 0}))
    return _handles['pair']


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for v in _handles.values():
        for g in v:
            g.handle.close()
    _handles.clear()


def _labels(B, S, seed):
    from ctrlhair_amd import procedural as P
    return P.blocky_labels(B, S, grid=8, seed=seed)


def _inputs(B, S, seed, ngf=NGF):
    from ctrlhair_amd import procedural as P
    return P.style_codes(B, seed=2024 + seed), P.noise_planes(B, S, ngf, seed=7 + seed)


def _dev(gen, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gen.device) for a in arrays]


def _stats(gen):
    return gen.handle.sean_label_memo_stats() + gen.handle.sean_spade_memo_stats()


def _call(pair, labels, seed, what):
    """one generate() on both handles from host arrays; asserts equal images; returns what the call added to (calls, hits, stores, loads)"""
    memo, ref = pair
    B, S = labels.shape[0], labels.shape[-1]
    codes, noise = _inputs(B, S, seed)
    s0 = _stats(memo)
    a = memo.generate(*_dev(memo, labels, codes, noise))
    b = ref.generate(*_dev(ref, labels, codes, noise))
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.isfinite(a).all(), what
    assert np.array_equal(a, b), f'{what}: max |memo - reference| = {float(np.abs(a - b).max()):.3e}'
    assert _stats(ref) == (0, 0, 0, 0), 'the reference handle has no memo'
    return tuple(int(x - y) for x, y in zip(_stats(memo), s0))


def test_repeat(hip_lib):
    """labels L with codes and noise of seeds 1-4: PLAIN, STORE, LOAD, LOAD"""
    pair = _pair()
    L = _labels(2, 256, 111)
    got = [_call(pair, L, seed, f'repeat, call {seed}') for seed in (1, 2, 3, 4)]
    assert got == [PLAIN, STORE, LOAD, LOAD], got


def test_change_and_return(hip_lib):
    """L, L, L, L' (one pixel changed), L', L', L: the store waits for the second sight of a label set, and a changed map drops the cache"""
    pair = _pair()
    L = _labels(2, 256, 121)
    L2 = L.copy()
    L2[1, 16, 16] = (L[1, 16, 16] + 1) % 19
    got = [_call(pair, lab, seed, f'change, call {seed}') for seed, lab in enumerate((L, L, L, L2, L2, L2, L))]
    assert got == [PLAIN, STORE, LOAD, PLAIN, STORE, LOAD, PLAIN], got


def test_shape(hip_lib):
    """B = 1 on the B = 2 handle, S = 128 on the 256 handle: the key changes -- PLAIN, then STORE, LOAD (at 128 pixels up_1 is the 32-pixel level)"""
    pair = _pair()
    L = _labels(2, 256, 131)
    L128 = np.ascontiguousarray(L[:, ::2, ::2])
    seq = [(L, PLAIN), (L, STORE), (L, LOAD), (L[:1], PLAIN), (L[:1], STORE), (L[:1], LOAD), (L128, PLAIN), (L128, STORE), (L128, LOAD), (L, PLAIN)]
    for i, (lab, want) in enumerate(seq):
        assert _call(pair, lab, i, f'shape, call {i}') == want, i


def test_option_change(hip_lib):
    """ch_set_option between hits: PLAIN (the reference handle takes the same key)"""
    pair = _pair()
    L = _labels(2, 256, 141)
    try:
        got = [_call(pair, L, seed, f'before, call {seed}') for seed in (0, 1, 2)]
        assert got == [PLAIN, STORE, LOAD], got
        for g in pair:
            g.handle.set_option('sean.sparse', 0)
        got = [_call(pair, L, seed, f'sean.sparse = 0, call {seed}') for seed in (3, 4, 5)]
        assert got == [PLAIN, STORE, LOAD], got
    finally:
        for g in pair:
            g.handle.set_option('sean.sparse', 1)
    assert _call(pair, L, 6, 'sean.sparse = 1 again') == PLAIN


def test_graph(hip_lib):
    """capture once (warm-up call + capture), replay over refilled labels: same, same, changed, same"""
    memo, ref = _pair()
    L, L2 = _labels(2, 256, 151), _labels(2, 256, 152)
    codes, noise = _inputs(2, 256, 9)
    lab, c, n = _dev(memo, L, codes, noise)
    s0 = _stats(memo)
    g, out = memo.capture(lab, c, n)
    got = []
    for labels in (L, L, L2, L2):
        lab.copy_(torch.from_numpy(labels).to(memo.device))
        g.replay()
        torch.cuda.synchronize()
        got.append(out.cpu().numpy())
    # warm-up: PLAIN; replays: STORE, LOAD, PLAIN, STORE
    assert tuple(int(x - y) for x, y in zip(_stats(memo), s0)) == (5, 3, 2, 1)
    for labels, a in zip((L, L, L2, L2), got):
        b = ref.generate(*_dev(ref, labels, codes, noise)).cpu().numpy()
        assert np.array_equal(a, b)
    del g


def test_off_switch(hip_lib):
    """sean.spade_memo = 0 with the label memo on: the label memo counts, the SPADE memo does not, the images are the reference's"""
    _, ref = _pair()
    off = _build(NGF, 2, 256, **{'sean.spade_memo': 0})
    try:
        L = _labels(2, 256, 161)
        for seed in (1, 2, 3):
            assert _call((off, ref), L, seed, f'off, call {seed}') == (1, int(seed > 1), 0, 0)
    finally:
        off.handle.close()


def test_no_v_route(hip_lib):
    """ngf = 16, max_batch = 3, max_size = 128 (the handles of tests/test_hip_label_memo.py: 2 C < 512 on the 32 / 64-pixel levels, so no ACE
    takes the V route): nothing is counted, and the option allocates nothing"""
    used = []
    for on in (1, 0):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        g = _build(16, 3, 128, **{'sean.spade_memo': on})
        try:
            torch.cuda.synchronize()
            used.append(free0 - torch.cuda.mem_get_info(0)[0])
            if on:
                L = _labels(3, 128, 171)
                for seed in (1, 2, 3):
                    codes, noise = _inputs(3, 128, seed, ngf=16)
                    g.generate(*_dev(g, L, codes, noise))
                torch.cuda.synchronize()
                assert _stats(g) == (3, 2, 0, 0)
        finally:
            g.handle.close()
    print('device memory of the ngf = 16 handle, sean.spade_memo = 1 / 0:', used)
    assert used[0] == used[1], used
