"""GPU tests of the code memo (option sean.code_memo, ctrlhair_amd/csrc/sean_model.h SeanModel::code_state): on a chunk that takes the grouped
style-LUT launch, fc_mu_batched and the grouped LUT GEMM return at once when the chunk brings the style codes of the chunk before; the
projections (mu_all) and the LUTs (lut_ahead) of that chunk are what every consumer then reads.  Every output is compared with
np.array_equal against a second handle built with sean.code_memo = 0 and fed the same calls, and the (calls, hits) counters are asserted
call by call.

ngf = 32, max_batch = 4, max_size = 128, sean.ahead = 0.  The grouped launch needs more than 64 (sample, label) columns (B >= 4) and
18 C % 128 == 0 for every styled ACE (SeanBuild::style_lut_groups): at ngf = 16 the last styled ACE has C = 32 (18 C = 576) and the handle
builds no group table, so ngf = 32 (C = 64 there) is the smallest generator that takes mode.grouped; test_same_codes_new_labels would count
(0, 0) otherwise.  The committed calibration table holds ngf = 16 and 64 only, so the weights run with the identity running statistics, as on
the ngf = 32 handles of tests/test_hip_spade_memo.py.  The handles are shared by the module, so every test brings codes and label maps that
no test before it used and counts from the counters it finds."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NGF, MB, MS = 32, 4, 128
MISS, HIT, NONE = (1, 0), (1, 1), (0, 0)      # (calls, hits) one call adds
_handles = {}


def _build(**opts):
    from ctrlhair_amd import procedural as P
    from ctrlhair_amd.sean.generator import SeanGenerator
    options = {'sean.ahead': 0}
    options.update(opts)
    sd = P.sean_state_dict(0, NGF, calibrated=False)
    return SeanGenerator(0, f16x3=0, options=options).load_state_dict(sd, max_batch=MB, max_size=MS)


def _pair():
    """(generator with the code memo, reference generator without it), built once per module"""
    if 'pair' not in _handles:
        _handles['pair'] = (_build(), _build(**{'sean.code_memo': 0}))
    return _handles['pair']


@pytest.fixture(scope='module', autouse=True)
def _close_handles():
    yield
    for v in _handles.values():
        for g in v:
            g.handle.close()
    _handles.clear()


def _labels(B, seed, S=MS):
    from ctrlhair_amd import procedural as P
    return P.blocky_labels(B, S, grid=8, seed=seed)


def _codes(B, seed):
    from ctrlhair_amd import procedural as P
    return P.style_codes(B, seed=5000 + seed)


def _noise(B, seed, S=MS):
    from ctrlhair_amd import procedural as P
    return P.noise_planes(B, S, NGF, seed=7 + seed)


def _dev(gen, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(gen.device) for a in arrays]


def _stats(gen):
    return gen.handle.sean_code_memo_stats() + gen.handle.sean_label_memo_stats()


def _call(pair, labels, codes, seed, what, dev_codes=None):
    """one generate() on both handles (codes: a host array, uploaded into new tensors, or dev_codes = the memo handle's own tensor); asserts
    equal images; returns what the call added to (code calls, code hits, label calls, label hits)"""
    memo, ref = pair
    B, S = labels.shape[0], labels.shape[-1]
    noise = _noise(B, seed, S)
    s0 = _stats(memo)
    lab, c, n = _dev(memo, labels, codes, noise)
    a = memo.generate(lab, c if dev_codes is None else dev_codes, n)
    b = ref.generate(*_dev(ref, labels, codes, noise))
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert np.isfinite(a).all(), what
    assert np.array_equal(a, b), f'{what}: max |memo - reference| = {float(np.abs(a - b).max()):.3e}'
    assert ref.handle.sean_code_memo_stats() == (0, 0), 'the reference handle has no code memo'
    return tuple(int(x - y) for x, y in zip(_stats(memo), s0))


def test_same_codes_new_labels(hip_lib):
    """codes C with the label maps and noise of seeds 1-3: miss, hit, hit"""
    pair = _pair()
    C = _codes(MB, 10)
    got = [_call(pair, _labels(MB, 1000 + i), C, i, f'same codes, call {i}')[:2] for i in (1, 2, 3)]
    assert got == [MISS, HIT, HIT], got


def test_changed_word(hip_lib):
    """C, C, C' (one word of the last sample's last label changed), C', C, C"""
    pair = _pair()
    C = _codes(MB, 20)
    C2 = C.copy()
    C2[MB - 1, 18, 511] = np.float32(0.25) if C[MB - 1, 18, 511] != np.float32(0.25) else np.float32(0.5)
    got = [_call(pair, _labels(MB, 1010 + i), c, i, f'changed word, call {i}')[:2] for i, c in enumerate((C, C, C2, C2, C, C))]
    assert got == [MISS, HIT, MISS, HIT, MISS, HIT], got


def test_equal_bits_other_tensor_and_overwrite(hip_lib):
    """a second tensor with equal contents is a hit; an in-place overwrite of that tensor with other contents is a miss; -0.0 for 0.0 is a
    miss (the words are compared as integers)"""
    pair = _pair()
    memo = pair[0]
    C, C2 = _codes(MB, 30), _codes(MB, 31)
    C[0, 0, 0] = 0.0
    C3 = C.copy()
    C3[0, 0, 0] = -0.0
    L = _labels(MB, 1020)
    (t1,) = _dev(memo, C)
    assert _call(pair, L, C, 0, 'first tensor', dev_codes=t1)[:2] == MISS
    t2 = t1.clone()
    assert t2.data_ptr() != t1.data_ptr()
    assert _call(pair, L, C, 1, 'second tensor, equal contents', dev_codes=t2)[:2] == HIT
    t2.copy_(torch.from_numpy(C2).to(memo.device))
    assert _call(pair, L, C2, 2, 'overwritten in place', dev_codes=t2)[:2] == MISS
    assert _call(pair, L, C2, 3, 'the overwritten tensor again', dev_codes=t2)[:2] == HIT
    assert _call(pair, L, C, 4, 'back to C')[:2] == MISS
    assert _call(pair, L, C3, 5, '-0.0 in place of 0.0')[:2] == MISS


def test_ineligible_batch(hip_lib):
    """B = 3 on the B = 4 handle has 57 (sample, label) columns and takes the GEMV branch: the chunk goes through no decision, clears the
    copy's valid flag, and the B = 4 call after it is a miss although it brings the codes of the B = 4 call before"""
    pair = _pair()
    C, L = _codes(MB, 40), _labels(MB, 1030)
    seq = [(MB, MISS), (MB, HIT), (3, NONE), (3, NONE), (MB, MISS), (MB, HIT)]
    for i, (B, want) in enumerate(seq):
        assert _call(pair, L[:B], C[:B], i, f'batch {B}, call {i}')[:2] == want, i


def test_encode_between(hip_lib):
    """the Zencoder between two calls touches neither mu_all nor a lut_ahead buffer: the call after it is a hit with equal images"""
    pair = _pair()
    C, L = _codes(MB, 50), _labels(MB, 1040)
    assert _call(pair, L, C, 0, 'before encode')[:2] == MISS
    img = np.tanh(np.random.default_rng(50).standard_normal((MB, 3, MS, MS))).astype(np.float32)
    enc = [g.encode(*_dev(g, img, L)).cpu().numpy() for g in pair]
    assert np.isfinite(enc[0]).all() and np.array_equal(enc[0], enc[1])
    assert _call(pair, L, C, 1, 'after encode')[:2] == HIT
    # ... and the encoder's own codes, fed back
    assert _call(pair, L, enc[0], 2, 'encoded codes')[:2] == MISS
    assert _call(pair, L, enc[0], 3, 'encoded codes again')[:2] == HIT


def test_four_combinations(hip_lib):
    """the code memo and the label memo decide independently: neither hits, both hit, the codes alone, the labels alone (both handles carry
    the label memo)"""
    pair = _pair()
    C, C2, C3 = _codes(MB, 60), _codes(MB, 61), _codes(MB, 62)
    L, L2, L3 = _labels(MB, 1050), _labels(MB, 1051), _labels(MB, 1052)
    seq = [(L, C, MISS + MISS), (L, C, HIT + HIT), (L2, C, HIT + MISS), (L2, C2, MISS + HIT), (L3, C3, MISS + MISS), (L3, C3, HIT + HIT),
           (L3, C2, MISS + HIT), (L, C2, HIT + MISS)]
    for i, (lab, c, want) in enumerate(seq):
        assert _call(pair, lab, c, i, f'combination {i}') == want, i


def test_option_change(hip_lib):
    """ch_set_option between hits: the epoch is part of the key -- a miss"""
    pair = _pair()
    C, L = _codes(MB, 70), _labels(MB, 1060)
    try:
        got = [_call(pair, L, C, i, f'before, call {i}')[:2] for i in (0, 1)]
        assert got == [MISS, HIT], got
        for g in pair:
            g.handle.set_option('sean.sparse', 0)
        got = [_call(pair, L, C, i, f'sean.sparse = 0, call {i}')[:2] for i in (2, 3)]
        assert got == [MISS, HIT], got
    finally:
        for g in pair:
            g.handle.set_option('sean.sparse', 1)
    assert _call(pair, L, C, 4, 'sean.sparse = 1 again')[:2] == MISS


def test_profiling(hip_lib):
    """while ch_profile_enable is on a chunk is not eligible (the records time the launches that do the work): it goes through no decision and
    clears the copy's valid flag"""
    pair = _pair()
    C, L = _codes(MB, 75), _labels(MB, 1065)
    got = [_call(pair, L, C, i, f'before, call {i}')[:2] for i in (0, 1)]
    assert got == [MISS, HIT], got
    try:
        for g in pair:
            g.handle.profile_enable(True)
        got = [_call(pair, L, C, i, f'profiling, call {i}')[:2] for i in (2, 3)]
        assert got == [NONE, NONE], got
    finally:
        for g in pair:
            g.handle.profile_enable(False)
    got = [_call(pair, L, C, i, f'after, call {i}')[:2] for i in (4, 5)]
    assert got == [MISS, HIT], got


def test_graph(hip_lib):
    """capture once (warm-up call + capture), replay over refilled codes: same, same, changed, same"""
    memo, ref = _pair()
    C, C2, L = _codes(MB, 80), _codes(MB, 81), _labels(MB, 1070)
    noise = _noise(MB, 9)
    lab, c, n = _dev(memo, L, C, noise)
    s0 = _stats(memo)[:2]
    g, out = memo.capture(lab, c, n)
    got = []
    for codes in (C, C, C2, C2):
        c.copy_(torch.from_numpy(codes).to(memo.device))
        g.replay()
        torch.cuda.synchronize()
        got.append(out.cpu().numpy())
    # warm-up: miss; replays: hit, hit, miss, hit
    assert tuple(int(x - y) for x, y in zip(_stats(memo)[:2], s0)) == (5, 3)
    for codes, a in zip((C, C, C2, C2), got):
        b = ref.generate(*_dev(ref, L, codes, noise)).cpu().numpy()
        assert np.array_equal(a, b)
    del g


def test_off_switch(hip_lib):
    """sean.code_memo = 0 (the reference handle of this module): nothing is counted whatever the calls bring, and the option's buffers -- a
    copy of max_batch x 19 x 512 codes and eight state words -- are what the two handles differ by in device memory"""
    _, ref = _pair()
    C, L = _codes(MB, 90), _labels(MB, 1080)
    for i in (0, 1):
        ref.generate(*_dev(ref, L, C, _noise(MB, i)))
    torch.cuda.synchronize()
    assert ref.handle.sean_code_memo_stats() == (0, 0)
    used = []
    for on in (1, 0):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        g = _build(**{'sean.code_memo': on})
        try:
            torch.cuda.synchronize()
            used.append(free0 - torch.cuda.mem_get_info(0)[0])
        finally:
            g.handle.close()
    print('device memory of the handle, sean.code_memo = 1 / 0:', used)
    # (the allocator hands out whole pages: the copy is 152 KiB, the state 32 bytes)
    assert 0 <= used[0] - used[1] <= 4 << 20, used
