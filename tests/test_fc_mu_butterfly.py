"""The wave reduction of fc_mu (ctrlhair_amd/csrc/sean_kernels.hip, fc_mu_body<TR = true>), restated in numpy float32 and checked bit for
bit against the 32 independent xor butterflies it replaces.  A wave holds 32 partial sums per lane (4 features x 8 samples).  The
transposed form halves the values a lane carries at every offset: at 32 the lanes below 32 keep values 0..15 and send 16..31 (the upper
lanes the reverse), then 8, 4, 2, 1 values per lane at offsets 16, 8, 4, 2, and a plain exchange at offset 1.  Every sum still adds lane l
and lane l ^ off in the order 32, 16, .., 1, so lane l must end with the very bits the independent butterfly of value l >> 1 leaves there."""
import numpy as np

LANES = np.arange(64)


def _independent(part):
    """part [64 lanes][32 values] float32 -> [64][32]: v += shfl_xor(v, off) for off = 32 .. 1, every value on its own."""
    v = part.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[LANES ^ off]).astype(np.float32)
    return v


def _transposed(part):
    """-> [64]: lane l's final register, the sum of value l >> 1."""
    q = part.copy()
    for off in (32, 16, 8, 4, 2):
        half = q.shape[1] // 2
        up = (LANES & off) != 0
        keep = np.where(up[:, None], q[:, half:], q[:, :half])
        send = np.where(up[:, None], q[:, :half], q[:, half:])
        q = (keep + send[LANES ^ off]).astype(np.float32)
    assert q.shape == (64, 1)
    q = q[:, 0]
    return (q + q[LANES ^ 1]).astype(np.float32)


def _check(part):
    with np.errstate(invalid='ignore', over='ignore'):
        ind, tr = _independent(part), _transposed(part)
    # the butterfly leaves the same bits in every lane
    assert (ind.view(np.uint32) == ind[0].view(np.uint32)[None, :]).all()
    want = ind[LANES, LANES >> 1]
    assert np.array_equal(tr.view(np.uint32), want.view(np.uint32))
    # and lane l >> 1 ... the element a result lane stores is the one lane 0 stored before
    assert np.array_equal(tr[::2].view(np.uint32), ind[0].view(np.uint32))


def test_transposed_butterfly_bits_mixed_magnitudes():
    rng = np.random.default_rng(5)
    for _ in range(50):
        part = (rng.standard_normal((64, 32)) * np.exp2(rng.integers(-30, 30, (64, 32)))).astype(np.float32)
        _check(part)
    # cancellation: large values of both signs beside small ones
    part = (rng.standard_normal((64, 32)) * 1e-3).astype(np.float32)
    part[::2] += np.float32(3e7)
    part[1::2] -= np.float32(3e7)
    _check(part)


def test_transposed_butterfly_bits_with_an_inf_row():
    rng = np.random.default_rng(6)
    part = rng.standard_normal((64, 32)).astype(np.float32)
    part[17, :] = np.inf                     # one lane's partial sums overflowed
    part[40, 3] = np.float32(3.0e38)         # and a value that overflows in the sum
    part[41, 3] = np.float32(3.0e38)
    _check(part)
    assert np.isinf(_transposed(part)).all()
