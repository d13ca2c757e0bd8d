"""ctrlhair_amd.devop.DeviceOp: the device and handle of a wrapper class (CPU, with a stub handle), its growing buffers and the
two-download return of ragged bytes (GPU)."""
import numpy as np
import pytest
import torch

from ctrlhair_amd.devop import DeviceOp


class StubHandle:
    """What DeviceOp reads of a lib.Handle."""

    def __init__(self, device=0):
        self.device = device


class Probe(DeviceOp):
    pass


# ---- CPU: the constructor ----------------------------------------------------------------------------------------------------------
def test_device_from_handle_int_string_and_torch_device():
    h = StubHandle(0)
    assert Probe(h).device == torch.device('cuda', 0) and Probe(h).handle is h
    assert Probe(StubHandle(5)).device == torch.device('cuda', 5)           # no device given: the handle's
    assert Probe(h, 1).device == torch.device('cuda', 1)
    assert Probe(h, 'cuda:2').device == torch.device('cuda', 2)
    d = torch.device('cuda', 3)
    assert Probe(h, d).device is d
    assert Probe(h, 'cuda').device == torch.device('cuda')                  # without an index: kept as given
    assert Probe(device='cuda:1', handle=h).device == torch.device('cuda', 1)


@pytest.mark.parametrize('device', ['cpu', torch.device('cpu')])
def test_cpu_device_is_refused_with_the_class_name(device):
    from ctrlhair_amd.alignment import FaceAligner
    from ctrlhair_amd.pngenc import PngEncoder
    from ctrlhair_amd.stylestats import StyleMedoid
    for cls in (Probe, FaceAligner, StyleMedoid, PngEncoder):
        with pytest.raises(RuntimeError) as e:
            cls(StubHandle(0), device)
        assert str(e.value) == f'{cls.__name__} runs on the GPU only (no CPU fallback exists)'


# ---- GPU: buffers and the ragged download ----------------------------------------------------------------------------------------------
@pytest.fixture
def op():
    return Probe(StubHandle(0), 'cuda:0')


@pytest.mark.gpu
def test_buffer_minimum_reuse_and_growth(op):
    for need in (0, 1):
        b = Probe(StubHandle(0), 'cuda:0')._buffer('_ws', need)
        assert b.dtype == torch.uint8 and b.is_cuda and b.numel() >= 256
    a = op._buffer('_ws', 1000)
    assert a.numel() >= 1000 and op._ws is a
    assert op._buffer('_ws', 1000) is a and op._buffer('_ws', 10) is a and op._buffer('_ws', 0) is a       # suffices: the same tensor
    b = op._buffer('_ws', a.numel() + 1)
    assert b is not a and b.numel() >= a.numel() + 1 and op._ws is b                                       # grown, same attribute
    other = op._buffer('_dws', 300)
    assert other is op._dws and other is not b and op._ws is b                                             # one buffer per name


@pytest.mark.gpu
def test_buffer_pinned(op):
    p = op._buffer('_pinned', 1, pinned=True)
    assert p.is_pinned() and not p.is_cuda and p.dtype == torch.uint8 and p.numel() >= 256
    assert op._buffer('_pinned', 256, pinned=True) is p
    q = op._buffer('_pinned', 5000, pinned=True)
    assert q.is_pinned() and q.numel() >= 5000 and op._pinned is q


LO, BOUND = 2, 16


def _slots(N):
    pattern = (np.arange(N * BOUND) * 7 % 251).astype(np.uint8)
    return pattern, torch.from_numpy(pattern).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize('lens', [[5], [LO], [BOUND], [LO, 5, BOUND]])
def test_fetch_ragged_returns_each_slot_s_bytes(op, lens):
    pattern, out = _slots(len(lens))
    sizes = torch.tensor(lens, dtype=torch.int64, device='cuda')
    got = op._fetch_ragged(out, BOUND, sizes, LO, 'probe returned lengths')
    assert got == [pattern[n * BOUND:n * BOUND + v].tobytes() for n, v in enumerate(lens)]
    assert all(isinstance(g, bytes) for g in got)
    assert op._fetch_ragged(out, BOUND, sizes, LO, 'probe returned lengths') == got         # the pinned stage is reused, same answer


@pytest.mark.gpu
@pytest.mark.parametrize('lens', [[LO - 1], [BOUND + 1], [LO, LO - 1, BOUND], [LO, 5, BOUND + 1]])
def test_fetch_ragged_refuses_a_length_out_of_range(op, lens):
    _, out = _slots(len(lens))
    sizes = torch.tensor(lens, dtype=torch.int64, device='cuda')
    with pytest.raises(RuntimeError) as e:
        op._fetch_ragged(out, BOUND, sizes, LO, 'ch_probe returned scan lengths')
    assert str(e.value) == f'ch_probe returned scan lengths {lens} outside {LO}..{BOUND}'
