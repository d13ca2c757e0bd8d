"""What every Python class that calls ch_* entry points with raw pointers needs besides its arithmetic: the (handle, device) pair, the
stream of a call, scratch memory that grows and never shrinks, and the two-download return of compressed bytes.  torch is imported
inside the methods, as in the modules this serves: importing them for their host-side helpers imports no torch."""
from . import lib as _lib


class DeviceOp:
    """Base of the classes that work on one ch_handle on one GPU."""

    def __init__(self, handle=None, device=None):
        """device: None, an int, a string or a torch.device; without one it is the handle's.  Without a handle one is created on the
        device (cuda:0 by default), which raises without the library or a GPU.  No CPU fallback exists: any other device raises."""
        import torch
        if device is None:
            device = torch.device('cuda', handle.device if handle is not None else 0)
        elif not isinstance(device, torch.device):
            device = torch.device('cuda', device) if isinstance(device, int) else torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'{type(self).__name__} runs on the GPU only (no CPU fallback exists)')
        self.device = device
        self.handle = handle if handle is not None else _lib.Handle(device.index or 0)

    def _stream(self):
        """The raw stream handle of torch's current stream on the device."""
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def _buffer(self, name: str, need: int, pinned: bool = False):
        """The uint8 tensor kept in attribute `name`, at least max(need, 256) bytes, on the device or in pinned host memory;
        reallocated only when it is too small.  Pass its numel() as the workspace_bytes of a call."""
        import torch
        buf = getattr(self, name, None)
        if buf is None or buf.numel() < need:
            where = {'pin_memory': True} if pinned else {'device': self.device}
            buf = torch.empty(max(need, 256), dtype=torch.uint8, **where)
            setattr(self, name, buf)
        return buf

    def _fetch_ragged(self, out, bound: int, sizes, lo: int, what: str):
        """N byte strings from the device in two downloads: the lengths, then exactly those bytes.  out: uint8 device buffer whose
        slot n starts at n * bound; sizes: int64 device tensor [N]; lo: the smallest legal length; what: '<entry> returned
        <thing> lengths' for the error.  -> list of N bytes."""
        import numpy as np
        import torch
        lens = [int(v) for v in sizes.cpu()]                                   # download 1 (synchronises)
        if any(v < lo or v > bound for v in lens):
            raise RuntimeError(f'{what} {lens} outside {lo}..{bound}')
        N = len(lens)
        packed = out[:lens[0]] if N == 1 else torch.cat([out[n * bound:n * bound + lens[n]] for n in range(N)])
        total = sum(lens)
        stage = self._buffer('_pinned', total, pinned=True)
        stage[:total].copy_(packed)                                            # download 2: exactly the compressed bytes
        raw = stage[:total].numpy().tobytes()
        offs = np.concatenate([[0], np.cumsum(lens)])
        return [raw[offs[n]:offs[n + 1]] for n in range(N)]
