"""EXIF orientation on the device: stored uint8 images of any sizes -> the upright images, one launch per batch (ch_orient_u8,
csrc/orient.hip).

A phone held upright stores the sensor's landscape pixels plus `Orientation = 6`; every viewer shows the upright picture.  Orienter.apply
is `ImageOps.exif_transpose` for pixels that are already on the device.  orient_numpy is the same permutation in numpy (the oracle of
the kernel, itself checked against Pillow for all eight values); orient_points / unorient_points carry pixel coordinates along.

The host half (oracle, points, the packing of a batch) imports neither torch nor the library.

Batch layout (include/ctrlhair_hip.h): N descriptors of 32 bytes {uint64 source address, int64 destination byte offset, int32 H, W, C,
orientation}; the sources are addressed by pointer (as in ingest.py: the decoders' tensors are used where they lie), the upright images
land in ONE destination buffer at ascending offsets, and apply returns views of it.
"""
from typing import List, Sequence, Tuple

import numpy as np

from .devop import DeviceOp

MAX_SIDE = 32768                                                # CH_ORIENT_MAX_SIDE
DESC = np.dtype([('src', '<u8'), ('dst', '<i8'), ('H', '<i4'), ('W', '<i4'), ('C', '<i4'), ('orient', '<i4')])
assert DESC.itemsize == 32
TRANSPOSING = (5, 6, 7, 8)
# orientation -> (transposes, reverses the stored rows, reverses the stored columns)
_FLAGS = {1: (0, 0, 0), 2: (0, 0, 1), 3: (0, 1, 1), 4: (0, 1, 0), 5: (1, 0, 0), 6: (1, 1, 0), 7: (1, 1, 1), 8: (1, 0, 1)}
_INVERSE = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 8, 7: 7, 8: 6}     # the orientation that turns the upright image back into the stored one


def turns(orientation) -> bool:
    """True for 2..8: the values that change the pixels.  1, a missing tag and anything outside 1..8 leave the image alone."""
    return isinstance(orientation, (int, np.integer)) and not isinstance(orientation, bool) and 2 <= int(orientation) <= 8


def inverse_orientation(orientation: int) -> int:
    return _INVERSE[int(orientation)] if turns(orientation) else 1


def orient_numpy(a: np.ndarray, orientation: int) -> np.ndarray:
    """The upright image of stored pixels a [H,W] or [H,W,C]: ImageOps.exif_transpose's permutation (a view of a)."""
    if not turns(orientation):
        return a
    o = int(orientation)
    t = a.transpose(1, 0, 2) if a.ndim == 3 else a.T
    return {2: a[:, ::-1], 3: a[::-1, ::-1], 4: a[::-1], 5: t, 6: t[:, ::-1], 7: t[::-1, ::-1], 8: t[::-1]}[o]


def upright_shape(H: int, W: int, orientation: int) -> Tuple[int, int]:
    """(H, W) of the upright image of a stored H x W one."""
    return (W, H) if turns(orientation) and int(orientation) in TRANSPOSING else (H, W)


def orient_points(points, orientation: int, H: int, W: int) -> np.ndarray:
    """Pixel-index coordinates (x, y) [..., 2] of the STORED H x W image -> the upright image: a point on pixel (x, y) lands on the pixel
    that received its value, orient_numpy(a, o)[y', x'] == a[y, x].  Fractions move with their pixel (x -> W - 1 - x for a mirror)."""
    p = np.array(points, dtype=np.float64)
    if not turns(orientation):
        return p
    T, FY, FX = _FLAGS[int(orientation)]
    x, y = p[..., 0].copy(), p[..., 1].copy()
    if FX:
        x = (W - 1) - x
    if FY:
        y = (H - 1) - y
    p[..., 0], p[..., 1] = (y, x) if T else (x, y)
    return p


def unorient_points(points, orientation: int, H: int, W: int) -> np.ndarray:
    """The inverse of orient_points: coordinates of the upright image -> the stored H x W image (H, W: the STORED image's)."""
    Hu, Wu = upright_shape(H, W, orientation)
    return orient_points(points, inverse_orientation(orientation), Hu, Wu)


def pack_batch(addresses: Sequence[int], shapes: Sequence[Tuple[int, int, int]], orientations: Sequence[int], align: int = 256):
    """(batch, offsets, dst_bytes) of one ch_orient_u8 call: the descriptors as uint8 host bytes, the byte offset of every upright image in
    the destination buffer (ascending, each a multiple of `align`) and that buffer's size.  shapes: (H, W, C) of the stored images."""
    N = len(addresses)
    if N < 1 or len(shapes) != N or len(orientations) != N:
        raise ValueError('pack_batch: need one (H, W, C) and one orientation per address, and at least one image')
    if align < 1:
        raise ValueError('pack_batch: align must be positive')
    desc = np.zeros(N, DESC)
    cur = 0
    for n, ((H, W, C), o) in enumerate(zip(shapes, orientations)):
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError(f'pack_batch: image {n} is {W} x {H}; sides must be in 1..{MAX_SIDE}')
        if C not in (1, 3, 4):
            raise ValueError(f'pack_batch: image {n} has {C} channels; expected 1, 3 or 4')
        if isinstance(o, bool) or not isinstance(o, (int, np.integer)) or not 1 <= int(o) <= 8:
            raise ValueError(f'pack_batch: image {n} has orientation {o!r}; expected 1..8')
        cur = -(-cur // align) * align
        desc[n] = (int(addresses[n]), cur, H, W, C, int(o))
        cur += H * W * C
    return desc.view(np.uint8), [int(v) for v in desc['dst']], cur


class Orienter(DeviceOp):
    """ch_orient_u8 on one ch_handle.  A call is one upload of the descriptors and one launch on torch's current stream, with no
    synchronisation.  No CPU fallback: the constructor needs the library and a GPU."""

    def apply(self, images, orientations, align: int = 256) -> List:
        """images: uint8 device tensors [H,W,C] (C = 1, 3 or 4) or [H,W], of any sizes; orientations: one EXIF value each.  -> the
        upright images, a list of uint8 device tensors ([W,H,...] for orientations 5..8).  Orientation 1 and any value outside 1..8
        return the input tensor itself; all the others are turned by ONE launch and are views of one new buffer, each starting at a
        multiple of `align` bytes."""
        import ctypes as C
        import torch
        images = list(images)
        orientations = list(orientations)
        if len(images) != len(orientations):
            raise ValueError(f'Orienter.apply: {len(orientations)} orientations for {len(images)} images')
        out = list(images)
        idx = [i for i, o in enumerate(orientations) if turns(o)]
        if not idx:
            return out
        src = []
        for i in idx:
            t = images[i]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.device != self.device or t.dim() not in (2, 3) or \
                    (t.dim() == 3 and t.shape[2] not in (1, 3, 4)) or t.numel() == 0:
                raise ValueError(f'Orienter.apply: input {i} must be a non-empty uint8 tensor [H,W,C] (C = 1, 3, 4) or [H,W] on {self.device}, '
                                 f'got {getattr(t, "dtype", type(t))} {tuple(getattr(t, "shape", ()))} on {getattr(t, "device", "the host")}')
            src.append(t.contiguous())                        # (kept alive until the call is enqueued)
        shapes = [(int(t.shape[0]), int(t.shape[1]), int(t.shape[2]) if t.dim() == 3 else 1) for t in src]
        turn = [int(orientations[i]) for i in idx]
        blob, offsets, total = pack_batch([t.data_ptr() for t in src], shapes, turn, align)
        blob = np.ascontiguousarray(blob)
        bp = blob.ctypes.data_as(C.c_void_p)
        need = int(self.handle.lib.ch_orient_workspace_bytes(bp, blob.nbytes, len(idx), total))
        if need == 0:
            raise ValueError(f'Orienter.apply: the library refuses this batch (N={len(idx)}, {total} bytes)')
        ws = self._buffer('_ws', need)
        dst = torch.empty(total, dtype=torch.uint8, device=self.device)
        self.handle.call('ch_orient_u8', bp, blob.nbytes, len(idx), dst.data_ptr(), total, ws.data_ptr(), ws.numel(), self._stream())
        for i, t, (H, W, Cn), o, off in zip(idx, src, shapes, turn, offsets):
            Hu, Wu = upright_shape(H, W, o)
            out[i] = dst[off:off + H * W * Cn].view((Hu, Wu, Cn) if t.dim() == 3 else (Hu, Wu))
        return out
