"""Device-side image ingest: decoded uint8 images of any sizes -> the float32 input tensor of a network, in one call per batch
(ch_ingest_images / ch_ingest_labels, csrc/ingest.hip).

What the masks and codes jobs do per image on one CPU core -- Pillow's `resize((512, 512), BILINEAR)` + FaceParsing.normalise, or
hostutil.resize_bilinear + `/ 127.5 - 1` -- is here one resize on 8-bit data followed by a 256-entry float table per channel.  The
resizes are integer arithmetic and equal the host's byte for byte; the table is evaluated ONCE by the host path's own code over the
256 byte values, so the floats are bit-identical whatever that code does (on the GPU torch turns `t / 255.0` into a multiplication by
a reciprocal: restating the division in a kernel would be wrong in the last bit for some values).

The host half (Pillow's coefficient tables, the packing of a batch) imports neither torch nor the library.

Batch layout (include/ctrlhair_hip.h): N descriptors of 32 bytes {uint64 address, int32 H, W, htab, vtab, int64 reserved}, then the
tables the descriptors point to, each {in, out, ksize, layout, bounds [out][2], k} in int32 and starting at a multiple of 16 bytes.
"""
from typing import List, Sequence, Tuple

import numpy as np

from .devop import DeviceOp

MODE_PIL_BILINEAR, MODE_CV2_LINEAR, MODE_LABELS = 0, 1, 2       # CH_INGEST_*
MAX_SIDE, MAX_OUT = 32768, 4096
PRECISION_BITS = 22                                             # Pillow: 32 - 8 - 2
DESC = np.dtype([('src', '<u8'), ('H', '<i4'), ('W', '<i4'), ('htab', '<i4'), ('vtab', '<i4'), ('reserved', '<i8')])
assert DESC.itemsize == 32

_coeffs = {}          # (n_in, n_out) -> (xmin, count, kk)
_tables = {}          # (n_in, n_out, layout) -> the packed int32 table


def pil_bilinear_coeffs(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the BILINEAR filter on one axis: (xmin int32 [n_out], count int32 [n_out],
    kk int32 [n_out, ksize]); output i is clip8(((1 << 21) + sum_j kk[i, j] * p[xmin[i] + j]) >> 22) over j < count[i], the rest of a
    row of kk is zero.  Double arithmetic in Pillow's order: the weights are summed first to last and divided by that sum."""
    if not (1 <= n_in <= MAX_SIDE and 1 <= n_out <= MAX_SIDE):
        raise ValueError(f'pil_bilinear_coeffs: sizes {n_in} -> {n_out} outside 1..{MAX_SIDE}')
    key = (int(n_in), int(n_out))
    if key not in _coeffs:
        scale = n_in / n_out
        fs = max(scale, 1.0)
        support = 1.0 * fs
        ksize = int(np.ceil(support)) * 2 + 1
        xmin, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
        kk = np.zeros((n_out, ksize), np.int32)
        for xx in range(n_out):
            center = (xx + 0.5) * scale
            lo = max(int(center - support + 0.5), 0)
            hi = min(int(center + support + 0.5), n_in)
            w = np.maximum(0.0, 1.0 - np.abs((np.arange(hi - lo) + lo - center + 0.5) / fs))
            ww = np.cumsum(w)[-1]                                # sequential, as the C loop adds them
            if ww != 0.0:
                w = w / ww
            xmin[xx], count[xx] = lo, hi - lo
            kk[xx, :hi - lo] = (w * float(1 << PRECISION_BITS) + 0.5).astype(np.int32)
        for a in (xmin, count, kk):
            a.setflags(write=False)
        _coeffs[key] = (xmin, count, kk)
    return _coeffs[key]


def _table(n_in: int, n_out: int, layout: int) -> np.ndarray:
    """The table of one pass as the batch holds it; layout 1: k stored [ksize][out] (horizontal pass), 0: [out][ksize] (vertical)."""
    key = (int(n_in), int(n_out), layout)
    if key not in _tables:
        if len(_tables) >= 256:
            _tables.clear()
        xmin, count, kk = pil_bilinear_coeffs(n_in, n_out)
        t = np.concatenate([np.array([n_in, n_out, kk.shape[1], layout], np.int32), np.stack([xmin, count], 1).ravel(),
                            (kk.T if layout else kk).ravel()])
        _tables[key] = np.concatenate([t, np.zeros(-t.size % 4, np.int32)])
    return _tables[key]


def pack_batch(addresses: Sequence[int], shapes: Sequence[Tuple[int, int]], size: int, mode: int) -> np.ndarray:
    """The batch of one ch_ingest_images / ch_ingest_labels call as uint8 host bytes: descriptors, then (mode 0) one table per distinct
    (in, size) pair and pass.  addresses: device addresses of the pixels; shapes: (H, W) per image."""
    N = len(addresses)
    if N < 1 or len(shapes) != N:
        raise ValueError('pack_batch: need one (H, W) per address and at least one image')
    if mode not in (MODE_PIL_BILINEAR, MODE_CV2_LINEAR, MODE_LABELS):
        raise ValueError(f'pack_batch: unknown mode {mode}')
    if not 1 <= size <= MAX_OUT:
        raise ValueError(f'pack_batch: output side {size} outside 1..{MAX_OUT}')
    desc = np.zeros(N, DESC)
    desc['src'] = np.asarray(addresses, np.uint64)
    desc['htab'] = desc['vtab'] = -1
    parts, where, cur = [], {}, N * DESC.itemsize // 4

    def place(n_in, layout):
        nonlocal cur
        if (n_in, layout) not in where:
            t = _table(n_in, size, layout)
            where[(n_in, layout)] = cur
            parts.append(t)
            cur += t.size
        return where[(n_in, layout)]

    for n, (H, W) in enumerate(shapes):
        if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
            raise ValueError(f'pack_batch: image {n} is {W} x {H}; sides must be in 1..{MAX_SIDE}')
        desc['H'][n], desc['W'][n] = H, W
        if mode == MODE_PIL_BILINEAR:
            if W != size:
                desc['htab'][n] = place(W, 1)
            if H != size:
                desc['vtab'][n] = place(H, 0)
    return np.concatenate([desc.view(np.uint8)] + [t.view(np.uint8) for t in parts])


def unpack_batch(blob: np.ndarray, N: int) -> List[dict]:
    """The inverse of pack_batch, for tests and debugging: per image {'src', 'H', 'W', 'h': table or None, 'v': table or None}, a table
    being (n_in, n_out, xmin, count, kk [n_out, ksize])."""
    blob = np.ascontiguousarray(blob, np.uint8)
    desc = blob[:N * DESC.itemsize].view(DESC)
    words = blob.view(np.int32)

    def table(at):
        if at < 0:
            return None
        n_in, n_out, ksize, layout = (int(v) for v in words[at:at + 4])
        bounds = words[at + 4:at + 4 + 2 * n_out].reshape(n_out, 2)
        k = words[at + 4 + 2 * n_out:at + 4 + 2 * n_out + n_out * ksize]
        kk = k.reshape(ksize, n_out).T if layout else k.reshape(n_out, ksize)
        return n_in, n_out, bounds[:, 0].copy(), bounds[:, 1].copy(), kk.copy()

    return [{'src': int(d['src']), 'H': int(d['H']), 'W': int(d['W']), 'h': table(int(d['htab'])), 'v': table(int(d['vtab']))} for d in desc]


def sean_lut() -> np.ndarray:
    """float32 [3,256]: HairEditor.preprocess_img's `/ 127.5 - 1.0` in float64, then the codes job's cast to float32."""
    return np.tile((np.arange(256) / 127.5 - 1.0).astype(np.float32), (3, 1))


class ImageIngest(DeviceOp):
    """ch_ingest_images / ch_ingest_labels on one ch_handle.  Every call is one upload of the batch and a fixed number of launches on
    torch's current stream, with no synchronisation; the inputs are lists of uint8 device tensors of any sizes."""

    def _call(self, tensors, channels, size, mode, lut):
        import ctypes as C
        import torch
        tensors = [t.contiguous() for t in tensors]          # (kept alive until the call is enqueued)
        for n, t in enumerate(tensors):
            ok = t.dtype == torch.uint8 and t.device == self.device and (t.dim() == 3 and t.shape[2] == 3 if channels == 3 else t.dim() == 2)
            if not ok:
                raise ValueError(f'ImageIngest: input {n} must be a uint8 tensor {"[H,W,3]" if channels == 3 else "[H,W]"} on {self.device}, '
                                 f'got {t.dtype} {tuple(t.shape)} on {t.device}')
        N = len(tensors)
        blob = pack_batch([t.data_ptr() for t in tensors], [(t.shape[0], t.shape[1]) for t in tensors], size, mode)
        bp = blob.ctypes.data_as(C.c_void_p)
        need = int(self.handle.lib.ch_ingest_workspace_bytes(bp, blob.nbytes, N, size, mode))
        if need == 0:
            raise ValueError(f'ImageIngest: the library refuses this batch (N={N}, size={size}, mode={mode})')
        ws = self._buffer('_ws', need)
        if mode == MODE_LABELS:
            out = torch.empty((N, size, size), dtype=torch.uint8, device=self.device)
            self.handle.call('ch_ingest_labels', bp, blob.nbytes, N, size, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        else:
            if lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256) or lut.device != self.device or not lut.is_contiguous():
                raise ValueError('ImageIngest: lut must be a contiguous float32 tensor [3,256] on the device')
            out = torch.empty((N, 3, size, size), dtype=torch.float32, device=self.device)
            self.handle.call('ch_ingest_images', bp, blob.nbytes, N, size, mode, lut.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                             self._stream())
        return out

    def parse_input(self, images, size: int = 512, lut=None):
        """Per image FaceParsing.normalise(Image.resize((size, size), BILINEAR)), float32 [N,3,size,size], bit for bit.
        lut: FaceParsing.ingest_lut() of the network the tensor is for."""
        if lut is None:
            raise ValueError('ImageIngest.parse_input: pass lut=FaceParsing.ingest_lut()')
        return self._call(images, 3, size, MODE_PIL_BILINEAR, lut)

    def sean_input(self, images, size: int):
        """Per image HairEditor.preprocess_img (cv2's bilinear resize, / 127.5 - 1) cast to float32: [N,3,size,size], bit for bit."""
        import torch
        if getattr(self, '_sean_lut', None) is None:
            self._sean_lut = torch.from_numpy(sean_lut()).to(self.device)
        return self._call(images, 3, size, MODE_CV2_LINEAR, self._sean_lut)

    def labels(self, maps, size: int):
        """Per map HairEditor.preprocess_mask (nearest resize): uint8 [N,size,size]."""
        return self._call(maps, 1, size, MODE_LABELS, None)
