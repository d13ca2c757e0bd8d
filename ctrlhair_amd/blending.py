"""The blending step that follows the generator, on the HIP library.

`PoissonBlender(handle)` is a drop-in for the reference's `poisson_blending.poisson_blending(source, target, mask,
with_gamma)` (poisson_blending.py:29-87) and for the mask construction of hair_editor.py:297-305 (`blend_mask`): numpy /
torch uint8 in, numpy uint8 out, all arithmetic in `ch_poisson_blend` / `ch_blend_mask`.  `blend_batch` is the same solve for
a batch of images in one call (`ch_poisson_blend_batch`: one pair of launches per CG iteration for the whole batch), device
tensors in and out; image i of it is bit-identical to `__call__` on image i.  No CPU fallback: without the library these raise."""
import warnings

import ctypes as C

import numpy as np
import torch

from . import lib as _lib
from .devop import DeviceOp


class PoissonBlender(DeviceOp):
    def __init__(self, handle: _lib.Handle, device: torch.device, max_iters: int = 4000, rel_tol: float = 1e-7):
        super().__init__(handle, device)
        self.max_iters, self.rel_tol = max_iters, rel_tol
        self.last_iters = 0              # blend_batch: per-image lists
        self.last_converged = True
        self.max_workspace_bytes = 1 << 30      # blend_batch solves larger batches in chunks of as many images as fit

    def _u8(self, a, shape):
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(a)))
        t = t.to(self.device).to(torch.uint8).reshape(shape).contiguous()
        return t

    @staticmethod
    def workspace_bytes(H: int, W: int) -> int:
        """Bytes of solver workspace per image (csrc/poisson_kernels.hip poisson_workspace_bytes: 15 f64 planes, the dot-product
        partials, the unknown map and the CG state)."""
        return 256 + (15 * H * W * 8 + 6 * 512 * 8 + H * W + 255) // 256 * 256

    def blend_mask(self, target_parsing, face_parsing) -> torch.Tensor:
        """hair_editor.py:297-305 -> res_mask_dilated uint8 [H,W] on the device (1 = generated image is kept).  A batch
        [B,H,W] of target parsings gives [B,H,W] in one call; face_parsing is then [B,H,W] or one [H,W] map for all."""
        tp = np.asarray(target_parsing) if not isinstance(target_parsing, torch.Tensor) else target_parsing
        H, W = tp.shape[-2:]
        if tp.ndim == 3:
            B = int(tp.shape[0])
            t = self._u8(target_parsing, (B, H, W))
            fp = face_parsing if isinstance(face_parsing, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(face_parsing)))
            f = self._u8(fp, (-1, H, W)).expand(B, H, W).contiguous()
            out = torch.empty(B, H, W, dtype=torch.uint8, device=self.device)
            self.handle.call('ch_blend_mask_batch', t.data_ptr(), f.data_ptr(), out.data_ptr(), B, H, W, self._stream())
            return out
        t, f = self._u8(target_parsing, (H, W)), self._u8(face_parsing, (H, W))
        out = torch.empty(H, W, dtype=torch.uint8, device=self.device)
        self.handle.call('ch_blend_mask', t.data_ptr(), f.data_ptr(), out.data_ptr(), H, W, self._stream())
        return out

    def __call__(self, source, target, mask, with_gamma=True) -> np.ndarray:
        """source, target: [H,W,3] uint8 (cv2 layout); mask [H,W] / [H,W,1], non-zero = keep source gradients, zero = keep
        the target pixel -> blended uint8 [H,W,3]."""
        H, W = int(source.shape[0]), int(source.shape[1])
        s, t = self._u8(source, (H, W, 3)), self._u8(target, (H, W, 3))
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
        m = (m.to(self.device).reshape(H, W) != 0).to(torch.uint8).contiguous()
        out = torch.empty(H, W, 3, dtype=torch.uint8, device=self.device)
        iters = C.c_int(0)
        self.handle.call('ch_poisson_blend', s.data_ptr(), t.data_ptr(), m.data_ptr(), out.data_ptr(), H, W,
                         1 if with_gamma else 0, self.max_iters, float(self.rel_tol), C.byref(iters), self._stream())
        # negated count (INT_MIN for zero iterations) = rel_tol not reached (include/ctrlhair_hip.h)
        self.last_iters = 0 if iters.value == -2 ** 31 else abs(iters.value)
        self.last_converged = iters.value >= 0
        if not self.last_converged:
            # the reference solves the system directly (poisson_blending.py:80-85): a partially converged image is not its result
            warnings.warn(f'Poisson blending stopped after {self.last_iters} CG iterations without reaching rel_tol='
                          f'{self.rel_tol:g}; raise PoissonBlender.max_iters', RuntimeWarning)
        return out.cpu().numpy()

    def blend_batch(self, source, target, mask, with_gamma=True) -> torch.Tensor:
        """__call__ for a batch, device-resident: target [B,H,W,3], mask [B,H,W] / [B,H,W,1], source [B,H,W,3] or one [H,W,3]
        image for the whole batch (numpy, or torch on any device; uint8 tensors already on the device are used in place) ->
        blended uint8 [B,H,W,3] ON THE DEVICE.  Image i is bit-identical to __call__(source_i, target_i, mask_i), iteration
        count included; last_iters / last_converged become per-image lists.  The only host synchronisation is the solver's
        convergence poll."""
        tt = target if isinstance(target, torch.Tensor) else np.asarray(target)
        B, H, W = int(tt.shape[0]), int(tt.shape[1]), int(tt.shape[2])
        t = self._u8(target, (B, H, W, 3))
        s = source if isinstance(source, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(source)))
        s = self._u8(s, (-1, H, W, 3)).expand(B, H, W, 3).contiguous()      # one source for all: repeated on the device
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask)))
        m = (m.to(self.device).reshape(B, H, W) != 0).to(torch.uint8).contiguous()
        out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=self.device)
        chunk = max(1, int(self.max_workspace_bytes) // self.workspace_bytes(H, W))
        stream = self._stream()
        counts = []
        for i in range(0, B, chunk):
            n = min(chunk, B - i)
            iters = (C.c_int * n)()
            self.handle.call('ch_poisson_blend_batch', s[i:].data_ptr(), t[i:].data_ptr(), m[i:].data_ptr(), out[i:].data_ptr(), n,
                             H, W, 1 if with_gamma else 0, self.max_iters, float(self.rel_tol), iters, stream)
            counts += list(iters)
        # negated count (INT_MIN for zero iterations) = rel_tol not reached (include/ctrlhair_hip.h)
        self.last_iters = [0 if v == -2 ** 31 else abs(v) for v in counts]
        self.last_converged = [v >= 0 for v in counts]
        bad = [i for i, ok in enumerate(self.last_converged) if not ok]
        if bad:
            warnings.warn(f'Poisson blending of image(s) {bad} stopped after {[self.last_iters[i] for i in bad]} CG iterations '
                          f'without reaching rel_tol={self.rel_tol:g}; raise PoissonBlender.max_iters', RuntimeWarning)
        return out
