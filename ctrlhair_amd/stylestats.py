"""Median style codes of a dataset on the HIP library: the fallback rows `gen_img` uses for regions absent from a portrait.

The reference (sean_codes/get_mean_code.py) collects every style code the Zencoder produced, and for each of the 19 regions keeps the
medoid: the code whose summed Euclidean distance to all codes of that region is smallest (hair_editor.py:130-168 reads the rows back
as mean_style_code/median/<i>/ACE.npy).  It builds the full N x N float32 distance matrix from the Gram identity
|a|^2 + |b|^2 - 2 a.b, which needs tens of GB per region at dataset scale and cancels badly on tanh-saturated codes.

Here `ch_style_medoid` (include/ctrlhair_hip.h) evaluates the distances in difference form, tile by tile, without storing the matrix,
for all 19 regions in one call.  A code counts for region j iff its row j is not all-zero -- the convention for an absent region
(hair_editor.py `_obj_dic`).  The host part of this module (presence, compaction, file formats) needs no GPU; StyleMedoid does, and
there is no CPU fallback.
"""
import ctypes as C
import os
from typing import Optional

import numpy as np

from .devop import DeviceOp

N_REGIONS, STYLE_LEN = 19, 512
PACKAGED = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'mean_style_code.npz')
NPZ_KEYS = ('mean', 'median')


# ---- host logic (no GPU) ---------------------------------------------------------------------------------------------------------
def as_code_array(codes):
    """[N,19,512] array / tensor, or the {key: [19,512]} dict of sean_code_dict.pkl -> (float32 [N,19,512], keys or None)."""
    keys = None
    if isinstance(codes, dict):
        keys = list(codes)
        codes = np.stack([np.asarray(codes[k], np.float32) for k in keys]) if keys else np.zeros((0, N_REGIONS, STYLE_LEN), np.float32)
    elif hasattr(codes, 'detach'):
        codes = codes.detach().cpu().numpy()
    a = np.ascontiguousarray(codes, dtype=np.float32)
    if a.ndim != 3 or a.shape[1] != N_REGIONS or a.shape[2] % 4 != 0 or a.shape[2] == 0:
        raise ValueError(f'expected style codes [N,{N_REGIONS},{STYLE_LEN}], got {a.shape}')
    return a, keys


def presence(codes: np.ndarray) -> np.ndarray:
    """bool [N,19]: image n has region j iff codes[n, j] is not all-zero."""
    return (np.asarray(codes) != 0).any(axis=2)


def compact(codes: np.ndarray):
    """float32 [N,19,D] -> (rows float32 [total,D]: region 0's present codes in input order, then region 1's, ...;
    seg_offsets int64 [20]; source int64 [total]: the input index of every row)."""
    pres = presence(codes)
    rows, source, offsets = [], [], [0]
    for j in range(codes.shape[1]):
        idx = np.nonzero(pres[:, j])[0]
        rows.append(codes[idx, j])
        source.append(idx)
        offsets.append(offsets[-1] + len(idx))
    return (np.ascontiguousarray(np.concatenate(rows, axis=0), dtype=np.float32), np.asarray(offsets, np.int64),
            np.concatenate(source).astype(np.int64))


def load_mean_style_code(path: Optional[str] = None) -> dict:
    """Read a mean_style_code .npz (None = the packaged one) -> {'mean', 'median'}: float32 [19,512].  ValueError on a file with other
    keys, dtypes or shapes."""
    with np.load(path if path is not None else PACKAGED) as z:
        if sorted(z.files) != sorted(NPZ_KEYS):
            raise ValueError(f'{path}: expected the keys {sorted(NPZ_KEYS)}, found {sorted(z.files)}')
        out = {k: z[k] for k in NPZ_KEYS}
    for k, v in out.items():
        if v.shape != (N_REGIONS, STYLE_LEN) or v.dtype != np.float32:
            raise ValueError(f'{path}: {k!r} is {v.dtype} {v.shape}, expected float32 {(N_REGIONS, STYLE_LEN)}')
    return out


def finish(codes: np.ndarray, offsets: np.ndarray, source: np.ndarray, index: np.ndarray, mean: np.ndarray, keys=None) -> dict:
    """The result dict of median_style_codes from the device's answers (index within the segment, mean per segment).  A region no
    image has keeps the packaged row for both median and mean, with index -1 and count 0."""
    count = np.diff(offsets).astype(np.int64)
    fallback = load_mean_style_code() if (count == 0).any() else None
    R, D = codes.shape[1], codes.shape[2]
    med, avg, idx = np.empty((R, D), np.float32), np.empty((R, D), np.float32), np.full(R, -1, np.int64)
    for j in range(R):
        if count[j] == 0:
            if D != STYLE_LEN:
                raise ValueError(f'region {j} is absent everywhere and the packaged rows have {STYLE_LEN} values, not {D}')
            med[j], avg[j] = fallback['median'][j], fallback['mean'][j]
        else:
            idx[j] = source[offsets[j] + int(index[j])]
            med[j], avg[j] = codes[idx[j], j], mean[j]
    return {'median': med, 'mean': avg, 'index': idx, 'count': count, 'keys': keys}


def save_mean_style_code(path: str, result: dict) -> None:
    """Write result['mean'] / result['median'] as an .npz with the packaged file's keys and dtypes."""
    arrs = {k: np.ascontiguousarray(result[k], dtype=np.float32) for k in NPZ_KEYS}
    for k, v in arrs.items():
        if v.shape != (N_REGIONS, STYLE_LEN):
            raise ValueError(f'{k!r} is {v.shape}, expected {(N_REGIONS, STYLE_LEN)}')
    with open(path, 'wb') as f:                    # a file object: np.savez would append '.npz' to a bare name
        np.savez(f, **arrs)


def write_reference_tree(dir_name: str, result: dict) -> None:
    """The reference's layout: <dir>/mean_style_code/{mean,median}/<i>/ACE.npy, float32 [512] each (hair_editor.py:130-147)."""
    for kind in NPZ_KEYS:
        for i in range(N_REGIONS):
            d = os.path.join(dir_name, 'mean_style_code', kind, str(i))
            os.makedirs(d, exist_ok=True)
            np.save(os.path.join(d, 'ACE.npy'), np.ascontiguousarray(result[kind][i], dtype=np.float32))


def read_reference_tree(dir_name: str) -> dict:
    """Inverse of write_reference_tree."""
    return {kind: np.stack([np.load(os.path.join(dir_name, 'mean_style_code', kind, str(i), 'ACE.npy')) for i in range(N_REGIONS)])
            for kind in NPZ_KEYS}


# ---- device side -----------------------------------------------------------------------------------------------------------------
class StyleMedoid(DeviceOp):
    """ch_style_medoid on one ch_handle.  No CPU fallback: the constructor needs the library and a GPU."""

    def segments(self, rows, seg_offsets, n_split: int = 0, want_sums: bool = True):
        """rows float32 [total, dim] (numpy is uploaded), seg_offsets int64 [R+1] -> device tensors (index int32 [R], sums float64
        [total] or None, mean float32 [R, dim])."""
        import torch
        x = rows if isinstance(rows, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32))
        x = x.to(self.device).float().contiguous()
        off = np.ascontiguousarray(seg_offsets, dtype=np.int64)
        if x.dim() != 2 or off.ndim != 1 or len(off) < 2 or off[0] != 0 or off[-1] != x.shape[0] or (np.diff(off) < 0).any():
            raise ValueError(f'rows {tuple(x.shape)} and seg_offsets {off.tolist()[:8]}... do not match')
        R, dim = len(off) - 1, int(x.shape[1])
        op = off.ctypes.data_as(C.c_void_p)
        need = int(self.handle.lib.ch_style_medoid_workspace_bytes(op, R, dim, int(n_split)))
        if need == 0:
            raise ValueError(f'ch_style_medoid rejects R={R}, dim={dim}, n_split={n_split} (dim must be a multiple of 4)')
        ws = self._buffer('_ws', need)
        index = torch.empty(R, dtype=torch.int32, device=self.device)
        sums = torch.empty(int(off[-1]), dtype=torch.float64, device=self.device) if want_sums else None
        mean = torch.empty(R, dim, dtype=torch.float32, device=self.device)
        self.handle.call('ch_style_medoid', x.data_ptr(), op, R, dim, int(n_split), index.data_ptr(),
                         sums.data_ptr() if sums is not None else None, mean.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        return index, sums, mean

    def median_style_codes(self, codes) -> dict:
        """[N,19,512] float32 (numpy or torch) or a sean_code_dict -> {'median' [19,512], 'mean' [19,512], 'index' int64 [19] into
        the input order (-1: no image has the region), 'count' int64 [19], 'keys' (the dict's keys, else None)}: one ABI call
        with R = 19."""
        a, keys = as_code_array(codes)
        rows, off, source = compact(a)
        index, _, mean = self.segments(rows, off, want_sums=False)
        return finish(a, off, source, index.cpu().numpy(), mean.cpu().numpy(), keys)


def median_style_codes(codes, handle=None, device=None) -> dict:
    """StyleMedoid(handle, device).median_style_codes(codes)."""
    return StyleMedoid(handle, device).median_style_codes(codes)
