"""Finding editing directions for a model: random candidates, batched slider sweeps, contact sheets and scores.

The reference finds the "used directions" of its shape latent (16-d) and texture latent (8-d) by hand
(shape_branch/script_find_direction.py, color_texture_branch/script_find_direction.py, util/find_semantic_direction.py): it draws
300 random unit vectors orthogonal to the directions already in use, and for each one renders 10 dataset images at 6 slider values
-- one set_input_img and six batch-1 output() calls per image -- into one PNG grid (util/canvas_grid.py) for a person to look at.

Here the images are analysed once (`DirectionSearch`), a candidate is a batch of latent moves and one batched render
(`DirectionSearch.sweep`), the grid is pasted together on the device (`ContactSheet`, ch_sheet_compose) and every render is
measured there as exact integers (`SweepStats`, ch_sweep_stats), from which `score` ranks the candidates on the host: a person
opens the twenty sheets at the top of scores.json, not three hundred.  `find_directions` is the job
(`python -m ctrlhair_amd.dataset directions`), writing the reference's files:
    <out>/<att>_dir_<k+1>/<i>.pkl    pickled float32 torch tensor [dim] (what hair_editor.py:82-119 loads from *_dir_used)
    <out>/<att>_<k+1>/<i>.png        the contact sheet of candidate i
    <out>/scores.json                one record per candidate, sorted by `effect`, largest first
with k the number of directions already in use.
"""
import json
import os
import pickle
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import hostutil as U
from . import lib as _lib
from .devop import DeviceOp

NSTAT = 16                          # CH_SWEEP_STATS
DIMS = {'shape': 16, 'texture': 8}  # shape_branch/config.py hair_dim, color_texture_branch/config.py noise_dim
KIND_FLOAT, KIND_U8, KIND_LABELS = 0, 1, 2


# ---- candidates (CPU torch) ------------------------------------------------------------------------------------------------
def random_direction(dim: int, existing: Sequence, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """util/find_semantic_direction.py:12-21: randn(dim), minus its projection on each existing direction in turn, flipped so that
    d[0] >= 0, normalised.  With torch.Generator().manual_seed(s) it equals the reference under torch.manual_seed(s) bit for bit."""
    d = torch.randn(dim, generator=generator)
    for e in existing:
        e = torch.as_tensor(np.asarray(e) if not isinstance(e, torch.Tensor) else e).float().cpu()
        d = d - torch.dot(d, e) * e
    if d[0] < 0:
        d = -d
    return d / d.norm()


def _mix32(x: int) -> int:
    """A bijection of 32-bit integers (xor-shift / multiply rounds)."""
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def candidate_direction(dim: int, existing: Sequence, seed: int, index: int) -> torch.Tensor:
    """Candidate `index` of the search with `seed`: a pure function of its arguments (its generator is seeded from (seed, index)),
    so a candidate is the same vector whichever rank draws it and whatever was drawn before.  torch's CPU generator keeps 32 bits
    of a seed, so the pair is folded into 32 bits, one-to-one in `index` for a given `seed`."""
    if not 0 <= index < 1 << 32 or not 0 <= seed < 1 << 32:
        raise ValueError(f'seed {seed} / index {index} out of range')
    return random_direction(dim, existing, torch.Generator().manual_seed(_mix32(int(index) ^ _mix32(int(seed)))))


def mask_lut(draw_type: int) -> np.ndarray:
    """hostutil.mask_to_rgb's colour table of a draw type: uint8 [256,3] (labels 19..254 black, 255 white)."""
    return np.ascontiguousarray(U.mask_to_rgb(np.arange(256, dtype=np.uint8)[None], draw_type=draw_type)[0])


# ---- device side ---------------------------------------------------------------------------------------------------------------
def _image_kind(t: torch.Tensor, what: str) -> int:
    if t.dtype == torch.float32 and t.dim() == 4 and t.shape[1] == 3:
        return KIND_FLOAT
    if t.dtype == torch.uint8 and t.dim() == 4 and t.shape[3] == 3:
        return KIND_U8
    raise ValueError(f'{what}: expected float32 [n,3,H,W] or uint8 [n,H,W,3], got {t.dtype} {tuple(t.shape)}')


def sheet_png_distances(cols: int, W: int, margin: int) -> tuple:
    """The match distances to give the PNG encoder for a sheet of `cols` columns of W pixels, `margin` apart: the column pitch in bytes,
    (W + margin) * 3, at which the renders of one row repeat each other outside the edited region.  Empty for a one-column sheet and
    for a pitch beyond deflate's window (32767)."""
    pitch = (int(W) + int(margin)) * 3
    return (pitch,) if cols > 1 and pitch <= 32767 else ()


class ContactSheet(DeviceOp):
    """util/canvas_grid.py Canvas on the device: uint8 [rows * H, cols * W + margin * (cols - 1), 3], filled with 255."""

    def __init__(self, handle: _lib.Handle, device, rows: int, cols: int, cell, margin: int = 0):
        super().__init__(handle, device)
        self.H, self.W = (int(cell), int(cell)) if isinstance(cell, (int, np.integer)) else (int(cell[0]), int(cell[1]))
        self.rows, self.cols, self.margin = int(rows), int(cols), int(margin)
        if min(self.rows, self.cols, self.H, self.W) < 1 or self.margin < 0:
            raise ValueError('ContactSheet: rows, cols and the cell size must be positive, margin >= 0')
        self.canvas = torch.full((self.rows * self.H, self.cols * self.W + self.margin * (self.cols - 1), 3), 255,
                                 dtype=torch.uint8, device=self.device)
        self._luts: Dict[int, torch.Tensor] = {}

    def draw(self, src: torch.Tensor, cells, kind: Optional[int] = None, draw_type: Optional[int] = None) -> 'ContactSheet':
        """Paste src[s] into cell cells[s] = (row, column).  src: float32 [n,3,Hs,Ws] in [-1,1] (kind 0), uint8 [n,Hs,Ws,3] (kind 1),
        or, with draw_type, uint8 label maps [n,Hs,Ws] coloured as hostutil.mask_to_rgb(draw_type) (kind 2).  A source of another
        size than the cell is nearest-mapped (cv2 INTER_NEAREST).  A cell outside the grid raises."""
        if draw_type is not None:
            if kind not in (None, KIND_LABELS):
                raise ValueError('draw: draw_type goes with label maps (kind 2)')
            kind = KIND_LABELS
            if src.dtype != torch.uint8 or src.dim() != 3:
                raise ValueError(f'draw: label maps must be uint8 [n,Hs,Ws], got {src.dtype} {tuple(src.shape)}')
            Hs, Ws = int(src.shape[1]), int(src.shape[2])
            lut = self._luts.get(draw_type)
            if lut is None:
                lut = self._luts[draw_type] = torch.from_numpy(mask_lut(draw_type)).to(self.device)
        else:
            found = _image_kind(src, 'draw')
            if kind is not None and kind != found:
                raise ValueError(f'draw: kind {kind} does not fit {src.dtype} {tuple(src.shape)}')
            kind, lut = found, None
            Hs, Ws = (int(src.shape[2]), int(src.shape[3])) if kind == KIND_FLOAT else (int(src.shape[1]), int(src.shape[2]))
        cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
        n = int(src.shape[0])
        if len(cells) != n:
            raise ValueError(f'draw: {n} sources but {len(cells)} cells')
        if n == 0:
            return self
        bad = (cells[:, 0] < 0) | (cells[:, 0] >= self.rows) | (cells[:, 1] < 0) | (cells[:, 1] >= self.cols)
        if bad.any():
            raise ValueError(f'draw: cell {tuple(cells[bad][0])} outside the {self.rows} x {self.cols} grid')
        src = src.to(self.device).contiguous()
        cells_dev = torch.from_numpy(cells.astype(np.int32)).to(self.device)
        self.handle.call('ch_sheet_compose', src.data_ptr(), kind, n, Hs, Ws, cells_dev.data_ptr(),
                         lut.data_ptr() if lut is not None else None, self.canvas.data_ptr(), self.rows, self.cols, self.H, self.W,
                         self.margin, self._stream())
        return self

    def numpy(self) -> np.ndarray:
        return U.to_host(self.canvas)

    def png_distances(self) -> tuple:
        """`distances` for pngenc.PngEncoder on this sheet's canvas: the column pitch in bytes (sheet_png_distances)."""
        return sheet_png_distances(self.cols, self.W, self.margin)


class SweepStats(DeviceOp):
    """ch_sweep_stats on one ch_handle: exact per-render measurements (column layout: include/ctrlhair_hip.h, CH_SWEEP_STATS)."""

    def measure(self, images: torch.Tensor, labels: torch.Tensor, ref) -> torch.Tensor:
        """images float32 [N,3,H,W] in [-1,1] or uint8 [N,H,W,3]; labels uint8 [N,h,w] (nearest-mapped to H x W); ref: per render
        the index of the render it is compared with, or -1 (host integers, checked here, or an int32 device tensor).
        -> int64 [N,16] device tensor."""
        kind = _image_kind(images, 'measure')
        N = int(images.shape[0])
        H, W = (int(images.shape[2]), int(images.shape[3])) if kind == KIND_FLOAT else (int(images.shape[1]), int(images.shape[2]))
        if labels.dtype != torch.uint8 or labels.dim() != 3 or labels.shape[0] != N:
            raise ValueError(f'measure: labels must be uint8 [{N},h,w], got {labels.dtype} {tuple(labels.shape)}')
        if isinstance(ref, torch.Tensor) and ref.is_cuda:
            ref_dev = ref.to(torch.int32).contiguous()
        else:
            r = np.asarray(ref.cpu() if isinstance(ref, torch.Tensor) else ref, dtype=np.int64).reshape(-1)
            if len(r) != N or (r >= N).any() or (r < -1).any():
                raise ValueError(f'measure: ref must hold {N} entries in -1..{N - 1}')
            ref_dev = torch.from_numpy(r.astype(np.int32)).to(self.device)
        if ref_dev.numel() != N:
            raise ValueError(f'measure: ref must hold {N} entries')
        images, labels = images.to(self.device).contiguous(), labels.to(self.device).contiguous()
        out = torch.empty(N, NSTAT, dtype=torch.int64, device=self.device)
        self.handle.call('ch_sweep_stats', images.data_ptr(), kind, labels.data_ptr(), ref_dev.data_ptr(), N, H, W,
                         int(labels.shape[1]), int(labels.shape[2]), out.data_ptr(), self._stream())
        return out


def to_u8(x: torch.Tensor) -> torch.Tensor:
    """float32 [n,3,H,W] in [-1,1] -> uint8 [n,H,W,3], the arithmetic of EditPipeline.edit_blended / ch_sheet_compose kind 0."""
    return (x * 127.5 + 127.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


class DirectionSearch:
    """Sweeps of arbitrary directions over a fixed set of images on an EditPipeline.  The constructor does everything that does not
    depend on the candidate once: parsing, the latent representation, the colour terms of an edit without sliders, the decoded input
    masks (what Backend.set_input_img shows) and one set of noise planes per image (all values of an image share it, as
    Backend.outputs does with pinned planes)."""

    def __init__(self, pipeline, imgs: torch.Tensor, noise_seed: int = 0):
        p = self.pipeline = pipeline
        gen = p.models.generator
        self.device = p.device
        self.handle = gen.handle
        self.max_batch = max(1, int(gen.max_batch))
        imgs = imgs.to(self.device).float().contiguous()
        if imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[2] != imgs.shape[3] or imgs.shape[-1] != p.img_size:
            raise ValueError(f'DirectionSearch: imgs must be [I,3,{p.img_size},{p.img_size}], got {tuple(imgs.shape)}')
        self.imgs, self.I, self.S = imgs, int(imgs.shape[0]), int(imgs.shape[-1])
        parts = []
        for a in range(0, self.I, self.max_batch):
            x = imgs[a:a + self.max_batch]
            parts.append(p.analyse(x, p.parse(x)))
        lat = {k: torch.cat([q[k] for q in parts], dim=0) for k in parts[0]}
        self.lat = p.apply_sliders(lat, {})                                    # adds 'hsv' / 'rgb': Backend.output's colour terms
        mg = p.models.mask_generator
        self.input_masks = torch.cat([mg.decode_labels(self.lat['shape'][a:a + self.max_batch], self.lat['face'][a:a + self.max_batch])
                                      for a in range(0, self.I, self.max_batch)], dim=0)   # [I,256,256]
        self.noise = gen.draw_noise(self.I, self.S, seed=noise_seed)
        self.stats_fn = SweepStats(self.handle, self.device)
        self.resizer = p.models.color_stats

    def latents(self, att: str, direction, values) -> torch.Tensor:
        """[I,V,dim]: cur + (val - cur . d) d for every image and value (Backend.continue_change_with_direction)."""
        if att not in DIMS:
            raise ValueError(f"att must be 'shape' or 'texture', got {att!r}")
        d = torch.as_tensor(np.asarray(direction.cpu() if isinstance(direction, torch.Tensor) else direction)).float().to(self.device)
        if tuple(d.shape) != (DIMS[att],):
            raise ValueError(f'a {att} direction has {DIMS[att]} entries, got {tuple(d.shape)}')
        cur = self.lat[att]
        return torch.stack([cur + (float(v) - cur @ d)[:, None] * d[None] for v in values], dim=1)

    def sweep(self, att: str, direction, values):
        """Render every image at every slider value of `direction` -> (images [I,V,3,S,S] in [-1,1], masks uint8 [I,V,256,256]) on the
        device.  One batched render per chunk of the pipeline's max_batch renders.  A texture sweep keeps the input's decoded mask (the
        shape decoder is not run again: the masks of a row are the same map)."""
        values = [float(v) for v in values]
        I, V, S = self.I, len(values), self.S
        moved = self.latents(att, direction, values).reshape(I * V, -1)
        rep = lambda t: t.repeat_interleave(V, dim=0)
        lat = {k: rep(self.lat[k]) for k in ('shape', 'face', 'codes', 'pca_std', 'texture', 'curliness', 'rgb')}
        lat[att] = moved
        noise = rep(self.noise)
        fixed = rep(self.input_masks) if att == 'texture' else None
        images = torch.empty(I * V, 3, S, S, dtype=torch.float32, device=self.device)
        masks = torch.empty(I * V, 256, 256, dtype=torch.uint8, device=self.device)
        for a in range(0, I * V, self.max_batch):
            b = min(a + self.max_batch, I * V)
            _, m = self.pipeline.render({k: v[a:b] for k, v in lat.items()}, noise=noise[a:b], out=images[a:b],
                                        mask=None if fixed is None else fixed[a:b])
            masks[a:b] = m
        return images.view(I, V, 3, S, S), masks.view(I, V, 256, 256)

    def sheet(self, att: str, images: torch.Tensor, masks: torch.Tensor, cell: Optional[int] = None, margin: int = 0) -> ContactSheet:
        """The reference's contact sheet of one candidate.  texture: I rows x (V + 1) columns, column 0 the input image
        (color_texture_branch/script_find_direction.py:61-73).  shape: 2 I rows, image rows and mask rows interleaved; column 0 of a
        mask row is the input's decoded mask with draw type 1 (what set_input_img returns), the other mask cells draw type 2
        (shape_branch/script_find_direction.py:61-75).  cell: side of a cell in pixels (default the image size); smaller cells are
        cv2-bilinear resizes of the uint8 images (ch_resize_linear_u8), label maps are always nearest-mapped."""
        I, V, S = int(images.shape[0]), int(images.shape[1]), self.S
        cell = S if cell is None else int(cell)
        step = 2 if att == 'shape' else 1
        sheet = ContactSheet(self.handle, self.device, step * I, V + 1, cell, margin)
        in_cells = [(step * i, 0) for i in range(I)]
        out_cells = [(step * i, v + 1) for i in range(I) for v in range(V)]
        flat = images.reshape(I * V, 3, S, S)
        if cell == S:
            sheet.draw(self.imgs[:I], in_cells)
            sheet.draw(flat, out_cells)
        else:
            sheet.draw(self.resizer.resize(to_u8(self.imgs[:I]), cell), in_cells)
            sheet.draw(self.resizer.resize(to_u8(flat), cell), out_cells)
        if att == 'shape':
            sheet.draw(self.input_masks[:I], [(2 * i + 1, 0) for i in range(I)], draw_type=1)
            sheet.draw(masks.reshape(I * V, 256, 256), [(2 * i + 1, v + 1) for i in range(I) for v in range(V)], draw_type=2)
        return sheet

    def stats(self, images: torch.Tensor, masks: torch.Tensor) -> np.ndarray:
        """int64 [I,V,16] (host): every render measured against the first value of its row."""
        I, V = int(images.shape[0]), int(images.shape[1])
        ref = np.repeat(np.arange(I) * V, V)
        out = self.stats_fn.measure(images.reshape(I * V, *images.shape[2:]), masks.reshape(I * V, *masks.shape[2:]), ref)
        return U.to_host(out).reshape(I, V, NSTAT)


# ---- scores (host, float64 from the exact integers) ------------------------------------------------------------------------------
def _slope(x: np.ndarray, y: np.ndarray) -> float:
    """Least-squares slope of y against x over the finite entries of y (0 with fewer than two)."""
    ok = np.isfinite(y)
    if ok.sum() < 2:
        return 0.0
    x, y = x[ok] - x[ok].mean(), y[ok]
    den = float((x * x).sum())
    return float((x * (y - y.mean())).sum() / den) if den > 0 else 0.0


def score(att: str, stats, values, H: int, W: int) -> Dict[str, float]:
    """Scores of one candidate from its int64 [I,V,16] measurements (ref = the row's first value); every entry is a mean over the
    images.
      effect      shape: labels changed between the first and the last value / (H W); texture: mean absolute colour change per channel
                  inside the hair of either render, first against last value (0 where neither has hair)
      monotone    share of adjacent value steps at which that statistic does not fall
      shape:      area, length, centroid_x, centroid_y: least-squares slopes against the slider value of hair area / (H W), the lowest
                  hair row, and the hair centroid (renders without hair are left out)
      texture:    colour_drift: largest channel difference of the mean hair colour between the first and the last value -- a texture
                  direction that moves the colour is entangled with the colour sliders"""
    if att not in DIMS:
        raise ValueError(f"att must be 'shape' or 'texture', got {att!r}")
    s = np.asarray(stats, dtype=np.int64)
    if s.ndim != 3 or s.shape[2] != NSTAT or s.shape[1] != len(values):
        raise ValueError(f'score: stats must be [I,{len(values)},{NSTAT}], got {s.shape}')
    x = np.asarray(values, dtype=np.float64)
    f = s.astype(np.float64)
    if att == 'shape':
        stat = f[:, :, 12] / float(H * W)
    else:
        stat = np.divide(f[:, :, 14], 3.0 * f[:, :, 15], out=np.zeros_like(f[:, :, 14]), where=s[:, :, 15] > 0)
    out = {'effect': float(stat[:, -1].mean()),
           'monotone': float((np.diff(stat, axis=1) >= 0).mean()) if s.shape[1] > 1 else 1.0}
    has = s[:, :, 0] > 0
    cnt = np.where(has, f[:, :, 0], 1.0)
    if att == 'shape':
        nan = np.full_like(cnt, np.nan)
        series = {'area': f[:, :, 0] / float(H * W), 'length': np.where(has, f[:, :, 6], nan),
                  'centroid_x': np.where(has, f[:, :, 1] / cnt, nan), 'centroid_y': np.where(has, f[:, :, 2] / cnt, nan)}
        for k, y in series.items():
            out[k] = float(np.mean([_slope(x, row) for row in y]))
    else:
        mean = f[:, :, 9:12] / cnt[:, :, None]
        both = has[:, 0] & has[:, -1]
        drift = np.where(both, np.abs(mean[:, -1] - mean[:, 0]).max(axis=1), 0.0)
        out['colour_drift'] = float(drift.mean())
    return out


# ---- the job ---------------------------------------------------------------------------------------------------------------------
def load_used(used_dir: Optional[str]) -> List[np.ndarray]:
    """The directions in use: every pickle of `used_dir` in sorted order, as checkpoints reads *_dir_used ([] without a folder)."""
    from .checkpoints import _load_dirs
    return _load_dirs(used_dir) if used_dir else []


class _AsTensor:
    """Pickles as `torch.from_numpy(array)`: loads as a torch tensor, like the reference's files, but with the same bytes every time
    (pickle.dump(tensor) embeds a storage key taken from a memory address)."""

    def __init__(self, array: np.ndarray):
        self.array = array

    def __reduce__(self):
        return torch.from_numpy, (self.array,)


def write_direction(path: str, direction) -> None:
    """The reference's file (script_find_direction.py:57-58): pickle.load gives a float32 torch tensor [dim]."""
    a = direction.detach().cpu().numpy() if isinstance(direction, torch.Tensor) else np.asarray(direction)
    with open(path, 'wb') as f:
        pickle.dump(_AsTensor(np.ascontiguousarray(a, dtype=np.float32)), f, protocol=4)


def write_png(path: str, rgb: np.ndarray) -> None:
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(rgb, dtype=np.uint8)).save(path)


def parse_sheets(spec: str):
    """'all' | 'none' | 'top:K' -> ('all' | 'none' | 'top', K)."""
    if spec in ('all', 'none'):
        return spec, 0
    if spec.startswith('top:') and spec[4:].isdigit() and int(spec[4:]) > 0:
        return 'top', int(spec[4:])
    raise ValueError(f"--sheets must be all, none or top:K, got {spec!r}")


def find_directions(search: DirectionSearch, att: str, existing: Sequence, out_dir: str, n: int = 300, values=None, seed: int = 0,
                    rank: int = 0, world: int = 1, sheets: str = 'all', cell: Optional[int] = None, png: str = 'host',
                    png_stride: bool = False) -> List[dict]:
    """This rank's candidates (round-robin over 0..n-1) of a direction search: direction pickle, contact sheet and scores per
    candidate.  sheets: 'all', 'none', or 'top:K' -- score every candidate of the rank first, then render only the rank's K best
    again into sheets (PNG encoding is host zlib and, at full size, the largest single cost per candidate).  png: 'host' downloads
    the sheet and writes it with Pillow (`write_png`); 'device' encodes it where it is (pngenc.PngEncoder) and downloads the
    compressed bytes: the same pixels in another file.  png_stride (with png='device' only): the encoder also matches at the
    sheet's column pitch (`ContactSheet.png_distances`), where the columns of a row repeat each other: a smaller file.  Writes
    <out_dir>/scores.rank<r>of<world>.json and returns its records; `merge_scores(out_dir, world)` makes scores.json from the files of
    that world's ranks (files an earlier run with another world size left behind are not read)."""
    from .dataset import shard
    from .pngenc import PngEncoder, check_png_mode
    if png_stride and check_png_mode(png) != 'device':
        raise ValueError("png_stride needs png='device': Pillow's writer takes no match distances")
    encoder = PngEncoder(search.handle, search.device) if check_png_mode(png) == 'device' else None
    mode, top = parse_sheets(sheets)
    values = np.linspace(-2.5, 2.5, 6) if values is None else np.asarray(values, dtype=np.float64)
    k = len(existing) + 1
    dir_dir, img_dir = os.path.join(out_dir, '%s_dir_%d' % (att, k)), os.path.join(out_dir, '%s_%d' % (att, k))
    for d in (dir_dir, img_dir):
        os.makedirs(d, exist_ok=True)
    S = search.S

    def run(idx, want_sheet, want_score):
        d = candidate_direction(DIMS[att], existing, seed, idx)
        images, masks = search.sweep(att, d, values)
        rec = None
        if want_score:
            write_direction(os.path.join(dir_dir, '%d.pkl' % idx), d)
            rec = {'index': int(idx), **score(att, search.stats(images, masks), values, S, S)}
        if want_sheet:
            sheet = search.sheet(att, images, masks, cell=cell)
            if encoder is None:
                write_png(os.path.join(img_dir, '%d.png' % idx), sheet.numpy())
            else:
                kw = {'distances': sheet.png_distances()} if png_stride else {}
                encoder.write([os.path.join(img_dir, '%d.png' % idx)], sheet.canvas[None], **kw)
        return rec

    mine = shard(list(range(n)), rank, world)
    records = [run(i, mode == 'all', True) for i in mine]
    if mode == 'top':
        for rec in sorted(records, key=lambda r: (-r['effect'], r['index']))[:top]:
            run(rec['index'], True, False)
    with open(os.path.join(out_dir, 'scores.rank%03dof%03d.json' % (rank, world)), 'w') as f:
        json.dump(records, f)
    return records


def merge_scores(out_dir: str, world: int = 1) -> List[dict]:
    """scores.json from scores.rank<r>of<world>.json of the ranks 0..world-1: one record per candidate, sorted by effect (largest
    first, then index).  A missing rank's file raises; files of runs with another world size are left alone."""
    records = []
    for rank in range(world):
        with open(os.path.join(out_dir, 'scores.rank%03dof%03d.json' % (rank, world))) as f:
            records += json.load(f)
    records.sort(key=lambda r: (-r['effect'], r['index']))
    with open(os.path.join(out_dir, 'scores.json'), 'w') as f:
        json.dump(records, f, indent=1)
    return records


def use_direction(out_dir: str, att: str, index: int, used_dir: str) -> str:
    """Copy candidate `index` of the search over `used_dir` into the used set under the next free name (NN.pkl, the layout
    checkpoints.write_reference_layout writes).  Returns the new path."""
    import shutil
    k = len(load_used(used_dir))
    src = os.path.join(out_dir, '%s_dir_%d' % (att, k + 1), '%d.pkl' % index)
    if not os.path.exists(src):
        raise FileNotFoundError(f'{src}: no such candidate (searches are numbered by the size of the used set, here {k})')
    os.makedirs(used_dir, exist_ok=True)
    while os.path.exists(os.path.join(used_dir, '%02d.pkl' % k)):
        k += 1
    dst = os.path.join(used_dir, '%02d.pkl' % k)
    shutil.copyfile(src, dst)
    return dst
