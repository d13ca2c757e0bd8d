"""Stage-by-stage float64 parity of the SEAN generator: label maps, pixel kinds, the F(4x4,3x3) rounding model, the bound and the checker
(CPU-only code: no GPU, no library; tests/test_stage_parity_model.py tests it, tests/test_hip_stage_parity.py uses it on the device).

Metric, per stage s and sample b:            E(x) = max |x[b] - ref64[b]| / rms(ref64[b])
Bound:                                       bound(s, b) = K * (E32(s, b) + e4 * uses_f4),   K = 4
  E32     E of the PyTorch f32 oracle's tap against the float64 run of the same oracle (oracle/sean_oracle.py, dtype argument);
  e4      E of the f32 model below of ONE F(4x4,3x3) conv (conv_wino4.h's matrices and order of operations) on N(0, 1) data with
          N(0, 1 / (9 C)) weights, at the largest channel count C of an F(4x4) layer of the shape; counted on the paths that run them;
  K = 4   the device sums the same products in another association (MFMA k-chains, split-K, table rows), and 15 to 20 convs feed the
          last stage: independent per-conv errors add as the square root of their count.
Nothing measured from the library enters the bound."""
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

K_BOUND = 4.0
INTERIOR, EDGE, FRAME, CONV = 0, 1, 2, 3
KIND_NAMES = ('interior', 'straight-edge', 'frame', 'boundary-conv')
PAIR_CODES = 2 * 19 * 19 * 4            # ace_sparse.h ACE_PAIR_CODES: the frame codes follow the straight-edge codes

MAP_NAMES = ('one_region', 'ring3', 'ring4', 'band255', 'noclass', 'face', 'stripes5', 'diag', 'offgrid')


# ---- label maps ------------------------------------------------------------------------------------------------------------------
def _ring(S, width, inner=13, ring=4):
    lab = np.full((S, S), ring, np.uint8)
    lab[width:S - width, width:S - width] = inner
    return lab


def offgrid_labels(S):
    """Rectangles of labels whose borders lie off every grid the kernels tile by: at x, y = 1, 2 and 3 mod 4 (quads, F(4x4) tiles), at 31, 33, 63
    and 65 (32-pixel tiles; 129, 191, 193 from 160 pixels on: the 128-pixel block column) -- corners, T-junctions (merged cells) and straight
    edges across quad, tile and 128 x 8 block boundaries; the first border at 2: a rectangle corner within 2 pixels of the image corner."""
    cuts = [c for c in (2, 31, 33, 63, 65, 90, 107, 121, 129, 150, 191, 193, 222, 239) if c <= S - 6]
    assert {c % 4 for c in cuts} == {1, 2, 3}
    edges = [0] + cuts + [S]
    n = len(edges) - 1
    cell = (3 * np.arange(n)[:, None] + 5 * np.arange(n)[None, :]) % 19          # neighbours differ by 3 or 5 (mod 19): never equal
    for i in range(1, n - 1, 3):                                                  # merged pairs of cells: T-junctions
        j = (2 * i) % (n - 1)
        cell[i, j + 1] = cell[i, j]
    for j in range(2, n - 1, 3):
        i = (2 * j + 1) % (n - 1)
        cell[i + 1, j] = cell[i, j]
    lab = np.empty((S, S), np.uint8)
    for i in range(n):
        for j in range(n):
            lab[edges[i]:edges[i + 1], edges[j]:edges[j + 1]] = cell[i, j]
    return lab


def label_map(name, S):
    """One label map [S][S] uint8: the sets of tests/test_hip_frame_rows.py and tests/test_hip_sparse_ace.py (first sample), rebuilt, and `offgrid`."""
    from ctrlhair_amd import procedural as P
    if name == 'one_region':
        return np.full((S, S), 13, np.uint8)
    if name == 'ring3':
        return _ring(S, 3)
    if name == 'ring4':
        return _ring(S, 4)
    if name == 'band255':
        lab = np.full((S, S), 7, np.uint8)
        lab[:, S // 2:S // 2 + 2] = 255
        return lab
    if name == 'noclass':
        lab = P.blocky_labels(1, S, grid=4, seed=77)[0].copy()
        lab[: S // 2, : S // 2] = 255
        lab[S // 2:, S // 2:] = 19
        return lab
    if name == 'face':
        return P.face_like_labels(S, 40)
    if name == 'stripes5':
        return np.repeat(((np.arange(S) // 5) % 19).astype(np.uint8)[None, :], S, 0)
    if name == 'diag':
        return (np.add.outer(np.arange(S), np.arange(S)) % 19).astype(np.uint8)
    if name == 'offgrid':
        return offgrid_labels(S)
    raise KeyError(name)


def label_batch(S, names: Sequence[str] = MAP_NAMES):
    return np.stack([label_map(n, S) for n in names])


def level_labels(lab, r):
    """Labels of the level of r pixels: F.interpolate(..., mode='nearest') of the one-hot (normalization.py:115) = every (S / r)-th pixel."""
    k = lab.shape[-1] // r
    assert k * r == lab.shape[-1]
    return lab[..., ::k, ::k]


# ---- pixel kinds (ace_sparse.h / ace_classify_kernel, restated) ------------------------------------------------------------------
def pixel_kinds(lab):
    """kind [H][W] (INTERIOR / EDGE / FRAME / CONV) and code [H][W] (-1: none) of one label map at its own resolution, options sean.edge and
    sean.frame on:
      interior       label < 19 and the whole 5x5 window inside the image and equal to it;
      straight-edge  else: window inside, five uniform columns (orientation 0, tried first) or rows (1) A^s B^(5-s), s = 1..4, A != B, both < 19;
                     code = ((o * 19 + A) * 19 + B) * 4 + (s - 1);
      frame          else: label A < 19, window cut by the image along exactly ONE axis, every in-image label of it equal to A;
                     code = 2888 + (o * 19 + A) * 4 + (s - 1), lines OUTSIDE^s A^(5-s) (s = 1, 2: left / top) or A^s OUTSIDE^(5-s) (s = 3, 4);
      boundary-conv  everything else."""
    H, W = lab.shape
    OUT = 1000
    P = np.full((H + 4, W + 4), OUT, np.int32)
    P[2:-2, 2:-2] = lab
    win = np.lib.stride_tricks.sliding_window_view(P, (5, 5))                    # [H][W][dy][dx]
    c = lab.astype(np.int32)
    kind = np.full((H, W), CONV, np.int8)
    code = np.full((H, W), -1, np.int32)
    interior = (c < 19) & (win == c[:, :, None, None]).all(axis=(2, 3))
    kind[interior] = INTERIOR
    taken = interior.copy()
    for o in (0, 1):
        v = win if o == 0 else win.transpose(0, 1, 3, 2)                        # v[i][j]: line j along the split direction
        l = v[:, :, 0, :]                                                       # [H][W][5]
        A, Bl = l[..., 0], l[..., 4]
        ok = (v == l[:, :, None, :]).all(axis=(2, 3)) & (A < 19) & (Bl < 19) & (A != Bl)
        isA = l == A[..., None]
        ok &= (isA | (l == Bl[..., None])).all(axis=-1) & (isA[..., :-1] >= isA[..., 1:]).all(axis=-1)
        s = isA.sum(axis=-1)
        ok &= ~taken
        kind[ok] = EDGE
        code[ok] = (((o * 19 + A) * 19 + Bl) * 4 + (s - 1))[ok]
        taken |= ok
    y, x = np.mgrid[0:H, 0:W]
    cl, cr = np.maximum(2 - x, 0), np.maximum(x + 3 - W, 0)
    rt, rb = np.maximum(2 - y, 0), np.maximum(y + 3 - H, 0)
    one_axis = ((cl + cr) != 0) != ((rt + rb) != 0)
    one_axis &= (cl * cr == 0) & (rt * rb == 0)
    same = ((win == c[:, :, None, None]) | (win == OUT)).all(axis=(2, 3))
    fr = ~taken & (c < 19) & one_axis & same
    o = np.where((cl + cr) != 0, 0, 1)
    lead, trail = np.where(o == 1, rt, cl), np.where(o == 1, rb, cr)
    s = np.where(lead != 0, lead, 5 - trail)
    kind[fr] = FRAME
    code[fr] = (PAIR_CODES + (o * 19 + c) * 4 + (s - 1))[fr]
    return kind, code


def decode(code):
    """(frame, o, A, B, s) of a code (ace_code_decode)."""
    s = (code & 3) + 1
    if code >= PAIR_CODES:
        r = (code - PAIR_CODES) >> 2
        return True, r // 19, r % 19, r % 19, s
    return False, (code >> 2) // 361, ((code >> 2) // 19) % 19, (code >> 2) % 19, s


def boundary_quads(kind):
    """Number of 2 x 2 quads with a boundary-conv pixel: what the gather conv lists (conv_wino.h)."""
    H, W = kind.shape
    q = (kind == CONV).reshape(H // 2, 2, W // 2, 2).any(axis=(1, 3))
    return int(q.sum())


# ---- F(4x4,3x3) rounding model (conv_wino4.h) ------------------------------------------------------------------------------------
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)


def _fma(a, b, c):
    """fmaf(a, b, c) for a small-integer constant a: one rounding (the product is exact in double, the sum's double rounding is far below f32's)."""
    if b.dtype == np.float64:
        return a * b + c
    return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(b.dtype)


def _in1d(d):
    """wino4_in1d on axis 0 (six lines): rows of B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]."""
    d0, d1, d2, d3, d4, d5 = d
    a, b = _fma(-4.0, d2, d4), _fma(-4.0, d1, d3)
    c, t = d4 - d2, d3 - d1
    return np.stack([_fma(4.0, d0, _fma(-5.0, d2, d4)), a + b, a - b, _fma(2.0, t, c), _fma(-2.0, t, c), _fma(4.0, d1, _fma(-5.0, d3, d5))])


def _out1d(m):
    """wino4_out1d on axis 0: rows of A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 0; 0 1 -1 8 -8 1]."""
    m0, m1, m2, m3, m4, m5 = m
    s1, d1, s2, d2 = m1 + m2, m1 - m2, m3 + m4, m3 - m4
    return np.stack([m0 + s1 + s2, _fma(2.0, d2, d1), _fma(4.0, s2, s1), _fma(8.0, d2, d1) + m5])


def wino4_model(x, w, dtype):
    """One zero-padded 3x3 conv as conv_wino4.h evaluates it: U = G g G^T in double, rounded once to `dtype` (pack_wino4_A); V = B^T d B by
    wino4_in1d along x then along y, M accumulated over the channels in their order (the MFMA's k-chain; product and sum rounded separately
    here: an upper model of the fused chain), Y = A^T M A by wino4_out1d along i then along j -- all in `dtype`.  x [C][H][W], w [K][C][3][3],
    H, W multiples of 4."""
    C, H, W = x.shape
    Kc, th, tw = w.shape[0], H // 4, W // 4
    U = np.einsum('ia,kcab,jb->ijkc', G4, w.astype(np.float64), G4).astype(dtype)          # [6][6][K][C]
    xp = np.zeros((C, H + 2, W + 2), dtype)
    xp[:, 1:-1, 1:-1] = x
    d = np.empty((6, 6, C, th, tw), dtype)                                                 # [patch row][patch column]
    for i in range(6):
        for j in range(6):
            d[i, j] = xp[:, i:i + 4 * th:4, j:j + 4 * tw:4]
    V = _in1d(_in1d(d.transpose(1, 0, 2, 3, 4)).transpose(1, 0, 2, 3, 4))                   # along x, then along y: [i][j][C][th][tw]
    M = np.zeros((6, 6, Kc, th, tw), dtype)
    for c in range(C):
        M += U[:, :, :, c][:, :, :, None, None] * V[:, :, c][:, :, None]
    Y = _out1d(_out1d(M).transpose(1, 0, 2, 3, 4)).transpose(1, 0, 2, 3, 4)                 # along i, then along j: [4][4][K][th][tw]
    return np.ascontiguousarray(Y.transpose(2, 3, 0, 4, 1)).reshape(Kc, H, W)


def direct_model(x, w, dtype):
    """The same conv as a sequential sum over (channel, tap) in `dtype`."""
    C, H, W = x.shape
    xp = np.zeros((C, H + 2, W + 2), dtype)
    xp[:, 1:-1, 1:-1] = x
    out = np.zeros((w.shape[0], H, W), dtype)
    wd = w.astype(dtype)
    for c in range(C):
        for t in range(9):
            out += wd[:, c, t // 3, t % 3][:, None, None] * xp[c, t // 3:t // 3 + H, t % 3:t % 3 + W][None]
    return out


def rel_err(x, ref):
    """E(x) of the module docstring for one sample."""
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(x, np.float64) - ref).max() / np.sqrt(np.mean(ref * ref)))


_e4_cache: Dict[int, tuple] = {}


def e4(C, with_direct=False):
    """E of the f32 F(4x4,3x3) model against float64 on N(0, 1) data [C][32][32] and N(0, 1 / (9 C)) weights [16][C][3][3] (seeded: a constant
    of C); with_direct: also E of the sequential direct f32 sum."""
    if C not in _e4_cache:
        rng = np.random.default_rng(4000 + C)
        x = rng.standard_normal((C, 32, 32))
        w = rng.standard_normal((16, C, 3, 3)) / np.sqrt(9 * C)
        x32, w32 = x.astype(np.float32), w.astype(np.float32)
        ref = direct_model(x32.astype(np.float64), w32.astype(np.float64), np.float64)      # of the SAME (f32-representable) operands
        _e4_cache[C] = (rel_err(wino4_model(x32, w32, np.float32), ref), rel_err(direct_model(x32, w32, np.float32), ref))
    return _e4_cache[C] if with_direct else _e4_cache[C][0]


def f4_channels(ngf, S):
    """Largest contraction length of a layer that can run as F(4x4,3x3) at this shape (0: none), by the library's own conditions:
      * ResBlock convs conv_0 (fin channels) / conv_1 (fmid) of a level of r pixels with r % 32 == 0, channels % 8 == 0 and >= 16 (conv_wino4.h
        wino4_supported; sean_model.cpp);
      * SPADE gamma / beta convs of the levels r % 32 == 0, r <= 64 (option sean.wino4_ace): the 128 hidden channels, and the 19 one-hot planes of the
        style term behind them on a styled ACE (conv_wino4.h wino4_ace_kernel).
    A level off the 32 grid never takes F(4x4): at ngf 24, S 160 only the 160-pixel level counts (48 and 24 channels)."""
    from ctrlhair_amd.sean import arch
    cs = [0]
    for b in arch.blocks(ngf):
        r = S // b.res_div
        if r < 32 or r % 32:
            continue
        cs += [c for c in (b.fin, b.fmid) if c % 8 == 0 and c >= 16]
        if r <= 64:
            cs.append(arch.SPADE_HIDDEN + (arch.LABEL_NC if b.styled else 0))
    return max(cs)


# ---- references and checker ------------------------------------------------------------------------------------------------------
IMAGE = 'image'


def oracle_pair(sd, labels, codes, noise, ngf):
    """(taps64, taps32) of the oracle, the image under IMAGE, in execution order."""
    from oracle import sean_oracle as O
    out = []
    for dt in (torch.float64, torch.float32):
        taps = {}
        img = O.generator_forward(O.to_torch(sd), labels, codes, noise, ngf, taps=taps, dtype=dt)
        taps[IMAGE] = img
        assert all(t.dtype == dt for t in taps.values())
        out.append(taps)
    return out[0], out[1]


@dataclass
class Failure:
    stage: str
    sample: int
    map: str
    c: int
    y: int
    x: int
    kind: str
    E: float
    bound: float
    by_kind: Dict[str, float]          # worst E of that (stage, sample) per pixel kind present

    def __str__(self):
        per = ', '.join(f'{k} {v:.2e}' for k, v in self.by_kind.items())
        return (f'stage {self.stage}, sample {self.sample} ({self.map}): E = {self.E:.3e} > bound {self.bound:.3e} at (c, y, x) = '
                f'({self.c}, {self.y}, {self.x}), a {self.kind} pixel of its level; worst E per kind: {per}')


class Reference:
    """The float64 taps of one shape with rms and E32 per (stage, sample); check() compares any set of taps with them.  device: where the
    comparison runs (the taps to compare are moved there)."""

    def __init__(self, taps64, taps32, labels, map_names, device='cpu'):
        self.stages: List[str] = list(taps64)
        self.labels, self.map_names, self.device = np.asarray(labels), list(map_names), torch.device(device)
        self.ref = {s: t.to(self.device) for s, t in taps64.items()}
        self.rms = {s: self._per_sample(t * t, 'mean').sqrt() for s, t in self.ref.items()}
        self.E32 = {s: self._per_sample((taps32[s].to(self.device).double() - self.ref[s]).abs(), 'max') / self.rms[s] for s in self.stages}
        self._kinds = {}

    @staticmethod
    def _per_sample(t, how):
        f = t.reshape(t.shape[0], -1)
        return f.mean(dim=1) if how == 'mean' else f.max(dim=1).values

    def kinds(self, b, r):
        if (b, r) not in self._kinds:
            self._kinds[(b, r)] = pixel_kinds(level_labels(self.labels[b], r))[0]
        return self._kinds[(b, r)]

    def bound(self, stage, e4_term=0.0):
        """[B] bound of the stage: K (E32 + e4 * uses_f4)."""
        return K_BOUND * (self.E32[stage] + e4_term)

    def check(self, got, e4_term=0.0, samples: Optional[Sequence[int]] = None, stages: Optional[Sequence[str]] = None):
        """got: {stage: tensor / array [n][C][h][w]} for the samples `samples` of the batch (default: all).  Returns (failure, worst): the first
        (stage in execution order, then sample) with E > bound or E not finite as a Failure, or None; worst = (max E / bound, stage, sample)."""
        idx = list(range(len(self.map_names))) if samples is None else list(samples)
        sel = torch.as_tensor(idx, device=self.device)
        failure, worst = None, (0.0, '', -1)
        for s in (self.stages if stages is None else stages):
            g = torch.as_tensor(got[s]).to(self.device).double()
            ref = self.ref[s][sel]
            assert g.shape == ref.shape, (s, g.shape, ref.shape)
            d = (g - ref).abs()
            E = self._per_sample(d, 'max') / self.rms[s][sel]
            bnd = self.bound(s, e4_term)[sel]
            ratio = (E / bnd).cpu().numpy()
            for i, b in enumerate(idx):
                if not ratio[i] <= worst[0]:
                    worst = (float(ratio[i]), s, b)
                if failure is None and not ratio[i] <= 1.0:
                    failure = self._failure(s, b, d[i], float(E[i]), float(bnd[i]), float(self.rms[s][b]))
        return failure, worst

    def _failure(self, s, b, d, E, bnd, rms):
        d = torch.nan_to_num(d, nan=float('inf')).cpu().numpy()
        c, y, x = np.unravel_index(int(d.argmax()), d.shape)
        kinds = self.kinds(b, d.shape[-1])
        per = d.max(axis=0) / rms
        by_kind = {KIND_NAMES[k]: float(per[kinds == k].max()) for k in range(4) if (kinds == k).any()}
        return Failure(s, b, self.map_names[b], int(c), int(y), int(x), KIND_NAMES[kinds[y, x]], E, bnd, by_kind)
