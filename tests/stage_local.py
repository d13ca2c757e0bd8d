"""Stage-LOCAL float64 parity of the single-term (f16 / bf16) SEAN generator paths, with f16x3 as the control: operand model, the packed weights as
the loader computes them, local references from the device's own taps, bounds and checker (CPU-only code: no GPU, no library;
tests/test_stage_local_model.py tests it, tests/test_hip_stage_local.py uses it on the device).

Why local: tests/stage_parity.py compares every stage with a float64 run of the whole network, and 15 to 20 convs of 8- or 11-bit operands
swamp anything one stage does wrong.  The library's taps on these paths hold exactly what the next kernel consumes -- '.hs' / '.h0' / '.h1' are
the decoded stored operand planes, '.xs' / '.dx' / the block outputs / 'fc' the f32 tensors -- so every stage is referenced from the DEVICE'S
inputs to that stage, and a fault in stage s fails stage s and no later one.

Metric, per stage s and sample b:      E(x) = max |x[b] - ref[b]| / rms(ref[b])           (stage_parity.rel_err)
  tight stage ('fc', '.xs', '.dx', '<block>', 'image'): every operand of the conv is tapped or exact, so the device sums exact products of known
      numbers in f32:                 E <= K * E32_local
  wide stage ('.hs', '.h0', '.h1'):   E <= K * (E32_local + Eq_local) + u * peak
    E32_local  E of the PyTorch f32 evaluation of the same local reference (same operands) against its float64 evaluation;
    Eq_local   E of the operand-rounded float64 reference against the same reference with nothing rounded: the whole local effect of the format
               (it covers a table row or an interior evaluation that rounds at another point, and f32-vs-f64 tie flips of the hidden activation);
    u          2^-8 (bf16), 2^-11 (f16), 0 (f16x3): one rounding of the stored output itself;   peak = max |ref| / rms(ref);
    K = 4      stage_parity.K_BOUND, for the same reason: another association of the same exact products.
Nothing measured from the library enters a bound; on f16x3 Eq_local and u vanish to f32 class (the control of the method).

What the loader does with each weight (restated here, not taken from the float64 oracle: an f64 / f32 disagreement in the spectral sigma flips about
2^-16 of the bf16 roundings, and one flipped weight is about 1e-4 of a conv output):
  conv_0 / conv_1 / conv_s   sigma = u . (W v) accumulated in double from the f32 tensors, cast to f32, w / (float) sigma in f32 (sn_read, sn_get);
                             row exponent k = 15 - frexp exponent of max |row| (sh16_row_exponent), conv_s and conv_1 on the shared-exponent rule of
                             the fused accumulator (block_convs); ldexp(w, k), rounded to the format, 2^-k undone in the epilogue;
  SPADE gamma / beta, style gamma / beta   rounded the same way, without sigma (the blend factors the loader folds in first move the rounding
                             point only: inside Eq_local);
  fc, conv_img               NOT rounded on any path: fc is an f32 label table summed per pixel (onehot_conv3x3), conv_img an f32 conv over the
                             f32 block output (conv_img_c4_kernel).  Both are therefore tight stages with f32 weights, and 'image' has no Eq / u term.
"""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from tests import sh16_emul as E
from tests import stage_parity as SP

FORMATS = ('f16', 'bf16', 'f16x3')
SIG_BITS = {'f16': 11, 'bf16': 8}
OUT_U = {'f16': 2.0 ** -11, 'bf16': 2.0 ** -8, 'f16x3': 0.0}
K_BOUND = SP.K_BOUND
IMAGE = SP.IMAGE
TIGHT, WIDE = 'tight', 'wide'


# ---- operand model ---------------------------------------------------------------------------------------------------------------
def round_operand(x, fmt, scale=1.0):
    """x (f32) as the format stores it, as f32 (exact): bf16 = round to nearest even on the f32 bit pattern (pack_A_sh16, the __bf16 conversions);
    f16 = np.float16 of x * scale with saturation, the scale undone; f16x3 = hi + lo of sh16_emul.split."""
    x = np.ascontiguousarray(x, np.float32)
    if fmt == 'bf16':
        u = x.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        return (r & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
    hi, lo = E.split(x, scale)
    v = hi if fmt == 'f16' else hi + lo
    return (v / scale).astype(np.float32)


def truncate_operand(x, fmt):
    """The planted fault: x cut toward zero to the format's significand instead of rounded (f16 / bf16)."""
    x = np.ascontiguousarray(x, np.float32)
    if fmt == 'bf16':
        return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    m, e = np.frexp(x.astype(np.float64))
    return np.ldexp(np.trunc(m * 2.0 ** SIG_BITS[fmt]) / 2.0 ** SIG_BITS[fmt], e).astype(np.float32)


def round_tensor(t, fmt, scale=1.0):
    """round_operand on a torch tensor of any floating dtype (through f32), in the tensor's dtype."""
    return torch.from_numpy(round_operand(t.detach().to(torch.float32).numpy(), fmt, scale)).to(t.dtype)


def is_representable(x, fmt):
    """Elementwise: x equals its own rounding to 11 (f16) / 8 (bf16) significant bits."""
    m, _ = np.frexp(np.asarray(x, np.float64))
    v = m * 2.0 ** SIG_BITS[fmt]
    return v == np.rint(v)


# ---- packed weights, as the loader computes them -------------------------------------------------------------------------------------
def spectral_f32(sd, prefix):
    """w / (float) sigma in f32, sigma = u . (W_mat v) accumulated in double from the f32 tensors (sean_model.cpp sn_read / sn_get)."""
    w = np.asarray(sd[prefix + '.weight_orig'], np.float32)
    u, v = np.asarray(sd[prefix + '.weight_u'], np.float64), np.asarray(sd[prefix + '.weight_v'], np.float64)
    sigma = float(u @ (w.reshape(w.shape[0], -1).astype(np.float64) @ v))
    return w / np.float32(sigma)


def row_exponents(w):
    """k [rows] with max |row| * 2^k in [2^14, 2^15); 0 for an all-zero row (net_common.h sh16_row_exponent)."""
    mx = np.abs(np.asarray(w, np.float32).reshape(w.shape[0], -1)).max(axis=1)
    _, e = np.frexp(mx)
    return np.where((mx > 0) & np.isfinite(mx), 15 - e, 0).astype(np.int64)


def shared_exponents(k1, ks):
    """(k1, ks, D) of a conv_1 / conv_s pair that shares an accumulator (block_convs): D = max (k1 - ks) clamped to +-24, ks = min(ks, k1 - D),
    k1 = ks + D -- row by row the two operands share 2^k * s_in, no row above its own optimum."""
    D = int(np.clip((k1 - ks).max(), -24, 24))
    ks = np.minimum(ks, k1 - D)
    return ks + D, ks, D


def quantize_rows(w, k, fmt, rounder=round_operand):
    """ldexp(w, k[row]) rounded to the format, the exponent undone: the value the MFMA operand stands for."""
    k = k.reshape((-1,) + (1,) * (w.ndim - 1))
    scaled = np.ldexp(np.asarray(w, np.float32), k).astype(np.float32)
    return np.ldexp(rounder(scaled, fmt), -k).astype(np.float32)


def block_conv_weights(sd, blk, fmt, rounder=round_operand):
    """{'conv_0' | 'conv_1' | 'conv_s': f32 [Cout][Cin][k][k]} of one ResBlock, quantized as packed."""
    n = blk.name
    w0, w1 = spectral_f32(sd, n + '.conv_0'), spectral_f32(sd, n + '.conv_1')
    k0, k1 = row_exponents(w0), row_exponents(w1)
    out = {}
    if blk.learned_shortcut:
        ws = spectral_f32(sd, n + '.conv_s')
        k1, ks, _ = shared_exponents(k1, row_exponents(ws))
        out['conv_s'] = quantize_rows(ws, ks, fmt, rounder)
    out['conv_0'], out['conv_1'] = quantize_rows(w0, k0, fmt, rounder), quantize_rows(w1, k1, fmt, rounder)
    return out


ACE_WEIGHTS = ('.Spade.mlp_gamma.weight', '.Spade.mlp_beta.weight', '.conv_gamma.weight', '.conv_beta.weight')


def rounded_state_dict(sd, ngf, fmt):
    """The state dict with the four conv weights of every ACE rounded (per-row exponent, no sigma); everything else as it is."""
    from ctrlhair_amd.sean import arch
    out = dict(sd)
    for a in arch.aces(ngf):
        for key in ACE_WEIGHTS:
            if a.name + key in sd:
                w = np.asarray(sd[a.name + key], np.float32)
                out[a.name + key] = quantize_rows(w, row_exponents(w), fmt)
    return out


# ---- stages ------------------------------------------------------------------------------------------------------------------------
def stage_list(ngf):
    """[(stage, type, kind of stage)] in execution order: the taps of the library and the image."""
    from ctrlhair_amd.sean import arch
    out = [('fc', TIGHT, 'fc')]
    for b in arch.blocks(ngf):
        if b.learned_shortcut:
            out += [(b.name + '.hs', WIDE, '.hs'), (b.name + '.xs', TIGHT, '.xs')]
        out += [(b.name + '.h0', WIDE, '.h0'), (b.name + '.dx', TIGHT, '.dx'), (b.name + '.h1', WIDE, '.h1'), (b.name, TIGHT, 'block')]
    return out + [(IMAGE, TIGHT, 'image')]


def _up2(x):
    return F.interpolate(x, scale_factor=2, mode='nearest')


@dataclass
class Result:
    failure: Optional[SP.Failure] = None                  # the first (stage in execution order, then sample) over its bound
    failed_stages: List[str] = field(default_factory=list)
    worst: tuple = (0.0, '', -1)                          # (max E / bound, stage, sample)
    by_type: Dict[str, float] = field(default_factory=dict)      # worst E / bound per stage type ('fc', '.hs', '.xs', '.h0', '.dx', '.h1', 'block', 'image')
    by_kind: Dict[str, float] = field(default_factory=dict)      # worst E / bound per pixel kind of the stage's level

    def merge(self, other):
        if self.failure is None:
            self.failure = other.failure
        self.failed_stages += [s for s in other.failed_stages if s not in self.failed_stages]
        self.worst = max(self.worst, other.worst)
        for mine, theirs in ((self.by_type, other.by_type), (self.by_kind, other.by_kind)):
            for k, v in theirs.items():
                mine[k] = max(mine.get(k, 0.0), v)
        return self

    def table(self):
        return ('by stage type: ' + ', '.join(f'{k} {v:.3f}' for k, v in self.by_type.items()) +
                '; by pixel kind: ' + ', '.join(f'{k} {v:.3f}' for k, v in self.by_kind.items()))


class Local:
    """The local references of one shape and format.  check() takes a full set of taps of the samples `samples` (the image under IMAGE) and
    references every stage from those taps' own predecessors."""

    def __init__(self, sd, labels, codes, noise, ngf, fmt, map_names, shared: Optional[dict] = None):
        """shared: a dict that the Local objects of one shape (same weights and inputs, another format) may share: what does not depend on
        the format -- the unrounded float64 modulation -- is then evaluated once."""
        from ctrlhair_amd.sean import arch
        from oracle import sean_oracle as O
        assert fmt in FORMATS
        self.fmt, self.ngf, self.O = fmt, ngf, O
        self.labels, self.map_names = np.asarray(labels), list(map_names)
        self.S = self.labels.shape[-1]
        self.blocks = arch.blocks(ngf)
        self.stages = stage_list(ngf)
        self.ace_index = {a.name: a.index for a in arch.aces(ngf)}
        sd32, sdq = O.to_torch(sd), O.to_torch(rounded_state_dict(sd, ngf, fmt))
        self.sd = {(torch.float32, False): sd32, (torch.float64, False): O._cast_sd(sd32, torch.float64),
                   (torch.float32, True): sdq, (torch.float64, True): O._cast_sd(sdq, torch.float64)}
        self.wq = {b.name: {k: torch.from_numpy(v) for k, v in block_conv_weights(sd, b, fmt).items()} for b in self.blocks}
        self.codes = torch.from_numpy(np.asarray(codes, np.float32))
        self.planes = O.split_noise(torch.from_numpy(np.asarray(noise, np.float32)), self.S, ngf)
        self.hooks = {'actv': lambda t: round_tensor(t, fmt, E.ACT_SCALE), 'mu': lambda t: round_tensor(t, fmt, E.ACT_SCALE)}
        self._kinds, self._mod, self._shared = {}, {}, ({} if shared is None else shared)

    # -- references ------------------------------------------------------------------------------------------------------------------
    def kinds(self, b, r):
        if (b, r) not in self._kinds:
            self._kinds[(b, r)] = SP.pixel_kinds(SP.level_labels(self.labels[b], r))[0]
        return self._kinds[(b, r)]

    def modulation(self, name, dtype, rounded):
        """(gamma, beta) [B][C][r][r] of the ACE `name` for the whole batch: they depend on the labels and the codes only, so they are evaluated
        once per (ACE, dtype, rounded or not) and shared by every run that is checked."""
        key = (name, dtype, rounded)
        store = self._mod if rounded else self._shared
        if key not in store:
            O = self.O
            blk = next(b for b in self.blocks if name.startswith(b.name + '.'))
            r, B = self.S // blk.res_div, len(self.map_names)
            C = self.sd[(dtype, rounded)][name + '.noise_var'].shape[0]
            seen = []
            hooks = dict(self.hooks) if rounded else {}
            hooks['modulation'] = lambda g, b: (seen.append((g, b)), (g, b))[1]
            O.ace(self.sd[(dtype, rounded)], name, torch.zeros(B, C, r, r, dtype=dtype), O.one_hot(torch.from_numpy(self.labels), dtype),
                  self.codes.to(dtype), torch.zeros(B, r, r, dtype=dtype), blk.styled, hooks=hooks)
            store[key] = seen[0]
        return store[key]

    def ace_ref(self, name, x, idx, dtype, rounded, act, fault=None, planes=None):
        """oracle ace (+ leaky-relu for '.h0' / '.h1') of the ACE `name` on the f32 input x [n][C][r][r] of the samples idx, in `dtype`.
        fault: callable on (gamma, beta) (planted faults of the model device)."""
        g, b = self.modulation(name, dtype, rounded)
        g, b = g[idx], b[idx]
        if fault is not None:
            g, b = fault(g, b)
        plane = (self.planes if planes is None else planes)[self.ace_index[name]][idx].to(dtype)
        y = self.O.ace(self.sd[(dtype, rounded)], name, x.to(dtype), None, None, plane, None, modulation=(g, b))
        return F.leaky_relu(y, 0.2) if act else y

    def _sources(self, stage, taps, folded):
        """What stage `stage` is computed from: ('ace', name, x, act) or ('conv', fn) with fn(dtype) the reference in that dtype."""
        prev = 'fc'
        for b in self.blocks:
            n = b.name
            if stage == n or stage.startswith(n + '.'):
                xin = _up2(taps[prev]) if b.up_before else taps[prev]
                w = self.wq[n]
                bias0 = self.sd[(torch.float32, False)][n + '.conv_0.bias']
                bias1 = self.sd[(torch.float32, False)][n + '.conv_1.bias']
                if stage == n + '.hs':
                    return ('ace', n + '.ace_s', xin, False)
                if stage == n + '.h0':
                    return ('ace', n + '.ace_0', xin, True)
                if stage == n + '.h1':
                    return ('ace', n + '.ace_1', taps[n + '.dx'], True)
                if stage == n + '.xs':
                    return ('conv', lambda dt: F.conv2d(taps[n + '.hs'].to(dt), w['conv_s'].to(dt)))
                if stage == n + '.dx':
                    return ('conv', lambda dt: F.conv2d(taps[n + '.h0'].to(dt), w['conv_0'].to(dt), bias0.to(dt), padding=1))

                def block(dt):
                    if not b.learned_shortcut:
                        sc = xin.to(dt)
                    elif folded:
                        sc = F.conv2d(taps[n + '.hs'].to(dt), w['conv_s'].to(dt))
                    else:
                        sc = taps[n + '.xs'].to(dt)
                    return sc + F.conv2d(taps[n + '.h1'].to(dt), w['conv_1'].to(dt), bias1.to(dt), padding=1)
                return ('conv', block)
            prev = n
        raise KeyError(stage)

    def references(self, stage, taps, idx, folded=False):
        """(ref64, ref32, ref64 with nothing rounded or None) of one stage from the taps (CPU f32 tensors of the samples idx)."""
        O = self.O
        sd32 = self.sd[(torch.float32, False)]
        if stage == 'fc':
            def fc(dt):
                seg = O.one_hot(torch.from_numpy(self.labels[idx]), dt)
                return F.conv2d(F.interpolate(seg, size=(self.S // 32, self.S // 32)), sd32['fc.weight'].to(dt), sd32['fc.bias'].to(dt), padding=1)
            return fc(torch.float64), fc(torch.float32), None
        if stage == IMAGE:
            def img(dt):
                x = F.leaky_relu(taps[self.blocks[-1].name], 0.2).to(dt)          # leaky-relu in f32, as the kernel applies it
                return torch.tanh(F.conv2d(x, sd32['conv_img.weight'].to(dt), sd32['conv_img.bias'].to(dt), padding=1))
            return img(torch.float64), img(torch.float32), None
        src = self._sources(stage, taps, folded)
        if src[0] == 'conv':
            return src[1](torch.float64), src[1](torch.float32), None
        _, name, x, act = src
        return (self.ace_ref(name, x, idx, torch.float64, True, act), self.ace_ref(name, x, idx, torch.float32, True, act),
                self.ace_ref(name, x, idx, torch.float64, False, act))

    # -- checker ---------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _per_sample(t, how):
        f = t.reshape(t.shape[0], -1)
        return f.mean(dim=1) if how == 'mean' else f.max(dim=1).values

    def check(self, taps, samples: Optional[Sequence[int]] = None, folded=False, only: Optional[str] = None) -> Result:
        """taps: {stage: tensor / array [n][C][h][w]} of the samples `samples` (default: all), every stage of stage_list() but the '.xs' ones when
        `folded` (no '.xs' tap: where its own rule allows it the library then adds the shortcut conv into conv_1's accumulator; either way the
        block is referenced as conv_s(hs) + conv_1(h1) + bias).  only: TIGHT / WIDE -- check the stages of that class alone (the tight ones need
        no modulation: cheap at any batch size)."""
        idx = list(range(len(self.map_names))) if samples is None else list(samples)
        got = {s: torch.as_tensor(t).detach().cpu().to(torch.float32) for s, t in taps.items()}
        res = Result()
        for stage, typ, name in self.stages:
            if (folded and name == '.xs') or (only is not None and typ != only):
                continue
            ref, ref32, refu = self.references(stage, got, idx, folded)
            g = got[stage].double()
            assert g.shape == ref.shape, (stage, g.shape, ref.shape)
            rms = self._per_sample(ref * ref, 'mean').sqrt()
            bound = K_BOUND * self._per_sample((ref32.double() - ref).abs(), 'max') / rms
            if typ == WIDE:
                rmsu = self._per_sample(refu * refu, 'mean').sqrt()
                bound = bound + K_BOUND * self._per_sample((ref - refu).abs(), 'max') / rmsu + OUT_U[self.fmt] * self._per_sample(ref.abs(), 'max') / rms
            d = torch.nan_to_num((g - ref).abs(), nan=float('inf'))
            ratio = (self._per_sample(d, 'max') / rms / bound).numpy()
            bnd = bound.numpy()
            per = (d.max(dim=1).values / (rms * bound)[:, None, None]).numpy()          # [n][h][w]: E / bound of each pixel
            for i, b in enumerate(idx):
                kinds = self.kinds(b, per.shape[-1])
                for k in range(4):
                    if (kinds == k).any():
                        res.by_kind[SP.KIND_NAMES[k]] = max(res.by_kind.get(SP.KIND_NAMES[k], 0.0), float(per[i][kinds == k].max()))
                res.by_type[name] = max(res.by_type.get(name, 0.0), float(ratio[i])) if ratio[i] == ratio[i] else float('inf')
                if not ratio[i] <= res.worst[0]:
                    res.worst = (float(ratio[i]), stage, b)
                if not ratio[i] <= 1.0:
                    if stage not in res.failed_stages:
                        res.failed_stages.append(stage)
                    if res.failure is None:
                        c, y, x = np.unravel_index(int(d[i].argmax()), d[i].shape)
                        by_kind = {SP.KIND_NAMES[k]: float(per[i][kinds == k].max() * bnd[i]) for k in range(4) if (kinds == k).any()}
                        res.failure = SP.Failure(stage, b, self.map_names[b], int(c), int(y), int(x), SP.KIND_NAMES[kinds[y, x]],
                                                 float(ratio[i] * bnd[i]), float(bnd[i]), by_kind)
        return res


# ---- the model device --------------------------------------------------------------------------------------------------------------
def conv_halves(x, w, bias=None, padding=0):
    """The conv in a second association: the input channels summed in two halves (torch f32)."""
    h = x.shape[1] // 2
    y = F.conv2d(x[:, :h], w[:, :h], None, padding=padding) + F.conv2d(x[:, h:], w[:, h:], None, padding=padding)
    return y if bias is None else y + bias.reshape(1, -1, 1, 1)


def model_device(loc: Local, sd, samples=None, folded=False, faults: Optional[dict] = None):
    """A torch-f32 forward that rounds its operands by the model above and sums every conv in two halves: the taps a correct device would give
    (the '.xs' taps left out when `folded`).  faults (each names where it is planted):
      'trunc': '<block>.conv_X'   the conv's weights cut toward zero instead of rounded;
      'swap':  '<block>.conv_X'   taps 6 and 8 swapped in the first 64 output rows of the conv;
      'gamma': '<ace>'            gamma zeroed on the last column of the ACE;
      'noise': '<ace>'            the ACE's noise plane transposed;
      'lo':    '<block>.h0'       the tap carries hi + lo while the conv reads hi (f16)."""
    faults = faults or {}
    O, fmt = loc.O, loc.fmt
    idx = list(range(len(loc.map_names))) if samples is None else list(samples)
    f32 = torch.float32
    sd32 = loc.sd[(f32, False)]
    taps = {}
    seg = O.one_hot(torch.from_numpy(loc.labels[idx]), f32)
    x = F.conv2d(F.interpolate(seg, size=(loc.S // 32, loc.S // 32)), sd32['fc.weight'], sd32['fc.bias'], padding=1)
    taps['fc'] = x

    def zero_last_column(g, b):
        g = g.clone()
        g[..., -1] = 0
        return g, b

    def ace(name, xin, act):
        fault = zero_last_column if faults.get('gamma') == name else None
        planes = None
        if faults.get('noise') == name:
            planes = list(loc.planes)
            planes[loc.ace_index[name]] = planes[loc.ace_index[name]].transpose(1, 2).contiguous()
        return round_tensor(loc.ace_ref(name, xin, idx, f32, True, act, fault=fault, planes=planes), fmt, E.ACT_SCALE)

    def conv(blk, which, xin, bias, padding):
        cname = f'{blk.name}.{which}'
        w = loc.wq[blk.name][which]
        if faults.get('trunc') == cname:
            w = torch.from_numpy(block_conv_weights(sd, blk, fmt, lambda a, f, *_: truncate_operand(a, f))[which])
        y = conv_halves(xin, w, bias, padding)
        if faults.get('swap') == cname:
            ws = w.clone()
            ws[:, :, 2, 0], ws[:, :, 2, 2] = w[:, :, 2, 2], w[:, :, 2, 0]
            y[:, :, :64] = conv_halves(xin, ws, bias, padding)[:, :, :64]
        return y

    for b in loc.blocks:
        n = b.name
        xin = _up2(x) if b.up_before else x
        if b.learned_shortcut:
            hs = ace(n + '.ace_s', xin, False)
            taps[n + '.hs'] = hs
            xs = conv(b, 'conv_s', hs, None, 0)
            if not folded:
                taps[n + '.xs'] = xs
        else:
            xs = xin
        h0 = ace(n + '.ace_0', xin, True)
        taps[n + '.h0'] = h0
        if faults.get('lo') == n + '.h0':                                # the conv reads hi, the tap shows hi + lo
            full = loc.ace_ref(n + '.ace_0', xin, idx, f32, True, True)
            taps[n + '.h0'] = round_tensor(full, 'f16x3', E.ACT_SCALE)
        dx = conv(b, 'conv_0', h0, sd32[n + '.conv_0.bias'], 1)
        taps[n + '.dx'] = dx
        h1 = ace(n + '.ace_1', dx, True)
        taps[n + '.h1'] = h1
        x = xs + conv(b, 'conv_1', h1, sd32[n + '.conv_1.bias'], 1)
        taps[n] = x
    taps[IMAGE] = torch.tanh(conv_halves(F.leaky_relu(x, 0.2), sd32['conv_img.weight'], sd32['conv_img.bias'], 1))
    return taps
