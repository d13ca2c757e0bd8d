"""Host oracle of the paste-back (test code only): ch_face_unalign's specification (include/ctrlhair_hip.h) restated in numpy, float64,
pixel by pixel with the full two-dimensional tap matrix of every pixel -- no separable passes, no tiles, nothing of the kernel's loop
structure.  `dtype=np.float32` runs the same per-pixel arithmetic in float32 (coordinates stay float64, as in the specification): the
CPU estimate of how many pixels a float32 evaluation moves across a rounding boundary.  `shift` displaces the map on purpose, for
the tests that need a known-wrong geometry to compare with."""
import numpy as np


def lanczos3(t):
    """L(t) = sinc(t) sinc(t / 3) inside |t| < 3, 0 outside (np.sinc is sin(pi t) / (pi t)); keeps t's dtype."""
    return np.where(np.abs(t) < 3, np.sinc(t) * np.sinc(t / t.dtype.type(3)), t.dtype.type(0))


def crop_coordinates(A, X, Y):
    """(x, y) = A (X + 0.5, Y + 0.5, 1) in float64, summed left to right (the order the ABI fixes)."""
    Xc, Yc = np.asarray(X, np.float64) + 0.5, np.asarray(Y, np.float64) + 0.5
    return (A[0, 0] * Xc + A[0, 1] * Yc) + A[0, 2], (A[1, 0] * Xc + A[1, 1] * Yc) + A[1, 2]


def alpha_map(x, y, S, feather_px, weight=None, dtype=np.float64):
    m = np.minimum(np.minimum(x, S - x), np.minimum(y, S - y))
    if feather_px > 0:
        a = np.clip(m.astype(dtype) / dtype(feather_px), 0, 1).astype(dtype)
        a[m <= 0] = 0
    else:
        a = (m > 0).astype(dtype)
    if weight is not None:
        w = np.asarray(weight).astype(dtype)
        u, v = x.astype(dtype) - dtype(0.5), y.astype(dtype) - dtype(0.5)
        fu, fv = np.floor(u), np.floor(v)
        du, dv = u - fu, v - fv
        i0, i1 = np.clip(fu.astype(np.int64), 0, S - 1), np.clip(fu.astype(np.int64) + 1, 0, S - 1)
        j0, j1 = np.clip(fv.astype(np.int64), 0, S - 1), np.clip(fv.astype(np.int64) + 1, 0, S - 1)
        top = w[j0, i0] + (w[j0, i1] - w[j0, i0]) * du
        bot = w[j1, i0] + (w[j1, i1] - w[j1, i0]) * du
        a = a * ((top + (bot - top) * dv) / dtype(255))
    return a


def _axis_weights(c, S, fs, nt, dtype):
    """Tap indices [P,nt] and weights [P,nt] (0 for taps outside the support or outside [0, S)) of coordinates c [P]."""
    i0 = np.floor(c - 3.0 * fs - 0.5).astype(np.int64) + 1
    idx = i0[:, None] + np.arange(nt)[None, :]
    d = (idx + 0.5) - c[:, None]
    valid = (np.abs(d) < 3.0 * fs) & (idx >= 0) & (idx < S)
    w = lanczos3(d.astype(dtype) / dtype(fs)) * valid
    return np.clip(idx, 0, S - 1), w.astype(dtype)


def paste_back(photo, edits, plan_u, weight=None, feather_px=None, dtype=np.float64, shift=(0.0, 0.0), chunk=1 << 15,
               return_alpha=False):
    """photo uint8 [H,W,3], edits uint8 [N,S,S,3] (or [S,S,3]), plan_u = alignment.unalign_plan's dict -> uint8 [N,H,W,3]
    (and, with return_alpha, alpha [H,W] in `dtype`, 0 outside bbox)."""
    photo = np.asarray(photo)
    edits = np.asarray(edits)
    edits = edits[None] if edits.ndim == 3 else edits
    H, W = photo.shape[:2]
    N, S = edits.shape[0], int(plan_u['output_size'])
    assert edits.shape[1:] == (S, S, 3)
    feather_px = S / 16.0 if feather_px is None else float(feather_px)
    A = np.asarray(plan_u['A'], np.float64)
    x0, y0, x1, y1 = plan_u['bbox']
    fs = max(1.0, float(plan_u['scale']))
    nt = int(np.floor(6.0 * fs)) + 1
    out = np.repeat(photo[None], N, axis=0)
    alpha_full = np.zeros((H, W), dtype)
    Y, X = np.mgrid[y0:y1, x0:x1]
    X, Y = X.ravel(), Y.ravel()
    x, y = crop_coordinates(A, X, Y)
    x, y = x + shift[0], y + shift[1]
    alpha = alpha_map(x, y, S, feather_px, weight, dtype)
    alpha_full[Y, X] = alpha
    live = np.nonzero(alpha > 0)[0]
    ef = edits.astype(dtype)
    for s in range(0, live.size, chunk):
        k = live[s:s + chunk]
        ix, wx = _axis_weights(x[k], S, fs, nt, dtype)
        iy, wy = _axis_weights(y[k], S, fs, nt, dtype)
        w2 = wy[:, :, None] * wx[:, None, :]                             # [P,nt,nt], every tap of every pixel
        w2 = w2 / w2.sum(axis=(1, 2), keepdims=True, dtype=dtype)
        a = alpha[k][:, None]
        p = photo[Y[k], X[k]].astype(dtype)
        for n in range(N):
            taps = ef[n][iy[:, :, None], ix[:, None, :]]                  # [P,nt,nt,3]
            e = (w2[..., None] * taps).sum(axis=(1, 2), dtype=dtype)
            v = np.floor(a * e + (dtype(1) - a) * p + dtype(0.5))
            out[n, Y[k], X[k]] = np.clip(v, 0, 255).astype(np.uint8)
    return (out, alpha_full) if return_alpha else out
