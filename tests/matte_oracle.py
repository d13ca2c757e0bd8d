"""Host oracle of the matte paste-back (test code only): ch_face_unalign_matte's specification (include/ctrlhair_hip.h) restated in
numpy float64.  Window sums are differences of two-dimensional cumulative sums -- integer ones for the 13 moments, so those are
exact -- with nothing of the kernels' strips, segments or running sums.  The geometry, the Lanczos taps and the composite are those of
tests/unalign_oracle.py, by import.  `moments='f32'` forms the window means in float32 and subtracts (E[Ip] - E[I]E[p]): the variant
the design rejected, kept to pin the reason (tests/test_matte.py)."""
import numpy as np

from tests import unalign_oracle as UO


def box(v, r):
    """Sums of v [H,W,...] over the windows [Y - r, Y + r] x [X - r, X + r] clipped to the array; keeps v's dtype."""
    H, W = v.shape[:2]
    c = np.zeros((H + 1, W + 1) + v.shape[2:], v.dtype)
    c[1:, 1:] = v.cumsum(0).cumsum(1)
    y0, y1 = np.clip(np.arange(H) - r, 0, H), np.clip(np.arange(H) + r + 1, 0, H)
    x0, x1 = np.clip(np.arange(W) - r, 0, W), np.clip(np.arange(W) + r + 1, 0, W)
    return c[y1][:, x1] - c[y0][:, x1] - c[y1][:, x0] + c[y0][:, x0]


def raw_weight(weight, x, y, S):
    """Step 1: weight[clamp(floor(y))][clamp(floor(x))] inside the quad, 0 outside; x, y float64 arrays -> int64."""
    inside = np.minimum(np.minimum(x, S - x), np.minimum(y, S - y)) > 0
    i = np.clip(np.floor(x).astype(np.int64), 0, S - 1)
    j = np.clip(np.floor(y).astype(np.int64), 0, S - 1)
    return np.where(inside, np.asarray(weight).astype(np.int64)[j, i], 0)


def moments(I8, p8, r):
    """Step 2: n [H,W], sum p [H,W], sum I [H,W,3], sum I p [H,W,3], sum I I^T [H,W,3,3], all int64 and exact."""
    H, W = p8.shape
    I, p = I8.astype(np.int64), p8.astype(np.int64)
    n = box(np.ones((H, W), np.int64), r)
    sII = box((I[..., :, None] * I[..., None, :]).reshape(H, W, 9), r).reshape(H, W, 3, 3)
    return n, box(p, r), box(I, r), box(I * p[..., None], r), sII


def coefficients(I8, p8, r, eps, moments_mode='int'):
    """Step 3: a float64 [H,W,3], b float64 [H,W] before their rounding to float32."""
    H, W = p8.shape
    n, sp, sI, sIp, sII = moments(I8, p8, r)
    if moments_mode == 'int':
        den = n.astype(np.float64) ** 2 * 65025.0
        cov = (n[..., None, None] * sII - sI[..., :, None] * sI[..., None, :]).astype(np.float64) / den[..., None, None]
        cIp = (n[..., None] * sIp - sI * sp[..., None]).astype(np.float64) / den[..., None]
        mI, mp = sI / (255.0 * n)[..., None], sp / (255.0 * n)
    else:                                             # float32 window means of a guide scaled to [0, 1], then the subtraction
        f = np.float32
        I, p = I8.astype(f) / f(255), p8.astype(f) / f(255)
        nf = n.astype(f)
        mI, mp = box(I, r) / nf[..., None], box(p, r) / nf
        mIp = box(I * p[..., None], r) / nf[..., None]
        mII = box((I[..., :, None] * I[..., None, :]).reshape(H, W, 9), r).reshape(H, W, 3, 3) / nf[..., None, None]
        cov = (mII - mI[..., :, None] * mI[..., None, :]).astype(np.float64)
        cIp = (mIp - mI * mp[..., None]).astype(np.float64)
        mI, mp = mI.astype(np.float64), mp.astype(np.float64)
    a = np.linalg.solve(cov + eps * np.eye(3), cIp[..., None])[..., 0]
    b = mp - (a[..., 0] * mI[..., 0] + a[..., 1] * mI[..., 1] + a[..., 2] * mI[..., 2])
    return a, b


def guided_matte(I8, p8, r, eps, moments_mode='int'):
    """Steps 2-4 on a domain: I8 uint8 [H,W,3] (the guide), p8 integer [H,W] in [0, 255] -> m float32 [H,W]."""
    I8, p8 = np.asarray(I8), np.asarray(p8)
    a, b = coefficients(I8, p8, r, eps, moments_mode)
    a, b = a.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
    n = box(np.ones(p8.shape, np.int64), r).astype(np.float64)
    ma, mb = box(a, r) / n[..., None], box(b, r) / n
    I = I8 / 255.0
    q = ma[..., 0] * I[..., 0] + ma[..., 1] * I[..., 1] + ma[..., 2] * I[..., 2] + mb
    return np.clip(q, 0.0, 1.0).astype(np.float32)


def paste_back_matte(photo, edits, plan_u, weight, feather_px, radius, eps, moments_mode='int', chunk=1 << 15):
    """photo uint8 [H,W,3], edits uint8 [N,S,S,3] (or [S,S,3]), plan_u = alignment.unalign_plan's dict, weight uint8 [S,S] ->
    (out uint8 [N,H,W,3], alpha float32 [bh,bw] over the plan's bbox)."""
    photo, edits = np.asarray(photo), np.asarray(edits)
    edits = edits[None] if edits.ndim == 3 else edits
    N, S = edits.shape[0], int(plan_u['output_size'])
    assert edits.shape[1:] == (S, S, 3) and np.asarray(weight).shape == (S, S)
    feather_px = S / 16.0 if feather_px is None else float(feather_px)
    A = np.asarray(plan_u['A'], np.float64)
    x0, y0, x1, y1 = plan_u['bbox']
    Y, X = np.mgrid[y0:y1, x0:x1]
    x, y = UO.crop_coordinates(A, X, Y)
    m = guided_matte(photo[y0:y1, x0:x1], raw_weight(weight, x, y, S), int(radius), float(eps), moments_mode)
    ramp = UO.alpha_map(x.ravel(), y.ravel(), S, feather_px, None, np.float32).reshape(m.shape)
    alpha = (m * ramp).astype(np.float32)                                    # step 5, float32 like the kernel

    fs = max(1.0, float(plan_u['scale']))
    nt = int(np.floor(6.0 * fs)) + 1
    out = np.repeat(photo[None], N, axis=0)
    X, Y, x, y, af = X.ravel(), Y.ravel(), x.ravel(), y.ravel(), alpha.ravel().astype(np.float64)
    live = np.nonzero(af > 0)[0]
    ef = edits.astype(np.float64)
    for s in range(0, live.size, chunk):                                     # the composite of unalign_oracle.paste_back, float64
        k = live[s:s + chunk]
        ix, wx = UO._axis_weights(x[k], S, fs, nt, np.float64)
        iy, wy = UO._axis_weights(y[k], S, fs, nt, np.float64)
        w2 = wy[:, :, None] * wx[:, None, :]
        w2 = w2 / w2.sum(axis=(1, 2), keepdims=True)
        a = af[k][:, None]
        p = photo[Y[k], X[k]].astype(np.float64)
        for n in range(N):
            taps = ef[n][iy[:, :, None], ix[:, None, :]]
            e = (w2[..., None] * taps).sum(axis=(1, 2))
            out[n, Y[k], X[k]] = np.clip(np.floor(a * e + (1.0 - a) * p + 0.5), 0, 255).astype(np.uint8)
    return out, alpha
