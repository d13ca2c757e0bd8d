"""Host oracle of the mask warp (test infrastructure; numpy / scipy only).

ARAP in float64 with a sparse direct solve (the per-element energy libigl uses for 2-D triangles:
E(U, R) = sum_t sum_{(i,j) in t} w_ij^t |(u_i - u_j) - R_t (v_i - v_j)|^2, w = cot(opposite angle) / 2), then the raster,
edge fix, sampling and compose in float32 in the reference's operation order (mesh_core.cpp:17-73,150-215,
triangle_wrap_hair.py:77-85, get_pixelValue.py:24-51, mask_adaptor.py:63-73,119-143).  numpy's float32 element-wise
arithmetic is IEEE and unfused, which is what `g++ -O2` makes of mesh_core.cpp on x86-64."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

CANVAS, IMG, BG, EXT, HAIR = 672, 512, 80, 10, 13
f32 = np.float32


def cot_weights(V, F):
    """[m,3]: w[t,k] = cot(angle at corner k of triangle t) / 2 -- the weight of the edge opposite corner k."""
    V = np.asarray(V, np.float64)
    P = V[F]                                        # [m,3,2]
    w = np.zeros((len(F), 3))
    for k in range(3):
        a, b = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
        cross = np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])
        dot = (a * b).sum(1)
        w[:, k] = np.where(cross != 0, 0.5 * dot / np.where(cross != 0, cross, 1), 0.0)
    return w


def _edges(F):
    """Per triangle the three directed edges (i, j) = (corner k+1, corner k+2), opposite corner k: [m,3] each."""
    return F[:, [1, 2, 0]], F[:, [2, 0, 1]]


def fit_rotations(V, F, w, U):
    I, J = _edges(F)
    eu, ev = U[I] - U[J], V[I] - V[J]               # [m,3,2]
    a = (w * (eu * ev).sum(-1)).sum(1)
    b = (w * (eu[..., 1] * ev[..., 0] - eu[..., 0] * ev[..., 1])).sum(1)
    n = np.hypot(a, b)
    c = np.where(n > 0, a / np.where(n > 0, n, 1), 1.0)
    s = np.where(n > 0, b / np.where(n > 0, n, 1), 0.0)
    return c, s


def energy(V, F, w, U, c, s):
    I, J = _edges(F)
    eu, ev = U[I] - U[J], V[I] - V[J]
    rx = c[:, None] * ev[..., 0] - s[:, None] * ev[..., 1]
    ry = s[:, None] * ev[..., 0] + c[:, None] * ev[..., 1]
    return float((w * ((eu[..., 0] - rx) ** 2 + (eu[..., 1] - ry) ** 2)).sum())


def arap(V, F, b, bc, iters=100, return_energy=False):
    """igl::arap_precomputation + arap_solve from U = V (my_arap.cpp:181-187), float64.  -> U [n,2] (and the energy after each
    local step and after each global step, interleaved, when return_energy)."""
    V = np.asarray(V, np.float64)
    F = np.asarray(F, np.int64)
    b = np.asarray(b, np.int64)
    bc = np.asarray(bc, np.float64)
    n = len(V)
    w = cot_weights(V, F)
    I, J = _edges(F)
    i, j, ww = I.ravel(), J.ravel(), w.ravel()
    L = sp.coo_matrix((np.concatenate([ww, ww, -ww, -ww]), (np.concatenate([i, j, i, j]), np.concatenate([i, j, j, i]))),
                      shape=(n, n)).tocsr()
    free = np.setdiff1d(np.arange(n), b)
    U = V.copy()
    U[b] = bc
    solve = spla.factorized(L[free][:, free].tocsc()) if len(free) else None
    Lfc = L[free][:, b]
    E = []
    for _ in range(iters):
        c, s = fit_rotations(V, F, w, U)
        if return_energy:
            E.append(energy(V, F, w, U, c, s))
        ev = V[I] - V[J]
        rx = w * (c[:, None] * ev[..., 0] - s[:, None] * ev[..., 1])
        ry = w * (s[:, None] * ev[..., 0] + c[:, None] * ev[..., 1])
        rhs = np.zeros((n, 2))
        np.add.at(rhs[:, 0], I.ravel(), rx.ravel())
        np.add.at(rhs[:, 0], J.ravel(), -rx.ravel())
        np.add.at(rhs[:, 1], I.ravel(), ry.ravel())
        np.add.at(rhs[:, 1], J.ravel(), -ry.ravel())
        if solve is not None:
            r = rhs[free] - Lfc @ bc
            U[free, 0], U[free, 1] = solve(r[:, 0]), solve(r[:, 1])
        if return_energy:
            E.append(energy(V, F, w, U, c, s))
    return (U, np.array(E)) if return_energy else U


def render_uv(U, V, F, return_margin=False):
    """render_colors_core with colours (V_x / 671, V_y / 671), all depths 0: [672,672,2] float32 preset to -1, the first covering
    triangle in face order wins.  With return_margin also min(|u|, |v|, |1 - u - v|) of the winning test, and for uncovered
    pixels the smallest such value over the triangles whose bounding box held them (how close they came to being covered)."""
    U = np.asarray(U, f32)
    col = (np.asarray(V, np.float64) / (CANVAS - 1)).astype(f32)
    img = np.full((CANVAS, CANVAS, 2), -1, f32)
    done = np.zeros((CANVAS, CANVAS), bool)
    margin = np.full((CANVAS, CANVAS), np.inf, f32)
    one, zero = f32(1), f32(0)
    for t in range(len(F)):
        i0, i1, i2 = F[t]
        p0, p1, p2 = U[i0], U[i1], U[i2]
        xs, ys = (p0[0], p1[0], p2[0]), (p0[1], p1[1], p2[1])
        xmin, xmax = max(int(np.ceil(min(xs))), 0), min(int(np.floor(max(xs))), CANVAS - 1)
        ymin, ymax = max(int(np.ceil(min(ys))), 0), min(int(np.floor(max(ys))), CANVAS - 1)
        if xmax < xmin or ymax < ymin:
            continue
        px = np.arange(xmin, xmax + 1, dtype=f32)[None, :]
        py = np.arange(ymin, ymax + 1, dtype=f32)[:, None]
        v0x, v0y, v1x, v1y = p2[0] - p0[0], p2[1] - p0[1], p1[0] - p0[0], p1[1] - p0[1]
        v2x, v2y = px - p0[0], py - p0[1]
        dot00, dot01, dot11 = v0x * v0x + v0y * v0y, v0x * v1x + v0y * v1y, v1x * v1x + v1y * v1y
        dot02, dot12 = v0x * v2x + v0y * v2y, v1x * v2x + v1y * v2y
        den = dot00 * dot11 - dot01 * dot01
        inv = zero if den == 0 else one / den
        u = (dot11 * dot02 - dot01 * dot12) * inv
        v = (dot00 * dot12 - dot01 * dot02) * inv
        inside = (u >= 0) & (v >= 0) & (u + v < 1)
        sl = (slice(ymin, ymax + 1), slice(xmin, xmax + 1))
        new = inside & ~done[sl]
        w0 = one - u - v
        for ch in range(2):
            val = w0 * col[i0, ch] + v * col[i1, ch] + u * col[i2, ch]
            img[sl + (ch,)] = np.where(new, val, img[sl + (ch,)])
        if return_margin:
            m = np.minimum(np.minimum(np.abs(u), np.abs(v)), np.abs(one - u - v)).astype(f32)
            margin[sl] = np.where(new, m, np.where(done[sl], margin[sl], np.minimum(margin[sl], m)))
        done[sl] |= new
    return (img, margin) if return_margin else img


def edge_fix(uv):
    """triangle_wrap_hair.py:77-85 on a float32 [672,672,2] image, in place."""
    n = uv.shape[0]
    lin = np.linspace(0, 1, n, endpoint=True)
    uv[[0, -1], :, 0] = lin
    uv[[0, -1], :, 1] = np.array([[0.0], [1.0 - 1 / n]])
    uv[-2, :, 1] = np.min(uv[[-2, -1], :, 1], axis=0)
    uv[:, [0, -1], 1] = lin[..., None]
    uv[:, [0, -1], 0] = np.array([0.0, 1 - 1 / n])
    uv[:, -2, 0] = np.min(uv[:, [-2, -1], 0], axis=1)
    return uv


def padded_mask(hair_parsing):
    """mask_adaptor.py:119-129 -> uint8 0/1 [672,672]."""
    m = np.zeros((CANVAS, CANVAS), np.uint8)
    m[BG:BG + IMG, BG:BG + IMG] = np.asarray(hair_parsing) == HAIR
    m[BG - EXT:BG, m[BG, :] == 1] = 1
    m[-BG:-BG + EXT, m[-1 - BG, :] == 1] = 1
    m[m[:, BG] == 1, BG - EXT:BG] = 1
    m[m[:, -1 - BG] == 1, -BG:-BG + EXT] = 1
    return m


def sample(mask, uv):
    """cv2.remap(mask as float32, u * W, v * H, INTER_LINEAR), constant border 0, then .astype('uint8') -- for a 0/1 mask.
    OpenCV's documented arithmetic: sx = cvRound(x * 32) (half to even), tap = sx >> 5, fraction = sx & 31, weights
    (32 - a)(32 - b) / 1024 ... (exact in float32, summing to 1): the truncated value is 1 iff every tap of non-zero weight is 1."""
    H, W = mask.shape
    x, y = uv[..., 0] * f32(W), uv[..., 1] * f32(H)
    sx, sy = np.rint(x * f32(32)).astype(np.int64), np.rint(y * f32(32)).astype(np.int64)
    ix, iy, ax, ay = sx >> 5, sy >> 5, sx & 31, sy & 31

    def tap(r, c):
        ok = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        return np.where(ok, mask[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)], 0).astype(np.int64)
    acc = (32 - ax) * (32 - ay) * tap(iy, ix) + ax * (32 - ay) * tap(iy, ix + 1) + (32 - ax) * ay * tap(iy + 1, ix) \
        + ax * ay * tap(iy + 1, ix + 1)
    return (acc >= 1024).astype(np.uint8)


def compose(warped, face_parsing):
    """Crop (mask_adaptor.py:139-140) + naive_transfer (:63-73) -> uint8 [512,512]."""
    w = warped[BG:-BG, BG:-BG]
    out = np.asarray(face_parsing).astype(np.uint8).copy()
    out[out == HAIR] = 255
    out[w == 1] = HAIR
    return out


def warp_from_U(hair_parsing, face_parsing, V, F, U):
    """Everything after the ARAP solve -> (labels uint8 [512,512], uv float32 [672,672,2] after the edge fix)."""
    uv = edge_fix(render_uv(U, V, F))
    return compose(sample(padded_mask(hair_parsing), uv), face_parsing), uv


def warp(hair_parsing, face_parsing, V, F, b, bc):
    """End to end on a given mesh; U is rounded to float32 once, where the GPU stores it."""
    U = arap(V, F, b, bc).astype(f32)
    labels, uv = warp_from_U(hair_parsing, face_parsing, V, F, U)
    return labels, uv, U
