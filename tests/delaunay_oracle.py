"""Exact checker of a planar Delaunay triangulation in canonical form (what warping.build_mesh and ch_delaunay_batch produce).

All decisions are made in Python integers on the 2^-20 grid (coordinates * 2^20 must be integral), so there is no tolerance
anywhere.  `check` raises MeshError naming the first violated property; it returns the number of hull points h and, on request,
the set of *unique* triangles: those whose circumcircle passes through no fourth point (every Delaunay triangulation of the set
contains them; two Delaunay triangulations differ only inside groups of co-circular points)."""
import numpy as np

GRID = 1 << 20


class MeshError(AssertionError):
    pass


def to_grid(V):
    """float [n,2] -> list of (x, y) Python ints on the 2^-20 grid; raises MeshError if a coordinate is off the grid."""
    s = np.asarray(V, np.float64) * GRID
    if s.ndim != 2 or s.shape[1] != 2 or not np.isfinite(s).all() or (s != np.rint(s)).any():
        raise MeshError('coordinates are not multiples of 2^-20')
    return [(int(x), int(y)) for x, y in s]


def orient(a, b, c):
    return (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])


def incircle(a, b, c, d):
    """> 0 iff d lies strictly inside the circle of the counter-clockwise triangle (a, b, c); 0 on it."""
    ax, ay, bx, by, cx, cy = a[0] - d[0], a[1] - d[1], b[0] - d[0], b[1] - d[1], c[0] - d[0], c[1] - d[1]
    return ((ax * ax + ay * ay) * (bx * cy - cx * by) + (bx * bx + by * by) * (cx * ay - ax * cy)
            + (cx * cx + cy * cy) * (ax * by - bx * ay))


def hull_boundary(P):
    """Indices of ALL points on the boundary of the convex hull (collinear ones included), counter-clockwise."""
    idx = sorted(range(len(P)), key=lambda i: P[i])

    def chain(order):
        h = []
        for i in order:
            while len(h) >= 2 and orient(P[h[-2]], P[h[-1]], P[i]) < 0:
                h.pop()
            h.append(i)
        return h
    lower, upper = chain(idx), chain(idx[::-1])
    return lower[:-1] + upper[:-1]


def unique_triangles(P, F):
    """The rows of F whose circumcircle passes through no other point.  A float64 evaluation sorts out the clear cases, every
    candidate within its error bound is decided in integers."""
    X = np.array(P, np.float64)
    F = np.asarray(F, np.int64)
    a, b, c = X[F[:, 0]], X[F[:, 1]], X[F[:, 2]]
    out = set()
    for t in range(len(F)):
        A, Bv, Cv = a[t] - X, b[t] - X, c[t] - X
        al, bl, cl = (A ** 2).sum(1), (Bv ** 2).sum(1), (Cv ** 2).sum(1)
        m1, m2, m3 = Bv[:, 0] * Cv[:, 1], Cv[:, 0] * Bv[:, 1], Cv[:, 0] * A[:, 1]
        m4, m5, m6 = A[:, 0] * Cv[:, 1], A[:, 0] * Bv[:, 1], Bv[:, 0] * A[:, 1]
        det = al * (m1 - m2) + bl * (m3 - m4) + cl * (m5 - m6)
        perm = al * (abs(m1) + abs(m2)) + bl * (abs(m3) + abs(m4)) + cl * (abs(m5) + abs(m6))
        near = np.nonzero(abs(det) <= 1e-14 * perm)[0]
        on = [int(d) for d in near if int(d) not in F[t] and incircle(P[F[t, 0]], P[F[t, 1]], P[F[t, 2]], P[int(d)]) == 0]
        if not on:
            out.add(tuple(int(v) for v in F[t]))
    return out


def check(V, F, want_unique=False):
    """Raises MeshError unless F is the canonical form of a Delaunay triangulation of the convex hull of V.
    -> (h, unique triangle set or None)."""
    P = to_grid(V)
    n = len(P)
    F = np.asarray(F)
    if F.ndim != 2 or F.shape[1] != 3 or len(F) < 1:
        raise MeshError(f'F must be [m,3] with m >= 1, got {F.shape}')
    if F.min() < 0 or F.max() >= n:
        raise MeshError('index out of range')
    rows = [tuple(int(v) for v in r) for r in F]
    # canonical form
    for r in rows:
        if not (r[0] < r[1] and r[0] < r[2]):
            raise MeshError(f'row {r} does not start with its smallest index')
    if any(rows[i] >= rows[i + 1] for i in range(len(rows) - 1)):
        raise MeshError('rows are not in strict lexicographic order (unsorted or duplicated)')
    # strictly positive areas
    area2 = 0
    for r in rows:
        o = orient(P[r[0]], P[r[1]], P[r[2]])
        if o <= 0:
            raise MeshError(f'triangle {r} is not counter-clockwise with positive area')
        area2 += o
    # every directed edge once; every undirected edge in one or two triangles
    opp = {}
    for r in rows:
        for k in range(3):
            e = (r[k], r[(k + 1) % 3])
            if e in opp:
                raise MeshError(f'directed edge {e} is in two triangles (overlap)')
            opp[e] = r[(k + 2) % 3]
    boundary = {e for e in opp if (e[1], e[0]) not in opp}
    # the boundary is the hull, all collinear points included
    hb = hull_boundary(P)
    h = len(hb)
    hull_edges = {(hb[i], hb[(i + 1) % h]) for i in range(h)}
    if boundary != hull_edges:
        raise MeshError(f'boundary edges differ from the hull: {len(boundary)} boundary edges, {h} hull edges, '
                        f'{len(boundary ^ hull_edges)} in one set only')
    if len(rows) != 2 * n - 2 - h:
        raise MeshError(f'{len(rows)} triangles, expected 2n - 2 - h = {2 * n - 2 - h}')
    hull_area2 = sum(P[hb[i]][0] * P[hb[(i + 1) % h]][1] - P[hb[(i + 1) % h]][0] * P[hb[i]][1] for i in range(h))
    if area2 != hull_area2:
        raise MeshError(f'triangle areas sum to {area2}, the hull has {hull_area2} (in half grid units squared)')
    used = {v for r in rows for v in r}
    if len(used) != n:
        raise MeshError(f'{n - len(used)} points are in no triangle')
    # every interior edge locally Delaunay
    for (u, v), w in opp.items():
        if u < v and (v, u) in opp:
            x = opp[(v, u)]
            if incircle(P[u], P[v], P[w], P[x]) > 0:
                raise MeshError(f'edge ({u}, {v}) is not locally Delaunay: {x} lies inside the circle of ({u}, {v}, {w})')
    return h, (unique_triangles(P, F) if want_unique else None)


def tied_edges(V, F):
    """Interior edges (u, v, w, x) whose two triangles (u, v, w), (v, u, x) are co-circular, and those that are not."""
    P = to_grid(V)
    opp = {}
    for r in np.asarray(F):
        r = [int(v) for v in r]
        for k in range(3):
            opp[(r[k], r[(k + 1) % 3])] = r[(k + 2) % 3]
    tied, strict = [], []
    for (u, v), w in opp.items():
        if u < v and (v, u) in opp:
            x = opp[(v, u)]
            (tied if incircle(P[u], P[v], P[w], P[x]) == 0 else strict).append((u, v, w, x))
    return tied, strict


def canonical(F):
    """Rows rotated to start with their smallest index, then sorted: the canonical form of an oriented triangle list."""
    F = np.asarray(F, np.int64)
    k = F.argmin(1)
    F = np.stack([F[np.arange(len(F)), (k + j) % 3] for j in range(3)], 1)
    return F[np.lexsort((F[:, 2], F[:, 1], F[:, 0]))].astype(np.int32)
