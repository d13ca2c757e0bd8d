// delaunay.hip -- batched exact Delaunay triangulation of small planar point sets (the meshes of the hair-shape transfer warp):
//   delaunay_kernel   one workgroup per set, the points in LDS, one lane per point.  Lane p finds p's nearest neighbour q0 (the
//                     edge p-q0 is in every Delaunay triangulation), then walks the triangles around p: the apex of the triangle
//                     left of a directed edge is found by one brute-force scan of the set (orientation + incircle per point).
//                     A triangle is emitted by the lane of its smallest vertex only, the emitted rows are sorted in LDS.
// Exactness: coordinates are multiples of 2^-20 in [0, 1024), i.e. 30-bit integers (checked per point, status OFF_GRID otherwise).
// Every predicate is evaluated in float64 with a proven error bound and, below the bound, again in integers (orientation:
// int64, incircle: 124 bits in __int128), so every decision is the exact one.
// Ties: k >= 4 points on one empty circle are triangulated as a fan from the smallest index among them.  The rule depends on the
// co-circular set alone, so every lane that meets the set draws the same diagonals (see apex()).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace chk {
namespace {

constexpr int DT = 1024;                       // threads of the workgroup; lane tid owns points tid, tid + DT
constexpr double GRID = 1048576.0;             // 2^20 grid units per pixel
constexpr double COORD_END = 1073741824.0;     // 2^30: coordinates are integers in [0, 2^30)
constexpr double ORIENT_BOUND = 4096.0;        // orientation in f64: two products < 2^62 rounded (<= 2^9 each) and one sum
constexpr double INCIRCLE_EPS = 0x1p-49;       // incircle in f64: |error| <= 16 * 2^-53 * permanent, see set_candidate()

__host__ __device__ inline size_t del_head(int B) { return ((size_t)B * 2 * sizeof(int) + 255) / 256 * 256; }

// Descriptors reach the device as kernel arguments (no host buffer has to outlive the call), DELAUNAY_DESC_SETS per store launch
__global__ void delaunay_store_desc_kernel(DelaunayDesc desc, int* __restrict__ dst) {
    const int i = threadIdx.x;
    if (i < desc.n * 2) dst[desc.set0 * 2 + i] = desc.d[i / 2][i % 2];
}

__device__ inline long long orient_exact(int ax, int ay, int bx, int by, int cx, int cy) {
    return (long long)(bx - ax) * (long long)(cy - ay) - (long long)(by - ay) * (long long)(cx - ax);
}

// sign of the incircle determinant of (0, b, c, d), all relative to a: > 0 iff d lies strictly inside the circle of the
// counter-clockwise triangle (a, b, c).  |coordinates| < 2^30: lifts < 2^61, 2x2 minors < 2^92, the determinant < 2^124.
__device__ inline int incircle_exact(long long bx, long long by, long long cx, long long cy, long long dx, long long dy) {
    const long long bl = bx * bx + by * by, cl = cx * cx + cy * cy, dl = dx * dx + dy * dy;
    const __int128 m1 = (__int128)bl * cy - (__int128)by * cl, m2 = (__int128)bx * cl - (__int128)bl * cx;
    const long long m3 = by * cx - bx * cy;
    const __int128 det = m1 * dx + m2 * dy + (__int128)dl * m3;
    return det > 0 ? 1 : (det < 0 ? -1 : 0);
}

struct Apex {                                  // the circle through a, b and the current candidate c, relative to a
    double cx, cy;                             // c - a
    double m1, m2, m3, p1, p2, p3;             // minors of the rows of b and c, and their permanents
};

// The minors are rounded: with e = 2^-53, bl and cl carry 2e, each product one more and the difference one more, so
// |m_i - exact| <= 4e * p_i.  det = dx m1 + dy m2 + dl m3 adds one rounding per product, 2e for dl and one per sum:
// |det - exact| <= 10e * (|dx| p1 + |dy| p2 + dl p3); 16e (INCIRCLE_EPS) also covers the rounding of the permanent itself.
// A fused multiply-add only removes roundings.
__device__ inline void set_candidate(Apex& A, double bx, double by, double cx, double cy) {
    const double bl = bx * bx + by * by, cl = cx * cx + cy * cy;
    A.cx = cx;
    A.cy = cy;
    A.m1 = bl * cy - by * cl;
    A.m2 = bx * cl - bl * cx;
    A.m3 = by * cx - bx * cy;
    A.p1 = bl * fabs(cy) + fabs(by) * cl;
    A.p2 = fabs(bx) * cl + bl * fabs(cx);
    A.p3 = fabs(by * cx) + fabs(bx * cy);
}

// Third vertex of the triangle left of the directed edge a -> b in the canonical Delaunay triangulation, or -1 when nothing lies
// left of it (a hull edge).  Requires a -> b to be an edge of that triangulation.
// One scan keeps c = the left point whose circle (a, b, c) holds no point seen so far, and the tie set T = the left points on
// that circle.  A later point strictly inside replaces c and empties T: the part of the disc left of a -> b only shrinks, so no
// earlier point can lie on the new circle.  With m = the smallest index of T + {a, b}, the polygon on the circle is fanned
// from m: m == a gives (a, b, the polygon's vertex after b), m == b gives (a, b, the vertex before a), otherwise (a, b, m).
// Points of the circle right of a -> b exist only when a -> b is a fan diagonal, and then m is a or b already.
__device__ inline int apex(const double* sX, const double* sY, int n, int a, int b, unsigned& tests, unsigned& exact) {
    const double ax = sX[a], ay = sY[a], bx = sX[b] - ax, by = sY[b] - ay;
    const int iax = (int)ax, iay = (int)ay, ibx = (int)sX[b], iby = (int)sY[b];
    Apex A;
    int c = -1, mT = 0, xq = 0, xp = 0;
    for (int d = 0; d < n; ++d) {
        const double dx = sX[d] - ax, dy = sY[d] - ay;
        const double o = bx * dy - by * dx;
        if (o < -ORIENT_BOUND) continue;
        if (fabs(o) <= ORIENT_BOUND && orient_exact(iax, iay, ibx, iby, (int)sX[d], (int)sY[d]) <= 0) continue;   // also d == a, b
        int s = 1;
        if (c >= 0) {
            const double dl = dx * dx + dy * dy;
            const double det = dx * A.m1 + dy * A.m2 + dl * A.m3;
            const double bound = INCIRCLE_EPS * (fabs(dx) * A.p1 + fabs(dy) * A.p2 + dl * A.p3);
            ++tests;
            if (det > bound)
                s = 1;
            else if (det < -bound)
                s = -1;
            else {
                ++exact;
                s = incircle_exact((int)bx, (int)by, (int)A.cx, (int)A.cy, (int)dx, (int)dy);
            }
        }
        if (s > 0) {
            c = mT = xq = xp = d;
            set_candidate(A, bx, by, dx, dy);
        } else if (s == 0) {
            const int idx = (int)sX[d], idy = (int)sY[d];
            mT = min(mT, d);
            if (orient_exact(ibx, iby, (int)sX[xq], (int)sY[xq], idx, idy) < 0) xq = d;    // d lies between b and xq on the circle
            if (orient_exact(iax, iay, (int)sX[xp], (int)sY[xp], idx, idy) > 0) xp = d;    // d lies between xp and a
        }
    }
    if (c < 0) return -1;
    const int m = min(min(a, b), mT);
    return m == a ? xq : (m == b ? xp : mT);
}

__global__ __launch_bounds__(DT) void delaunay_kernel(const float* __restrict__ V, int B, char* __restrict__ ws, int* __restrict__ F,
                                                      int* __restrict__ n_f, int* __restrict__ status) {
    __shared__ double sX[WARP_MAX_V], sY[WARP_MAX_V];
    __shared__ unsigned long long sKey[WARP_MAX_F];        // emitted rows, (v0 << 22) | (v1 << 11) | v2
    __shared__ short sNear[WARP_MAX_V];
    __shared__ unsigned long long sStat[2];
    __shared__ int sCount, sStatus;
    static_assert(WARP_MAX_V <= 2048 && WARP_MAX_V <= 2 * DT, "keys hold 11 bits per index, a lane owns two points");

    const int tid = threadIdx.x, set = blockIdx.x;
    const int* desc = reinterpret_cast<const int*>(ws) + 2 * set;
    const int off = desc[0], n = desc[1];
    unsigned long long* stat = reinterpret_cast<unsigned long long*>(ws + del_head(B)) + 2 * set;
    int* Fo = F + (size_t)set * WARP_MAX_F * 3;

    if (tid == 0) {
        sCount = 0;
        sStatus = DELAUNAY_OK;
        sStat[0] = sStat[1] = 0;
        stat[0] = stat[1] = 0;
    }
    __syncthreads();
    if (off < 0 || n < 3 || n > WARP_MAX_V) {              // uniform; nothing of V is read
        if (tid == 0) {
            n_f[set] = 0;
            status[set] = DELAUNAY_BAD_COUNT;
        }
        return;
    }
    for (int i = tid; i < n; i += DT) {
        const double x = (double)V[2 * ((size_t)off + i)] * GRID, y = (double)V[2 * ((size_t)off + i) + 1] * GRID;
        const bool ok = x >= 0.0 && x < COORD_END && y >= 0.0 && y < COORD_END && x == floor(x) && y == floor(y);   // false for NaN
        if (!ok) sStatus = DELAUNAY_OFF_GRID;
        sX[i] = ok ? x : 0.0;
        sY[i] = ok ? y : 0.0;
    }
    __syncthreads();
    if (sStatus != DELAUNAY_OK) {
        if (tid == 0) {
            n_f[set] = 0;
            status[set] = sStatus;
        }
        return;
    }

    // ---- nearest neighbour of every point (exact squared distances; the float64 value only skips the clear cases) ------------
    for (int p = tid; p < n; p += DT) {
        const double px = sX[p], py = sY[p];
        const int ipx = (int)px, ipy = (int)py;
        long long best = 0x7fffffffffffffffLL;
        double skip = 1e300;
        int q = 0;
        for (int d = 0; d < n; ++d) {
            const double dx = sX[d] - px, dy = sY[d] - py;
            if (dx * dx + dy * dy > skip || d == p) continue;
            const long long ix = (int)sX[d] - ipx, iy = (int)sY[d] - ipy, dd = ix * ix + iy * iy;
            if (dd < best) {
                best = dd;
                q = d;
                skip = (double)dd * (1.0 + 0x1p-50);
            }
        }
        if (best == 0) sStatus = DELAUNAY_DUPLICATE;
        sNear[p] = (short)q;
    }
    __syncthreads();
    if (sStatus != DELAUNAY_OK) {
        if (tid == 0) {
            n_f[set] = 0;
            status[set] = sStatus;
        }
        return;
    }

    // ---- walk the triangles around every point; the lane of a triangle's smallest vertex emits it ---------------------------
    unsigned tests = 0, exact = 0;
    auto emit = [&](int p, int v1, int v2) {
        if (p > v1 || p > v2) return;
        const int slot = atomicAdd(&sCount, 1);            // the order is fixed by the sort below, not by this counter
        if (slot < WARP_MAX_F) sKey[slot] = ((unsigned long long)p << 22) | ((unsigned long long)v1 << 11) | (unsigned long long)v2;
    };
    for (int p = tid; p < n; p += DT) {
        const int q0 = sNear[p];
        int q = q0;
        bool closed = false;
        for (int step = 0; step < n; ++step) {             // counter-clockwise from p -> q0
            const int x = apex(sX, sY, n, p, q, tests, exact);
            if (x < 0) break;
            emit(p, q, x);
            if (x == q0) {
                closed = true;
                break;
            }
            q = x;
        }
        if (closed) continue;
        q = q0;                                            // p is on the hull: the other way round from p -> q0
        for (int step = 0; step < n; ++step) {
            const int x = apex(sX, sY, n, q, p, tests, exact);
            if (x < 0) break;
            emit(p, x, q);
            q = x;
        }
    }
    atomicAdd(&sStat[0], (unsigned long long)tests);
    atomicAdd(&sStat[1], (unsigned long long)exact);
    __syncthreads();
    const int count = sCount;
    if (count < 1 || count > WARP_MAX_F) {                 // uniform.  No triangle at all: every point is on one line
        if (tid == 0) {
            n_f[set] = 0;
            status[set] = count < 1 ? DELAUNAY_COLLINEAR : DELAUNAY_INTERNAL;
            stat[0] = sStat[0];
            stat[1] = sStat[1];
        }
        return;
    }

    // ---- bitonic sort of the keys: rows in lexicographic order ---------------------------------------------------------------
    int N2 = 2;
    while (N2 < count) N2 <<= 1;
    for (int i = count + tid; i < N2; i += DT) sKey[i] = ~0ull;
    __syncthreads();
    for (int k = 2; k <= N2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < N2; i += DT) {
                const int o = i ^ j;
                if (o > i) {
                    const unsigned long long a = sKey[i], b = sKey[o];
                    if ((a > b) == ((i & k) == 0)) {
                        sKey[i] = b;
                        sKey[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (int t = tid; t + 1 < count; t += DT)
        if (sKey[t] == sKey[t + 1]) sStatus = DELAUNAY_INTERNAL;           // cannot happen: every triangle has one smallest vertex
    __syncthreads();
    if (sStatus != DELAUNAY_OK) {
        if (tid == 0) {
            n_f[set] = 0;
            status[set] = sStatus;
        }
        return;
    }
    for (int t = tid; t < count; t += DT) {
        const unsigned long long key = sKey[t];
        Fo[3 * t] = (int)(key >> 22);
        Fo[3 * t + 1] = (int)((key >> 11) & 2047);
        Fo[3 * t + 2] = (int)(key & 2047);
    }
    if (tid == 0) {
        n_f[set] = count;
        status[set] = DELAUNAY_OK;
        stat[0] = sStat[0];
        stat[1] = sStat[1];
    }
}

}  // namespace

size_t delaunay_workspace_bytes(int B) { return B > 0 ? del_head(B) + (size_t)B * 2 * sizeof(unsigned long long) : 0; }

hipError_t delaunay_batch(const float* V, const int* v_desc_host, int* F, int* n_f, int* status, void* ws, int B, hipStream_t s) {
    char* w = static_cast<char*>(ws);
    for (int s0 = 0; s0 < B; s0 += DELAUNAY_DESC_SETS) {
        DelaunayDesc desc;
        desc.n = B - s0 < DELAUNAY_DESC_SETS ? B - s0 : DELAUNAY_DESC_SETS;
        desc.set0 = s0;
        for (int i = 0; i < DELAUNAY_DESC_SETS; ++i)
            for (int k = 0; k < 2; ++k) desc.d[i][k] = i < desc.n ? v_desc_host[2 * (s0 + i) + k] : 0;
        delaunay_store_desc_kernel<<<1, DELAUNAY_DESC_SETS * 2, 0, s>>>(desc, reinterpret_cast<int*>(w));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    delaunay_kernel<<<B, DT, 0, s>>>(V, B, w, F, n_f, status);
    return hipGetLastError();
}

}  // namespace chk
