// face_matte.hip -- paste-back with an edge-aware matte: the weight map is refined by a guided filter whose guide is the photo's own
// RGB (He, Sun, Tang: "Guided Image Filtering"), so the border of the pasted region follows the edges visible in the photo instead of
// the staircase of an up-sampled label map.  Specification: ch_face_unalign_matte in include/ctrlhair_hip.h; DESIGN.md, "Matte".
//
// Domain D = the plan's bounding box, bw x bh pixels.  Four launches after the copy of everything outside D:
//   1. matte_weight_kernel   p8 = weight[floor(y)][floor(x)] inside the quad, 0 outside                       -> uint8 plane
//   2. matte_coeff_kernel    13 exact integer window sums (p, I, I p, I I^T) -> int64 covariances -> float64 LDL^T solve
//                            of (cov + eps Id) a = cov_Ip, b = mean p - a . mean I                             -> float4 (a, b) plane
//   3. matte_alpha_kernel    window means of (a, b) in float64, q = mean a . I / 255 + mean b, alpha = clamp(q, 0, 1) ramp -> float plane
//   4. face_unalign_matte_kernel   the composite of face_unalign.hip with alpha read from the plane (face_unalign_dev.h)
//
// Passes 2 and 3 are one skeleton (box_pass): a workgroup of 256 threads owns 256 consecutive columns (256 - 2 r outputs and r halo
// columns on each side) and `seg` consecutive rows.  Every thread keeps the K column sums of rows [Y - r, Y + r] in registers and
// slides them down one row at a time (add row Y + r + 1, subtract row Y - r); per row the K sums go through an inclusive prefix over
// the 256 columns (shuffles inside a wave, wave totals through LDS), and output column t takes prefix[t + r] - prefix[t - r - 1].
// The work per pixel does not depend on r; only the halo (2 r of 256 columns) and the warm-up (2 r + 1 rows per segment) do.
// Columns and rows outside D contribute zeros, which is the clipping of the specification.  The horizontal pass is fused: no plane
// of moments is ever stored, the workspace is 21 bytes per pixel (a, b: 16, alpha: 4, p8: 1).
//
// Pass 2 is integer: the prefix over 256 column sums may pass 2^31 (255^2 * 129 * 256), so it is kept in uint32, where the
// difference of two prefixes is exact modulo 2^32 and the true window sum (<= 255^2 * 129^2 < 2^31) comes out exact.  Exact sums
// make the result independent of how D is cut into workgroups.  Pass 3 slides float64 sums of float32 values: not exact, but a
// rounding error of 2^-53 per operation on sums of at most 129 * 256 terms, nine orders of magnitude below the float32 result.
#include "face_unalign_dev.h"

namespace chk {
namespace {

using namespace unalign;

constexpr int MBLK = 256, MWAVES = MBLK / 64;

struct MatteGeom {
    int bw, bh, r, seg;          // domain size, radius, rows per workgroup
    double eps;
};

// ---- pass 1 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MBLK) void matte_weight_kernel(const uint8_t* __restrict__ weight, UnalignGeom g, int bw, uint8_t* __restrict__ p8) {
    const int cx = blockIdx.x * MBLK + threadIdx.x, cy = blockIdx.y;
    if (cx >= bw) return;
    double x, y;
    crop_xy(g, g.x0 + cx, g.y0 + cy, x, y);
    const double m = fmin(fmin(x, (double)g.S - x), fmin(y, (double)g.S - y));
    uint8_t v = 0;
    if (m > 0.0) {
        const int i = min(max((int)floor(x), 0), g.S - 1), j = min(max((int)floor(y), 0), g.S - 1);
        v = weight[(size_t)j * g.S + i];
    }
    p8[(size_t)cy * bw + cx] = v;
}

// ---- the sliding box skeleton -------------------------------------------------------------------------------------------------
// inclusive prefix of v[k] over the workgroup's 256 threads, then the window sum prefix[t + r] - prefix[t - r - 1] for the output
// threads (r <= t < 256 - r).  tot: [K][MWAVES], pre: [K][MBLK] in LDS.  Two barriers; safe to call again at once (tot is read
// before the second barrier and written before the first of the next call, pre the other way round).
template <int K, typename T>
__device__ __forceinline__ void window_sums(const T (&v)[K], T (&w)[K], int r, bool is_out, T* tot, T* pre) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    T p[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T s = v[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T o = __shfl_up(s, d, 64);
            if (lane >= d) s += o;
        }
        p[k] = s;
        if (lane == 63) tot[k * MWAVES + wave] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        T base = T(0);
#pragma unroll
        for (int q = 0; q < MWAVES - 1; ++q)
            if (q < wave) base += tot[k * MWAVES + q];
        pre[k * MBLK + t] = p[k] + base;
    }
    __syncthreads();
    if (is_out) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T hi = pre[k * MBLK + t + r];
            const T lo = t - r - 1 >= 0 ? pre[k * MBLK + t - r - 1] : T(0);
            w[k] = hi - lo;
        }
    }
}

// load(cx, cy, T (&)[K]) gives the K terms of domain pixel (cx, cy); emit(cx, cy, n, T (&)[K]) takes the K window sums of an output
// pixel and the pixel count n of its clipped window.
template <int K, typename T, typename Load, typename Emit>
__device__ __forceinline__ void box_pass(const MatteGeom& m, Load load, Emit emit) {
    __shared__ T tot[K * MWAVES];
    __shared__ T pre[K * MBLK];
    const int t = threadIdx.x, r = m.r, outw = MBLK - 2 * r;
    const int cx = (int)blockIdx.x * outw - r + t;
    const bool col_ok = cx >= 0 && cx < m.bw;
    const bool is_out = col_ok && t >= r && t < r + outw;
    const int ys = (int)blockIdx.y * m.seg, ye = min(ys + m.seg, m.bh);
    T v[K], w[K], c[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = T(0), w[k] = T(0);
    if (col_ok) {
        for (int yy = max(ys - r, 0); yy <= min(ys + r, m.bh - 1); ++yy) {        // warm-up: the window of the segment's first row
            load(cx, yy, c);
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] += c[k];
        }
    }
    const int nx = min(cx + r, m.bw - 1) - max(cx - r, 0) + 1;
    for (int y = ys; y < ye; ++y) {                   // uniform over the workgroup: every thread reaches the barriers
        window_sums<K, T>(v, w, r, is_out, tot, pre);
        if (is_out) emit(cx, y, nx * (min(y + r, m.bh - 1) - max(y - r, 0) + 1), w);
        if (col_ok && y + 1 < ye) {
            if (y + r + 1 < m.bh) {
                load(cx, y + r + 1, c);
#pragma unroll
                for (int k = 0; k < K; ++k) v[k] += c[k];
            }
            if (y - r >= 0) {
                load(cx, y - r, c);
#pragma unroll
                for (int k = 0; k < K; ++k) v[k] -= c[k];
            }
        }
    }
}

// ---- pass 2 ------------------------------------------------------------------------------------------------------------------
// sums: 0 p | 1..3 I_c | 4..6 I_c p | 7..12 I_0 I_0, I_0 I_1, I_0 I_2, I_1 I_1, I_1 I_2, I_2 I_2
__global__ __launch_bounds__(MBLK) void matte_coeff_kernel(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ p8, UnalignGeom g,
                                                           MatteGeom m, float4* __restrict__ ab) {
    auto load = [&](int cx, int cy, uint32_t (&c)[13]) {
        const uint8_t* q = photo + ((size_t)(g.y0 + cy) * g.W + (g.x0 + cx)) * 3;
        const uint32_t i0 = q[0], i1 = q[1], i2 = q[2], p = p8[(size_t)cy * m.bw + cx];
        c[0] = p, c[1] = i0, c[2] = i1, c[3] = i2;
        c[4] = i0 * p, c[5] = i1 * p, c[6] = i2 * p;
        c[7] = i0 * i0, c[8] = i0 * i1, c[9] = i0 * i2, c[10] = i1 * i1, c[11] = i1 * i2, c[12] = i2 * i2;
    };
    auto emit = [&](int cx, int cy, int n, const uint32_t (&w)[13]) {
        const long long nn = n, sp = w[0], s0 = w[1], s1 = w[2], s2 = w[3];
        const double den = (double)n * (double)n * 65025.0;              // n^2 255^2 <= 1.8e13: exact
        // exact integer numerators (|.| <= 129^2 * 1.08e9 < 2^63), one rounding each on the way to float64
        const double c0 = (double)(nn * (long long)w[4] - s0 * sp) / den;
        const double c1 = (double)(nn * (long long)w[5] - s1 * sp) / den;
        const double c2 = (double)(nn * (long long)w[6] - s2 * sp) / den;
        const double a00 = (double)(nn * (long long)w[7] - s0 * s0) / den + m.eps;
        const double a01 = (double)(nn * (long long)w[8] - s0 * s1) / den;
        const double a02 = (double)(nn * (long long)w[9] - s0 * s2) / den;
        const double a11 = (double)(nn * (long long)w[10] - s1 * s1) / den + m.eps;
        const double a12 = (double)(nn * (long long)w[11] - s1 * s2) / den;
        const double a22 = (double)(nn * (long long)w[12] - s2 * s2) / den + m.eps;
        // (cov + eps Id) a = c by LDL^T (Cholesky without the square roots): the matrix is symmetric positive definite, every pivot >= eps
        const double l10 = a01 / a00, l20 = a02 / a00;
        const double d1 = a11 - l10 * a01;
        const double u = a12 - l20 * a01;
        const double l21 = u / d1;
        const double d2 = a22 - l20 * a02 - l21 * u;
        const double z1 = c1 - l10 * c0;
        const double z2 = c2 - l20 * c0 - l21 * z1;
        const double x2 = z2 / d2;
        const double x1 = z1 / d1 - l21 * x2;
        const double x0 = c0 / a00 - l10 * x1 - l20 * x2;
        const double dn = 255.0 * (double)n;
        const double b = (double)sp / dn - (x0 * ((double)s0 / dn) + x1 * ((double)s1 / dn) + x2 * ((double)s2 / dn));
        ab[(size_t)cy * m.bw + cx] = make_float4((float)x0, (float)x1, (float)x2, (float)b);
    };
    box_pass<13, uint32_t>(m, load, emit);
}

// ---- pass 3 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MBLK) void matte_alpha_kernel(const uint8_t* __restrict__ photo, const float4* __restrict__ ab, UnalignGeom g,
                                                           MatteGeom m, float* __restrict__ alpha) {
    auto load = [&](int cx, int cy, double (&c)[4]) {
        const float4 v = ab[(size_t)cy * m.bw + cx];
        c[0] = v.x, c[1] = v.y, c[2] = v.z, c[3] = v.w;
    };
    auto emit = [&](int cx, int cy, int n, const double (&w)[4]) {
        const uint8_t* q = photo + ((size_t)(g.y0 + cy) * g.W + (g.x0 + cx)) * 3;
        const double dn = (double)n;
        const double v = (w[0] / dn) * ((double)q[0] / 255.0) + (w[1] / dn) * ((double)q[1] / 255.0) + (w[2] / dn) * ((double)q[2] / 255.0) + w[3] / dn;
        const float mt = (float)fmin(fmax(v, 0.0), 1.0);
        double x, y;
        crop_xy(g, g.x0 + cx, g.y0 + cy, x, y);
        alpha[(size_t)cy * m.bw + cx] = mt * border_ramp(g, x, y);
    };
    box_pass<4, double>(m, load, emit);
}

// ---- pass 4 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLK) void face_unalign_matte_kernel(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ edits,
                                                                 const float* __restrict__ alpha_plane, UnalignGeom g, uint8_t* __restrict__ out) {
    extern __shared__ float wx_lds[];                 // [nt][BLK]
    const int tid = threadIdx.y * TW + threadIdx.x;
    const int X = g.x0 + blockIdx.x * TW + threadIdx.x, Y = g.y0 + blockIdx.y * TH + threadIdx.y;
    if (X >= g.x1 || Y >= g.y1) return;
    const int n = blockIdx.z;
    const size_t pix = ((size_t)Y * g.W + X) * 3;
    const uint8_t* p = photo + pix;
    uint8_t* o = out + (size_t)n * g.H * g.W * 3 + pix;
    const uint8_t p0 = p[0], p1 = p[1], p2 = p[2];
    const float alpha = alpha_plane[(size_t)(Y - g.y0) * (g.x1 - g.x0) + (X - g.x0)];
    if (!(alpha > 0.0f)) {                            // outside the quad (the ramp is 0 there), or matte 0: the photo, untouched
        o[0] = p0, o[1] = p1, o[2] = p2;
        return;
    }
    double x, y;
    crop_xy(g, X, Y, x, y);
    resample_composite(g, edits, n, x, y, alpha, p0, p1, p2, o, wx_lds, tid);
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

// workspace: float4 ab [bh bw] | float alpha [bh bw] | uint8 p8 [bh bw], each part starting on a 256-byte boundary
size_t face_matte_workspace_bytes(int bw, int bh) {
    const size_t n = (size_t)bw * bh;
    return round_up(16 * n, 256) + round_up(4 * n, 256) + round_up(n, 256);
}

hipError_t face_unalign_matte(const uint8_t* photo, const uint8_t* edits, const uint8_t* weight, const UnalignPlan& p, int H, int W, int N,
                              double feather_px, int radius, double eps, uint8_t* out, float* alpha_out, void* ws, hipStream_t s) {
    const UnalignGeom g = make_geom(p, H, W, N, feather_px);
    MatteGeom m;
    m.bw = p.x1 - p.x0, m.bh = p.y1 - p.y0, m.r = radius, m.eps = eps;
    const size_t n = (size_t)m.bw * m.bh;
    float4* ab = static_cast<float4*>(ws);
    float* alpha_ws = reinterpret_cast<float*>(static_cast<uint8_t*>(ws) + round_up(16 * n, 256));
    uint8_t* p8 = static_cast<uint8_t*>(ws) + round_up(16 * n, 256) + round_up(4 * n, 256);
    float* alpha = alpha_out ? alpha_out : alpha_ws;

    copy_outside(photo, out, g, s);
    matte_weight_kernel<<<dim3((unsigned)((m.bw + MBLK - 1) / MBLK), (unsigned)m.bh), MBLK, 0, s>>>(weight, g, m.bw, p8);

    // rows per workgroup: long segments amortise the 2 r + 1 warm-up rows, short ones fill the device; the integer pass gives the
    // same bits for any cut, the float64 pass sees the same cut for the same (bw, bh, r), whatever N
    const int outw = MBLK - 2 * radius, nbx = (m.bw + outw - 1) / outw;
    int seg = 128;
    while (seg > 16 && seg > radius && (long long)nbx * ((m.bh + seg - 1) / seg) < 1024) seg /= 2;
    m.seg = seg;
    const dim3 grid((unsigned)nbx, (unsigned)((m.bh + seg - 1) / seg));
    matte_coeff_kernel<<<grid, MBLK, 0, s>>>(photo, p8, g, m, ab);
    matte_alpha_kernel<<<grid, MBLK, 0, s>>>(photo, ab, g, m, alpha);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_composite(face_unalign_matte_kernel, photo, edits, static_cast<const float*>(alpha), g, out, s);
}

}  // namespace chk
