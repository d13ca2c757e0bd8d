// face_unalign_dev.h -- device code shared by the two paste-back entries: face_unalign.hip (alpha from the geometric ramp and an
// optional bilinear weight) and face_matte.hip (alpha from the guided-filter matte plane).  The geometry, the Lanczos-3 resample, the
// composite and the copy of everything outside the bounding box exist once, here; the two kernels differ only in where alpha comes from.
#pragma once
#include "kernels.h"

namespace chk {
namespace unalign {

constexpr int TW = 32, TH = 8, BLK = TW * TH;

struct UnalignGeom {
    double a[6];                 // A row-major [2][3]
    int x0, y0, x1, y1;          // bounding box in the photo
    int H, W, S, N;
    int nt;                      // LDS rows per thread: floor(6 fs) + 1 >= the number of x taps of any pixel
    float inv_fs;                // 1 / fs
    double support;              // 3 fs
    float feather;               // <= 0: hard edge
};

inline UnalignGeom make_geom(const UnalignPlan& p, int H, int W, int N, double feather_px) {
    UnalignGeom g;
    for (int i = 0; i < 6; ++i) g.a[i] = p.A[i];
    g.x0 = p.x0, g.y0 = p.y0, g.x1 = p.x1, g.y1 = p.y1;
    g.H = H, g.W = W, g.S = p.S, g.N = N;
    const double fs = p.scale > 1.0 ? p.scale : 1.0;
    g.nt = (int)(6.0 * fs) + 1;
    g.inv_fs = (float)(1.0 / fs);
    g.support = 3.0 * fs;
    g.feather = (float)feather_px;
    return g;
}

__device__ __forceinline__ float lanczos3f(float t) {           // t already divided by fs
    const float a = fabsf(t);
    if (a >= 3.0f) return 0.0f;
    if (a < 1e-4f) return 1.0f;
    return sinpif(t) * sinpif(t * (1.0f / 3.0f)) * (3.0f / (float)(M_PI * M_PI)) / (t * t);
}

// first and one-past-last tap of the open interval |i + 0.5 - c| < sup, clipped to [0, S)
__device__ __forceinline__ void tap_range(double c, double sup, int S, int& lo, int& hi) {
    lo = (int)floor(c - sup - 0.5) + 1;
    hi = (int)ceil(c + sup - 0.5);
    lo = lo < 0 ? 0 : lo;
    hi = hi > S ? S : hi;
}

// crop coordinates of photo pixel (X, Y): float64, left to right, no fused multiply-add
__device__ __forceinline__ void crop_xy(const UnalignGeom& g, int X, int Y, double& x, double& y) {
    const double Xc = X + 0.5, Yc = Y + 0.5;
    x = __dadd_rn(__dadd_rn(__dmul_rn(g.a[0], Xc), __dmul_rn(g.a[1], Yc)), g.a[2]);
    y = __dadd_rn(__dadd_rn(__dmul_rn(g.a[3], Xc), __dmul_rn(g.a[4], Yc)), g.a[5]);
}

// clamp(min(x, S - x, y, S - y) / feather, 0, 1); 0 outside the quad, 1 inside it for feather <= 0
__device__ __forceinline__ float border_ramp(const UnalignGeom& g, double x, double y) {
    const double m = fmin(fmin(x, (double)g.S - x), fmin(y, (double)g.S - y));
    float alpha = 0.0f;
    if (m > 0.0) alpha = g.feather > 0.0f ? fminf((float)m / g.feather, 1.0f) : 1.0f;
    return alpha;
}

// o = clamp(floor(alpha e + (1 - alpha) p + 0.5), 0, 255), e = the Lanczos-3 resample of edit n at (x, y); alpha > 0 inside the quad.
// The tap weights differ from pixel to pixel (the map is rotated) but are separable inside one pixel: each thread keeps its x weights
// in its own LDS column (tap-major, so a wave reads 64 consecutive floats: no bank conflict), evaluates one y weight per tap row and
// accumulates weighted row sums.  wx_lds: [nt][BLK] floats, tid: this thread's column.  No barrier.
__device__ __forceinline__ void resample_composite(const UnalignGeom& g, const uint8_t* __restrict__ edits, int n, double x, double y, float alpha,
                                                   uint8_t p0, uint8_t p1, uint8_t p2, uint8_t* __restrict__ o, float* wx_lds, int tid) {
    int ilo, ihi, jlo, jhi;
    tap_range(x, g.support, g.S, ilo, ihi);
    tap_range(y, g.support, g.S, jlo, jhi);
    ihi = min(ihi, ilo + g.nt);                       // never cuts (an open interval of length 6 fs holds <= nt integers): keeps LDS in bounds
    const float dx0 = (float)((ilo + 0.5) - x), dy0 = (float)((jlo + 0.5) - y);
    float sumx = 0.0f;
    for (int t = 0; t < ihi - ilo; ++t) {
        const float w = lanczos3f((dx0 + (float)t) * g.inv_fs);
        wx_lds[t * BLK + tid] = w;
        sumx += w;
    }
    const uint8_t* e = edits + ((size_t)n * g.S * g.S + (size_t)jlo * g.S + ilo) * 3;
    float acc0 = 0.0f, acc1 = 0.0f, acc2 = 0.0f, sumy = 0.0f;
    for (int j = 0; j < jhi - jlo; ++j, e += (size_t)g.S * 3) {
        const float wy = lanczos3f((dy0 + (float)j) * g.inv_fs);
        float r0 = 0.0f, r1 = 0.0f, r2 = 0.0f;
        for (int t = 0; t < ihi - ilo; ++t) {
            const float w = wx_lds[t * BLK + tid];
            r0 += w * (float)e[3 * t];
            r1 += w * (float)e[3 * t + 1];
            r2 += w * (float)e[3 * t + 2];
        }
        acc0 += wy * r0, acc1 += wy * r1, acc2 += wy * r2;
        sumy += wy;
    }
    const float inv = 1.0f / (sumx * sumy);
    const float beta = 1.0f - alpha;
    const float v0 = floorf(alpha * (acc0 * inv) + beta * (float)p0 + 0.5f);
    const float v1 = floorf(alpha * (acc1 * inv) + beta * (float)p1 + 0.5f);
    const float v2 = floorf(alpha * (acc2 * inv) + beta * (float)p2 + 0.5f);
    o[0] = (uint8_t)(int)fminf(fmaxf(v0, 0.0f), 255.0f);
    o[1] = (uint8_t)(int)fminf(fmaxf(v1, 0.0f), 255.0f);
    o[2] = (uint8_t)(int)fminf(fmaxf(v2, 0.0f), 255.0f);
}

// out[n] = photo for every chunk of sizeof(T) bytes that is not wholly inside the bounding box (those bytes belong to the composite
// kernel).  bytes = H * W * 3 is a multiple of sizeof(T); row = W * 3 bytes; the box spans bytes [bx0, bx1) of rows [y0, y1).
template <typename T>
__global__ __launch_bounds__(BLK) void copy_outside_kernel(const T* __restrict__ photo, T* __restrict__ out, long long chunks, long long row,
                                                           long long bx0, long long bx1, int y0, int y1) {
    T* dst = out + (long long)blockIdx.y * chunks;
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < chunks; i += (long long)gridDim.x * BLK) {
        const long long b = i * (long long)sizeof(T);
        const long long r = b / row, c = b - r * row;
        if (r >= y0 && r < y1 && c >= bx0 && c + (long long)sizeof(T) <= bx1) continue;
        dst[i] = photo[i];
    }
}

template <typename T>
inline void launch_copy(const uint8_t* photo, uint8_t* out, const UnalignGeom& g, hipStream_t s) {
    const long long bytes = (long long)g.H * g.W * 3, chunks = bytes / (long long)sizeof(T);
    const long long blocks = (chunks + BLK - 1) / BLK;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048), (unsigned)g.N);
    copy_outside_kernel<T><<<grid, BLK, 0, s>>>(reinterpret_cast<const T*>(photo), reinterpret_cast<T*>(out), chunks, (long long)g.W * 3,
                                                 (long long)g.x0 * 3, (long long)g.x1 * 3, g.y0, g.y1);
}

// the widest chunk the pointers and the size allow
inline void copy_outside(const uint8_t* photo, uint8_t* out, const UnalignGeom& g, hipStream_t s) {
    const long long bytes = (long long)g.H * g.W * 3;
    const uintptr_t align = reinterpret_cast<uintptr_t>(photo) | reinterpret_cast<uintptr_t>(out) | (uintptr_t)bytes;
    if (align % 16 == 0) launch_copy<uint4>(photo, out, g, s);
    else if (align % 4 == 0) launch_copy<uint32_t>(photo, out, g, s);
    else launch_copy<uint8_t>(photo, out, g, s);
}

// The composite launch of kernel `k` (signature: photo, edits, extra, geom, out) with its dynamic LDS.
template <typename K, typename E>
inline hipError_t launch_composite(K k, const uint8_t* photo, const uint8_t* edits, E extra, const UnalignGeom& g, uint8_t* out, hipStream_t s) {
    const size_t lds = (size_t)g.nt * BLK * sizeof(float);
    if (lds > 65536) {                                // s > 10.5: more dynamic LDS than a launch gets without asking
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((g.x1 - g.x0 + TW - 1) / TW), (unsigned)((g.y1 - g.y0 + TH - 1) / TH), (unsigned)g.N);
    k<<<grid, dim3(TW, TH), lds, s>>>(photo, edits, extra, g, out);
    return hipGetLastError();
}

}  // namespace unalign
}  // namespace chk
