// face_unalign.hip -- paste N edited FFHQ-aligned crops back into the photo they were aligned from (the inverse of face_align.hip's
// geometry; the reference stops at the crop, so there is no upstream arithmetic to restate: DESIGN.md, "Paste-back").
//
// Per photo pixel (X, Y) of the quad's bounding box and per edit n:
//   (x, y) = A (X + 0.5, Y + 0.5, 1)                    crop coordinates, float64, left to right, no fused multiply-add
//   alpha  = clamp(min(x, S - x, y, S - y) / feather, 0, 1) [* bilinear(weight)(x, y) / 255]
//   e      = Lanczos-3 resample of the edit at (x, y) with filter scale fs = max(1, s): taps |i + 0.5 - x| < 3 fs, those outside
//            [0, S) dropped and the rest renormalised (Pillow's border rule); float32
//   out    = clamp(floor(alpha e + (1 - alpha) p + 0.5), 0, 255)
// The tap weights differ from pixel to pixel (the map is rotated) but are separable inside one pixel: each thread keeps its x weights
// in its own LDS column (tap-major, so a wave reads 64 consecutive floats: no bank conflict), evaluates one y weight per tap row and
// accumulates weighted row sums.  No barrier, no atomics, one workgroup per 32 x 8 tile and edit.
// Everything outside the bounding box is copied from the photo by copy_outside_kernel, 16 bytes per thread where the sizes allow.
#include "kernels.h"

namespace chk {
namespace {

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

__device__ __forceinline__ float weight_bilinear(const uint8_t* __restrict__ w, int S, float x, float y) {
    const float u = x - 0.5f, v = y - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float du = u - fu, dv = v - fv;
    const int i0 = min(max((int)fu, 0), S - 1), i1 = min(max((int)fu + 1, 0), S - 1);
    const int j0 = min(max((int)fv, 0), S - 1), j1 = min(max((int)fv + 1, 0), S - 1);
    const float a = (float)w[(size_t)j0 * S + i0], b = (float)w[(size_t)j0 * S + i1];
    const float c = (float)w[(size_t)j1 * S + i0], d = (float)w[(size_t)j1 * S + i1];
    const float top = a + (b - a) * du, bot = c + (d - c) * du;
    return (top + (bot - top) * dv) * (1.0f / 255.0f);
}

__global__ __launch_bounds__(BLK) void face_unalign_kernel(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ edits,
                                                           const uint8_t* __restrict__ weight, UnalignGeom g, uint8_t* __restrict__ out) {
    extern __shared__ float wx_lds[];                 // [nt][BLK]
    const int tid = threadIdx.y * TW + threadIdx.x;
    const int X = g.x0 + blockIdx.x * TW + threadIdx.x, Y = g.y0 + blockIdx.y * TH + threadIdx.y;
    if (X >= g.x1 || Y >= g.y1) return;
    const int n = blockIdx.z;
    const size_t pix = ((size_t)Y * g.W + X) * 3;
    const uint8_t* p = photo + pix;
    uint8_t* o = out + (size_t)n * g.H * g.W * 3 + pix;
    const uint8_t p0 = p[0], p1 = p[1], p2 = p[2];

    const double Xc = X + 0.5, Yc = Y + 0.5;
    const double x = __dadd_rn(__dadd_rn(__dmul_rn(g.a[0], Xc), __dmul_rn(g.a[1], Yc)), g.a[2]);
    const double y = __dadd_rn(__dadd_rn(__dmul_rn(g.a[3], Xc), __dmul_rn(g.a[4], Yc)), g.a[5]);
    const double m = fmin(fmin(x, (double)g.S - x), fmin(y, (double)g.S - y));
    float alpha = 0.0f;
    if (m > 0.0) alpha = g.feather > 0.0f ? fminf((float)m / g.feather, 1.0f) : 1.0f;
    if (alpha > 0.0f && weight) alpha *= weight_bilinear(weight, g.S, (float)x, (float)y);
    if (!(alpha > 0.0f)) {                            // outside the quad, or weight 0: the photo, untouched
        o[0] = p0, o[1] = p1, o[2] = p2;
        return;
    }

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

// out[n] = photo for every chunk of sizeof(T) bytes that is not wholly inside the bounding box (those bytes belong to
// face_unalign_kernel).  bytes = H * W * 3 is a multiple of sizeof(T); row = W * 3 bytes; the box spans bytes [bx0, bx1) of rows [y0, y1).
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
void launch_copy(const uint8_t* photo, uint8_t* out, const UnalignGeom& g, hipStream_t s) {
    const long long bytes = (long long)g.H * g.W * 3, chunks = bytes / (long long)sizeof(T);
    const long long blocks = (chunks + BLK - 1) / BLK;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048), (unsigned)g.N);
    copy_outside_kernel<T><<<grid, BLK, 0, s>>>(reinterpret_cast<const T*>(photo), reinterpret_cast<T*>(out), chunks, (long long)g.W * 3,
                                                 (long long)g.x0 * 3, (long long)g.x1 * 3, g.y0, g.y1);
}

}  // namespace

hipError_t face_unalign(const uint8_t* photo, const uint8_t* edits, const uint8_t* weight, const UnalignPlan& p, int H, int W, int N,
                        double feather_px, uint8_t* out, hipStream_t s) {
    UnalignGeom g;
    for (int i = 0; i < 6; ++i) g.a[i] = p.A[i];
    g.x0 = p.x0, g.y0 = p.y0, g.x1 = p.x1, g.y1 = p.y1;
    g.H = H, g.W = W, g.S = p.S, g.N = N;
    const double fs = p.scale > 1.0 ? p.scale : 1.0;
    g.nt = (int)(6.0 * fs) + 1;
    g.inv_fs = (float)(1.0 / fs);
    g.support = 3.0 * fs;
    g.feather = (float)feather_px;

    const long long bytes = (long long)H * W * 3;
    const uintptr_t align = reinterpret_cast<uintptr_t>(photo) | reinterpret_cast<uintptr_t>(out) | (uintptr_t)bytes;
    if (align % 16 == 0) launch_copy<uint4>(photo, out, g, s);
    else if (align % 4 == 0) launch_copy<uint32_t>(photo, out, g, s);
    else launch_copy<uint8_t>(photo, out, g, s);

    const size_t lds = (size_t)g.nt * BLK * sizeof(float);
    if (lds > 65536) {                                // s > 10.5: more dynamic LDS than a launch gets without asking
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(face_unalign_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const dim3 grid((unsigned)((g.x1 - g.x0 + TW - 1) / TW), (unsigned)((g.y1 - g.y0 + TH - 1) / TH), (unsigned)N);
    face_unalign_kernel<<<grid, dim3(TW, TH), lds, s>>>(photo, edits, weight, g, out);
    return hipGetLastError();
}

}  // namespace chk
