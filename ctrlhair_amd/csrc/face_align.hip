// face_align.hip -- FFHQ face alignment of one photo (external_code/crop.py:20-107 `recreate_aligned_images`) on gfx950.
//
// Three stages, each restating the arithmetic of the library the reference calls ("Face alignment"):
//   * Lanczos-3 resample of uint8 HWC images: Pillow's 8-bit path (Resample.c): double coefficient tables built on the host with
//     libm sin, normalised, rounded to 22 fractional bits; horizontal pass into a uint8 intermediate, then the vertical pass; int32
//     accumulation from 1 << 21, arithmetic shift, clip to 0..255.
//   * Image.transform(QUAD, BILINEAR) (Geometry.c quad_transform / bilinear_filter32RGB) in float64, fused into the horizontal Lanczos
//     pass: one workgroup evaluates one row of the transform grid into LDS and filters it at once; the transform_size^2 image never
//     reaches memory.
//   * the padding branch: np.pad(reflect) to float32, scipy.ndimage.gaussian_filter (correlate1d's symmetric loop, double
//     accumulation, float32 between the passes), the feather mask and the two blends as numpy evaluates them (float64 products,
//     float32 stores), np.median by an exact radix select, rint / clip / uint8.
// This file is compiled with -ffp-contract=off (Makefile): every product and sum above is a single IEEE operation, on the host
// (coefficient tables) and on the device.
#include "kernels.h"

#include <cmath>
#include <cstring>

namespace chk {
namespace {

constexpr int PREC = 22;                       // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int BLK = 256;

inline size_t up256(size_t n) { return (n + 255) & ~size_t(255); }

// ---- Lanczos tables (host) ------------------------------------------------------------------------------------------------------
double sinc_pi(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return std::sin(x) / x;
}
double lanczos3(double x) {
    if (-3.0 <= x && x < 3.0) return sinc_pi(x) * sinc_pi(x / 3);
    return 0.0;
}

void build_table(int in_size, int out_size, LanczosTable& t) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    t.in_size = in_size;
    t.out_size = out_size;
    t.ksize = ksize;
    t.data.assign((size_t)out_size * 2 + (size_t)out_size * ksize * 2, 0);
    int32_t* bounds = t.data.data();
    int32_t* kk = bounds + (size_t)out_size * 2;                 // [out][ksize]
    int32_t* kt = kk + (size_t)out_size * ksize;                 // [ksize][out]
    std::vector<double> k(ksize);
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = 0.0 + (xx + 0.5) * scale;
        double ww = 0.0;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        for (int x = 0; x < xmax; ++x) {
            const double w = lanczos3((x + xmin - center + 0.5) * ss);
            k[x] = w;
            ww += w;
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) k[x] /= ww;
            const double v = k[x];
            const int32_t q = v < 0 ? (int32_t)(-0.5 + v * (1 << PREC)) : (int32_t)(0.5 + v * (1 << PREC));
            kk[(size_t)xx * ksize + x] = q;
            kt[(size_t)x * out_size + xx] = q;
        }
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = xmax;
    }
}

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= PREC;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- Lanczos passes -------------------------------------------------------------------------------------------------------------
// src rows of `stride` bytes, C interleaved channels; kt [ksize][Wo]; dst [H][Wo][C]
__global__ __launch_bounds__(BLK) void lanczos_h_kernel(const uint8_t* __restrict__ src, long long stride, int H, int C,
                                                        const int* __restrict__ bounds, const int* __restrict__ kt, int Wo,
                                                        uint8_t* __restrict__ dst) {
    const int xo = blockIdx.x * BLK + threadIdx.x;
    if (xo >= Wo) return;
    const int xmin = bounds[2 * xo], n = bounds[2 * xo + 1];
    for (int y = blockIdx.y; y < H; y += gridDim.y) {
        const uint8_t* p = src + (long long)y * stride + (long long)xmin * C;
        int ss[4] = {1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1), 1 << (PREC - 1)};
        for (int t = 0; t < n; ++t) {
            const int k = kt[(long long)t * Wo + xo];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) ss[c] += (int)p[t * C + c] * k;
        }
        uint8_t* o = dst + ((long long)y * Wo + xo) * C;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) o[c] = clip8(ss[c]);
    }
}

// src: Hs rows of `sstride` bytes, the first rowlen used; kk [Ho][ksize]; dst [Ho][rowlen]
__global__ __launch_bounds__(BLK) void lanczos_v_kernel(const uint8_t* __restrict__ src, long long sstride, int rowlen, const int* __restrict__ bounds,
                                                        const int* __restrict__ kk, int ksize, int Ho, uint8_t* __restrict__ dst) {
    const int i = blockIdx.x * BLK + threadIdx.x;
    if (i >= rowlen) return;
    for (int yo = blockIdx.y; yo < Ho; yo += gridDim.y) {
        const int ymin = bounds[2 * yo], n = bounds[2 * yo + 1];
        const int* k = kk + (long long)yo * ksize;
        const uint8_t* p = src + (long long)ymin * sstride + i;
        int ss = 1 << (PREC - 1);
        for (int t = 0; t < n; ++t) ss += (int)p[(long long)t * sstride] * k[t];
        dst[(long long)yo * rowlen + i] = clip8(ss);
    }
}

// ---- quad transform (+ horizontal Lanczos) ----------------------------------------------------------------------------------------
struct QuadCoef {
    double a[8];
};

// Pillow's quad_transform + bilinear_filter32RGB for output pixel (x, y) of the T x T grid; rgb = 0 outside the source
__device__ __forceinline__ void quad_sample(const uint8_t* __restrict__ src, long long stride, int Hs, int Ws, const QuadCoef& q, int x,
                                            int y, uint8_t rgb[3]) {
    const double xin = x + 0.5, yin = y + 0.5;
    double xs = q.a[0] + q.a[1] * xin + q.a[2] * yin + q.a[3] * xin * yin;
    double ys = q.a[4] + q.a[5] * xin + q.a[6] * yin + q.a[7] * xin * yin;
    rgb[0] = rgb[1] = rgb[2] = 0;
    if (!(xs >= 0.0 && xs < (double)Ws && ys >= 0.0 && ys < (double)Hs)) return;      // also rejects NaN
    xs -= 0.5;
    ys -= 0.5;
    const int xi = xs < 0.0 ? (int)floor(xs) : (int)xs;
    const int yi = ys < 0.0 ? (int)floor(ys) : (int)ys;
    const double dx = xs - xi, dy = ys - yi;
    const int x0 = (xi < 0 ? 0 : (xi < Ws ? xi : Ws - 1)) * 3;
    const int x1 = (xi + 1 < 0 ? 0 : (xi + 1 < Ws ? xi + 1 : Ws - 1)) * 3;
    const int yc = yi < 0 ? 0 : (yi < Hs ? yi : Hs - 1);
    const uint8_t* r0 = src + (long long)yc * stride;
    const bool has1 = yi + 1 >= 0 && yi + 1 < Hs;
    const uint8_t* r1 = has1 ? src + (long long)(yi + 1) * stride : r0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double v1 = (double)r0[x0 + c] + (double)((int)r0[x1 + c] - (int)r0[x0 + c]) * dx;
        double v2 = v1;
        if (has1) v2 = (double)r1[x0 + c] + (double)((int)r1[x1 + c] - (int)r1[x0 + c]) * dx;
        v1 = v1 + (v2 - v1) * dy;
        rgb[c] = (uint8_t)(int)v1;
    }
}

// one workgroup per row of the transform grid: T samples into LDS, then the horizontal Lanczos pass T -> So.  dst [T][So][3]
__global__ __launch_bounds__(BLK) void quad_lanczos_h_kernel(const uint8_t* __restrict__ src, long long stride, int Hs, int Ws, QuadCoef q,
                                                             int T, const int* __restrict__ bounds, const int* __restrict__ kt, int So,
                                                             uint8_t* __restrict__ dst) {
    extern __shared__ uint8_t row[];              // [T][3]
    for (int y = blockIdx.x; y < T; y += gridDim.x) {
        for (int x = threadIdx.x; x < T; x += BLK) {
            uint8_t rgb[3];
            quad_sample(src, stride, Hs, Ws, q, x, y, rgb);
            row[3 * x] = rgb[0];
            row[3 * x + 1] = rgb[1];
            row[3 * x + 2] = rgb[2];
        }
        __syncthreads();
        for (int xo = threadIdx.x; xo < So; xo += BLK) {
            const int xmin = bounds[2 * xo], n = bounds[2 * xo + 1];
            const uint8_t* p = row + 3 * xmin;
            int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
            for (int t = 0; t < n; ++t) {
                const int k = kt[(long long)t * So + xo];
                s0 += (int)p[3 * t] * k;
                s1 += (int)p[3 * t + 1] * k;
                s2 += (int)p[3 * t + 2] * k;
            }
            uint8_t* o = dst + ((long long)y * So + xo) * 3;
            o[0] = clip8(s0);
            o[1] = clip8(s1);
            o[2] = clip8(s2);
        }
        __syncthreads();
    }
}

// output_size == transform_size: the transform itself.  dst [T][T][3]
__global__ __launch_bounds__(BLK) void quad_direct_kernel(const uint8_t* __restrict__ src, long long stride, int Hs, int Ws, QuadCoef q, int T,
                                                          uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * BLK + threadIdx.x;
    if (x >= T) return;
    for (int y = blockIdx.y; y < T; y += gridDim.y) {
        uint8_t rgb[3];
        quad_sample(src, stride, Hs, Ws, q, x, y, rgb);
        uint8_t* o = dst + ((long long)y * T + x) * 3;
        o[0] = rgb[0];
        o[1] = rgb[1];
        o[2] = rgb[2];
    }
}

// ---- padding branch -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect_np(int i, int n) {        // np.pad 'reflect': d c b | a b c d | c b a
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}
__device__ __forceinline__ int reflect_sp(int i, int n) {        // scipy 'reflect': c b a | a b c | c b a
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}

// P [Hp][Wp][3] float32 = np.pad(np.float32(src), reflect)
__global__ __launch_bounds__(BLK) void pad_reflect_kernel(const uint8_t* __restrict__ src, long long stride, int Hs, int Ws, int pl, int pt,
                                                          int Hp, int Wp, float* __restrict__ P) {
    const int i = blockIdx.x * BLK + threadIdx.x;             // x * 3 + c
    if (i >= Wp * 3) return;
    const int x = i / 3, c = i - 3 * x;
    const int sx = reflect_np(x - pl, Ws);
    for (int y = blockIdx.y; y < Hp; y += gridDim.y) {
        const int sy = reflect_np(y - pt, Hs);
        P[(long long)y * Wp * 3 + i] = (float)src[(long long)sy * stride + sx * 3 + c];
    }
}

// correlate1d along axis 0 / axis 1 of a [Hp][Wp][3] float32 image: symmetric weights w[0..2r], centre first, then the tap pairs from
// the outermost inwards, double accumulation, float32 store
template <int AXIS>
__global__ __launch_bounds__(BLK) void gauss_kernel(const float* __restrict__ in, const double* __restrict__ w, int r, int Hp, int Wp,
                                                    float* __restrict__ out) {
    const int i = blockIdx.x * BLK + threadIdx.x;             // x * 3 + c
    if (i >= Wp * 3) return;
    const int x = i / 3, c = i - 3 * x;
    const long long rowlen = (long long)Wp * 3;
    for (int y = blockIdx.y; y < Hp; y += gridDim.y) {
        double tmp = (double)in[y * rowlen + i] * w[r];
        for (int jj = -r; jj < 0; ++jj) {
            double a, b;
            if (AXIS == 0) {
                a = (double)in[reflect_sp(y + jj, Hp) * rowlen + i];
                b = (double)in[reflect_sp(y - jj, Hp) * rowlen + i];
            } else {
                a = (double)in[y * rowlen + reflect_sp(x + jj, Wp) * 3 + c];
                b = (double)in[y * rowlen + reflect_sp(x - jj, Wp) * 3 + c];
            }
            tmp += (a + b) * w[r + jj];
        }
        out[y * rowlen + i] = (float)tmp;
    }
}

struct PadGeom {
    int Hp, Wp, pl, pt, pr, pb;
};

// mask = max(1 - min(x / pl, (Wp - 1 - x) / pr), 1 - min(y / pt, (Hp - 1 - y) / pb)) in float64 (numpy promotes the float32 ramps
// divided by int64 pad widths to float64)
__device__ __forceinline__ double feather_mask(const PadGeom& g, int x, int y) {
    const double ax = (double)(float)x / (double)g.pl, bx = (double)(float)(g.Wp - 1 - x) / (double)g.pr;
    const double ay = (double)(float)y / (double)g.pt, by = (double)(float)(g.Hp - 1 - y) / (double)g.pb;
    const double mx = 1.0 - (ax < bx ? ax : bx), my = 1.0 - (ay < by ? ay : by);
    return mx > my ? mx : my;
}
__device__ __forceinline__ double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }

// img += (gauss - img) * clip(mask * 3 + 1, 0, 1): float32 difference, float64 product and sum, float32 store
__global__ __launch_bounds__(BLK) void blend_blur_kernel(float* __restrict__ P, const float* __restrict__ G, PadGeom g) {
    const int x = blockIdx.x * BLK + threadIdx.x;
    if (x >= g.Wp) return;
    for (int y = blockIdx.y; y < g.Hp; y += gridDim.y) {
        const double f = clip01(feather_mask(g, x, y) * 3.0 + 1.0);
        float* p = P + ((long long)y * g.Wp + x) * 3;
        const float* q = G + ((long long)y * g.Wp + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = q[c] - p[c];
            p[c] = (float)((double)p[c] + (double)d * f);
        }
    }
}

// ---- exact median: radix select over the float bits, 4 passes of 8 bits, 6 selections (3 channels x lower / upper middle) -------------
struct SelectState {
    unsigned prefix[6];
    unsigned krem[6];
    unsigned hist[6][256];
};

__device__ __forceinline__ unsigned float_key(float v) {          // monotone map float -> uint32
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ void select_init_kernel(SelectState* st, unsigned k_lo, unsigned k_hi) {
    for (int i = threadIdx.x; i < 6 * 256; i += blockDim.x) (&st->hist[0][0])[i] = 0;
    if (threadIdx.x < 6) {
        st->prefix[threadIdx.x] = 0;
        st->krem[threadIdx.x] = (threadIdx.x & 1) ? k_hi : k_lo;
    }
}

__global__ __launch_bounds__(BLK) void select_hist_kernel(const float* __restrict__ P, long long npix, SelectState* st, int shift,
                                                          unsigned himask) {
    __shared__ unsigned h[6][256];
    __shared__ unsigned pre[6];
    for (int i = threadIdx.x; i < 6 * 256; i += BLK) (&h[0][0])[i] = 0;
    if (threadIdx.x < 6) pre[threadIdx.x] = st->prefix[threadIdx.x];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * BLK + threadIdx.x; i < npix; i += (long long)gridDim.x * BLK) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned key = float_key(P[i * 3 + c]);
            const unsigned bin = (key >> shift) & 255u;
            if (((key ^ pre[2 * c]) & himask) == 0) atomicAdd(&h[2 * c][bin], 1u);
            if (((key ^ pre[2 * c + 1]) & himask) == 0) atomicAdd(&h[2 * c + 1][bin], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 6 * 256; i += BLK) {
        const unsigned v = (&h[0][0])[i];
        if (v) atomicAdd(&(&st->hist[0][0])[i], v);
    }
}

__global__ void select_scan_kernel(SelectState* st, int shift) {
    if (threadIdx.x < 6) {
        const int s = threadIdx.x;
        unsigned k = st->krem[s], cum = 0;
        int b = 0;
        for (; b < 255; ++b) {
            const unsigned n = st->hist[s][b];
            if (cum + n > k) break;
            cum += n;
        }
        st->prefix[s] |= (unsigned)b << shift;
        st->krem[s] = k - cum;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 6 * 256; i += blockDim.x) (&st->hist[0][0])[i] = 0;
}

// img += (median - img) * clip(mask, 0, 1), then uint8(clip(rint(img), 0, 255)).  dst [Hp][Wp][3]
__global__ __launch_bounds__(BLK) void blend_median_kernel(const float* __restrict__ P, const SelectState* __restrict__ st, PadGeom g,
                                                           uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * BLK + threadIdx.x;
    if (x >= g.Wp) return;
    float med[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float lo = key_float(st->prefix[2 * c]), hi = key_float(st->prefix[2 * c + 1]);
        med[c] = (lo + hi) / 2.0f;               // np.mean of the two middle values in float32 (the same value twice for an odd count)
    }
    for (int y = blockIdx.y; y < g.Hp; y += gridDim.y) {
        const double f = clip01(feather_mask(g, x, y));
        const float* p = P + ((long long)y * g.Wp + x) * 3;
        uint8_t* o = dst + ((long long)y * g.Wp + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = med[c] - p[c];
            float v = (float)((double)p[c] + (double)d * f);
            v = rintf(v);
            v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
            o[c] = (uint8_t)(int)v;
        }
    }
}

inline unsigned grid_y(int n) { return (unsigned)(n < 65535 ? n : 65535); }
inline unsigned cdiv(long long a, int b) { return (unsigned)((a + b - 1) / b); }

struct TableDev {
    const int *bounds, *kk, *kt;
    int ksize;
};

// copies the table of (in, out) to the workspace cursor
hipError_t upload_table(AlignCache& cache, int in_size, int out_size, char*& cur, TableDev& td, hipStream_t s) {
    const auto key = std::make_pair(in_size, out_size);
    auto it = cache.tables.find(key);
    if (it == cache.tables.end()) {
        if (cache.tables.size() >= 64) {          // tables of earlier calls may still be in flight to the device
            hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) return e;
            cache.tables.clear();
        }
        it = cache.tables.emplace(key, LanczosTable()).first;
        build_table(in_size, out_size, it->second);
    }
    const LanczosTable& t = it->second;
    const size_t bytes = t.data.size() * sizeof(int32_t);
    hipError_t e = hipMemcpyAsync(cur, t.data.data(), bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    td.bounds = reinterpret_cast<const int*>(cur);
    td.kk = td.bounds + (size_t)out_size * 2;
    td.kt = td.kk + (size_t)out_size * t.ksize;
    td.ksize = t.ksize;
    cur += up256(bytes);
    return hipSuccess;
}

size_t table_bytes(int in_size, int out_size) {
    const double scale = (double)in_size / out_size;
    const double support = 3.0 * (scale < 1.0 ? 1.0 : scale);
    const size_t ksize = (size_t)std::ceil(support) * 2 + 1;
    return up256(((size_t)out_size * 2 + (size_t)out_size * ksize * 2) * sizeof(int32_t));
}

}  // namespace

// ---- launchers ------------------------------------------------------------------------------------------------------------------
size_t lanczos_workspace_bytes(int Hs, int Ws, int C, int Hd, int Wd) {
    return table_bytes(Ws, Wd) + table_bytes(Hs, Hd) + up256((size_t)Hs * Wd * C);
}

hipError_t lanczos_resample_u8(AlignCache& cache, const uint8_t* src, long long stride, int Hs, int Ws, int C, uint8_t* dst, int Hd, int Wd,
                               void* ws, hipStream_t s) {
    char* cur = static_cast<char*>(ws);
    const bool need_h = Wd != Ws, need_v = Hd != Hs;
    const uint8_t* vin = src;
    long long vstride = stride;
    if (need_h) {
        TableDev th;
        hipError_t e = upload_table(cache, Ws, Wd, cur, th, s);
        if (e != hipSuccess) return e;
        uint8_t* hout = need_v ? reinterpret_cast<uint8_t*>(cur) : dst;
        if (need_v) cur += up256((size_t)Hs * Wd * C);
        lanczos_h_kernel<<<dim3(cdiv(Wd, BLK), grid_y(Hs)), BLK, 0, s>>>(src, stride, Hs, C, th.bounds, th.kt, Wd, hout);
        vin = hout;
        vstride = (long long)Wd * C;
    }
    if (need_v) {
        TableDev tv;
        hipError_t e = upload_table(cache, Hs, Hd, cur, tv, s);
        if (e != hipSuccess) return e;
        lanczos_v_kernel<<<dim3(cdiv((long long)Wd * C, BLK), grid_y(Hd)), BLK, 0, s>>>(vin, vstride, Wd * C, tv.bounds, tv.kk, tv.ksize, Hd, dst);
    }
    if (!need_h && !need_v) {
        hipError_t e = hipMemcpy2DAsync(dst, (size_t)Wd * C, src, (size_t)stride, (size_t)Wd * C, Hd, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    return hipGetLastError();
}

size_t quad_warp_workspace_bytes(int T, int S) { return S == T ? 0 : table_bytes(T, S) + up256((size_t)T * S * 3); }

hipError_t quad_warp_resample_u8(AlignCache& cache, const uint8_t* src, long long stride, int Hs, int Ws, const double* coef, int T, int S,
                                 uint8_t* dst, void* ws, hipStream_t s) {
    QuadCoef q;
    std::memcpy(q.a, coef, sizeof(q.a));
    if (S == T) {
        quad_direct_kernel<<<dim3(cdiv(T, BLK), grid_y(T)), BLK, 0, s>>>(src, stride, Hs, Ws, q, T, dst);
        return hipGetLastError();
    }
    char* cur = static_cast<char*>(ws);
    TableDev t;
    hipError_t e = upload_table(cache, T, S, cur, t, s);
    if (e != hipSuccess) return e;
    uint8_t* inter = reinterpret_cast<uint8_t*>(cur);
    quad_lanczos_h_kernel<<<dim3((unsigned)T), BLK, (size_t)T * 3, s>>>(src, stride, Hs, Ws, q, T, t.bounds, t.kt, S, inter);
    lanczos_v_kernel<<<dim3(cdiv((long long)S * 3, BLK), grid_y(S)), BLK, 0, s>>>(inter, (long long)S * 3, S * 3, t.bounds, t.kk, t.ksize, S, dst);
    return hipGetLastError();
}

size_t align_pad_workspace_bytes(int Hp, int Wp, int radius) {
    const size_t plane = up256((size_t)Hp * Wp * 3 * sizeof(float));
    return up256((size_t)(2 * radius + 1) * sizeof(double)) + up256(sizeof(SelectState)) + 3 * plane;
}

hipError_t align_pad_feather_u8(const uint8_t* src, long long stride, int Hs, int Ws, const int* pads, const double* gauss_w, int radius,
                                uint8_t* dst, void* ws, hipStream_t s) {
    PadGeom g;
    g.pl = pads[0], g.pt = pads[1], g.pr = pads[2], g.pb = pads[3];
    g.Hp = Hs + g.pt + g.pb;
    g.Wp = Ws + g.pl + g.pr;
    const size_t plane = up256((size_t)g.Hp * g.Wp * 3 * sizeof(float));
    char* cur = static_cast<char*>(ws);
    double* w = reinterpret_cast<double*>(cur);
    cur += up256((size_t)(2 * radius + 1) * sizeof(double));
    SelectState* st = reinterpret_cast<SelectState*>(cur);
    cur += up256(sizeof(SelectState));
    float* P = reinterpret_cast<float*>(cur);
    float* G0 = reinterpret_cast<float*>(cur + plane);
    float* G1 = reinterpret_cast<float*>(cur + 2 * plane);
    hipError_t e = hipMemcpyAsync(w, gauss_w, (size_t)(2 * radius + 1) * sizeof(double), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    const dim3 ge(cdiv((long long)g.Wp * 3, BLK), grid_y(g.Hp)), gp(cdiv(g.Wp, BLK), grid_y(g.Hp));
    pad_reflect_kernel<<<ge, BLK, 0, s>>>(src, stride, Hs, Ws, g.pl, g.pt, g.Hp, g.Wp, P);
    gauss_kernel<0><<<ge, BLK, 0, s>>>(P, w, radius, g.Hp, g.Wp, G0);
    gauss_kernel<1><<<ge, BLK, 0, s>>>(G0, w, radius, g.Hp, g.Wp, G1);
    blend_blur_kernel<<<gp, BLK, 0, s>>>(P, G1, g);
    const long long npix = (long long)g.Hp * g.Wp;
    select_init_kernel<<<1, BLK, 0, s>>>(st, (unsigned)((npix - 1) / 2), (unsigned)(npix / 2));
    const unsigned hb = cdiv(npix, BLK) < 1024u ? cdiv(npix, BLK) : 1024u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned himask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
        select_hist_kernel<<<hb, BLK, 0, s>>>(P, npix, st, shift, himask);
        select_scan_kernel<<<1, BLK, 0, s>>>(st, shift);
    }
    blend_median_kernel<<<gp, BLK, 0, s>>>(P, st, g, dst);
    return hipGetLastError();
}

// ---- the whole plan ---------------------------------------------------------------------------------------------------------------
size_t face_align_workspace_bytes(int H, int W, const AlignPlan& p, int radius) {
    size_t n = 0;
    if (p.shrink > 1) n += lanczos_workspace_bytes(H, W, 3, p.rh, p.rw) + up256((size_t)p.rh * p.rw * 3);
    if (p.do_pad) {
        const int Hp = (p.cy1 - p.cy0) + p.pt + p.pb, Wp = (p.cx1 - p.cx0) + p.pl + p.pr;
        n += align_pad_workspace_bytes(Hp, Wp, radius) + up256((size_t)Hp * Wp * 3);
    }
    return n + quad_warp_workspace_bytes(p.T, p.S);
}

hipError_t face_align(AlignCache& cache, const uint8_t* src, int H, int W, const AlignPlan& p, const double* gauss_w, int radius, uint8_t* dst,
                      void* ws, hipStream_t s) {
    char* cur = static_cast<char*>(ws);
    const uint8_t* img = src;
    long long stride = (long long)W * 3;
    hipError_t e;
    if (p.shrink > 1) {
        uint8_t* small = reinterpret_cast<uint8_t*>(cur);
        cur += up256((size_t)p.rh * p.rw * 3);
        e = lanczos_resample_u8(cache, img, stride, H, W, 3, small, p.rh, p.rw, cur, s);
        if (e != hipSuccess) return e;
        cur += lanczos_workspace_bytes(H, W, 3, p.rh, p.rw);
        img = small;
        stride = (long long)p.rw * 3;
    }
    img += (long long)p.cy0 * stride + (long long)p.cx0 * 3;          // the crop: an offset and a stride
    int h = p.cy1 - p.cy0, w = p.cx1 - p.cx0;
    if (p.do_pad) {
        const int pads[4] = {p.pl, p.pt, p.pr, p.pb};
        const int Hp = h + p.pt + p.pb, Wp = w + p.pl + p.pr;
        uint8_t* padded = reinterpret_cast<uint8_t*>(cur);
        cur += up256((size_t)Hp * Wp * 3);
        e = align_pad_feather_u8(img, stride, h, w, pads, gauss_w, radius, padded, cur, s);
        if (e != hipSuccess) return e;
        cur += align_pad_workspace_bytes(Hp, Wp, radius);
        img = padded;
        stride = (long long)Wp * 3;
        h = Hp;
        w = Wp;
    }
    return quad_warp_resample_u8(cache, img, stride, h, w, p.q, p.T, p.S, dst, cur, s);
}

}  // namespace chk
