// sheet.hip -- what a direction search does with its renders after the generator (shape_branch/script_find_direction.py:55-76,
// color_texture_branch/script_find_direction.py:55-74, util/canvas_grid.py:15-31), on the GPU:
//   sheet_compose   pastes n sources (float images, uint8 images or label maps through a colour table) into cells of a uint8 contact sheet
//   sweep_stats     exact int64 measurements of N renders: hair area, moments, bounding box, colour sums, and the differences to a
//                   reference render (changed labels, hair overlap / union, colour change inside the union)
// The float -> uint8 conversion is the project's to_u8 (pipeline.py edit_blended, hair_editor.py postprocess_blending_batch): x * 127.5 and
// + 127.5 each rounded to float32, clamped, truncated.  This file is compiled with -ffp-contract=off: a fused multiply-add rounds once and
// gives another byte for about two inputs in a million.  Everything measured is an integer, so block partials are combined with integer
// atomics and the result does not depend on the order in which blocks arrive.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>

#include "kernels.h"

namespace chk {

namespace {

constexpr int HAIR = 13;                       // CelebAMask-HQ hair id (hostutil.HAIR_IDX)

__device__ __forceinline__ uint8_t to_u8(float x) {
#pragma clang fp contract(off)
    const float a = x * 127.5f;
    const float b = a + 127.5f;
    return (uint8_t)(b > 0.f ? (b < 255.f ? b : 255.f) : 0.f);          // NaN fails b > 0: 0
}

// hostutil.resize_nearest: src = min((int)(dst * (in / out)), in - 1), the ratio in double
__device__ __forceinline__ int nearest(int d, double ratio, int n_in) {
    const int s = (int)(d * ratio);
    return s < n_in - 1 ? s : n_in - 1;
}

// one pixel of source image b as uint8 RGB.  kind 0: float32 planes [3,Hs,Ws]; kind 1: uint8 [Hs,Ws,3]
template <int KIND>
__device__ __forceinline__ void load_rgb(const void* __restrict__ src, size_t b, int Hs, int Ws, int sy, int sx, uint8_t c[3]) {
    const size_t plane = (size_t)Hs * Ws, at = (size_t)sy * Ws + sx;
    if (KIND == 0) {
        const float* p = static_cast<const float*>(src) + b * 3 * plane + at;
        c[0] = to_u8(p[0]);
        c[1] = to_u8(p[plane]);
        c[2] = to_u8(p[2 * plane]);
    } else {
        const uint8_t* p = static_cast<const uint8_t*>(src) + (b * plane + at) * 3;
        c[0] = p[0];
        c[1] = p[1];
        c[2] = p[2];
    }
}

}  // namespace

// ---- contact sheet ------------------------------------------------------------------------------------------------------
// Grid (row groups, n).  A block takes four rows of its cell at a time, one per wave.  A wave converts SHEET_TW pixels of its row -- lanes
// read neighbouring source pixels, three planes for a float source -- into a 3-byte interleaved run in its LDS slice, placed so that LDS
// offset and canvas address agree modulo 16; the run then leaves as aligned 16-byte stores with a byte-wise head and tail (a cell starts at
// byte j * (W + margin) * 3 of a row whose pitch need not be a multiple of four, so the alignment differs from cell to cell and row to row).
constexpr int SHEET_TW = 256;                                // pixels per wave and pass
constexpr int SHEET_SLICE = SHEET_TW * 3 + 32;               // bytes: the run plus its misalignment, rounded up to 16

template <int KIND>
__global__ __launch_bounds__(256) void sheet_compose_kernel(const void* __restrict__ src, int Hs, int Ws, const int* __restrict__ cells,
                                                            const uint8_t* __restrict__ lut, uint8_t* __restrict__ canvas, int rows, int cols,
                                                            int H, int W, int margin) {
    __shared__ uint4 stage[4 * SHEET_SLICE / 16];
    __shared__ uint8_t slut[768];
    const int b = blockIdx.y;
    const int ci = cells[2 * b], cj = cells[2 * b + 1];
    if (ci < 0 || ci >= rows || cj < 0 || cj >= cols) return;               // (uniform for the block: ahead of every barrier)
    if (KIND == 2) {
        for (int i = threadIdx.x; i < 768; i += blockDim.x) slut[i] = lut[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* buf = reinterpret_cast<uint8_t*>(stage) + wave * SHEET_SLICE;
    const size_t pitch = ((size_t)cols * W + (size_t)margin * (cols - 1)) * 3;
    const double ry = (double)Hs / (double)H, rx = (double)Ws / (double)W;
    const bool same = Hs == H && Ws == W;
    for (int y0 = blockIdx.x * 4; y0 < H; y0 += gridDim.x * 4) {            // (uniform trip count: the barriers below are reached by all)
        const int y = y0 + wave;
        const bool live = y < H;
        const int sy = live ? (same ? y : nearest(y, ry, Hs)) : 0;
        for (int x0 = 0; x0 < W; x0 += SHEET_TW) {
            const int tw = W - x0 < SHEET_TW ? W - x0 : SHEET_TW;
            uint8_t* d = canvas + ((size_t)ci * H + (live ? y : 0)) * pitch + ((size_t)cj * (W + margin) + x0) * 3;
            const int a = (int)(reinterpret_cast<uintptr_t>(d) & 15);
            if (live) {
                for (int p = lane; p < tw; p += 64) {
                    const int sx = same ? x0 + p : nearest(x0 + p, rx, Ws);
                    uint8_t c[3];
                    if (KIND == 2) {
                        const int l = static_cast<const uint8_t*>(src)[((size_t)b * Hs + sy) * Ws + sx];
                        c[0] = slut[3 * l];
                        c[1] = slut[3 * l + 1];
                        c[2] = slut[3 * l + 2];
                    } else {
                        load_rgb<KIND>(src, b, Hs, Ws, sy, sx, c);
                    }
                    uint8_t* o = buf + a + 3 * p;
                    o[0] = c[0];
                    o[1] = c[1];
                    o[2] = c[2];
                }
            }
            // A wave reads back only its own slice, so a wave-level fence would order this; the block barrier is kept because it is the
            // plain, well-defined way to make LDS bytes written by other lanes visible, both barriers are reached by all four waves (the
            // trip counts are uniform and the early return is per block), and at these sizes the call is bound by its launch, not by them.
            __syncthreads();
            if (live) {
                const int begin = a, end = a + 3 * tw;
                int vb = (begin + 15) & ~15, ve = end & ~15;
                if (vb > ve) vb = ve = end;                                 // shorter than one aligned chunk: all of it is head
                uint8_t* d0 = d - a;                                        // 16-byte aligned
                for (int m = begin + lane; m < vb; m += 64) d0[m] = buf[m];
                for (int m = vb + 16 * lane; m < ve; m += 16 * 64)
                    *reinterpret_cast<uint4*>(d0 + m) = *reinterpret_cast<const uint4*>(buf + m);
                for (int m = ve + lane; m < end; m += 64) d0[m] = buf[m];
            }
            __syncthreads();
        }
    }
}

hipError_t sheet_compose(const void* src, int kind, int n, int Hs, int Ws, const int* cells, const uint8_t* lut, uint8_t* canvas, int rows,
                         int cols, int H, int W, int margin, hipStream_t s) {
    int nb = (H + 3) / 4;
    nb = nb > 32 ? 32 : nb;
    const dim3 grid(nb, n), block(256);
    if (kind == 0)
        hipLaunchKernelGGL(sheet_compose_kernel<0>, grid, block, 0, s, src, Hs, Ws, cells, lut, canvas, rows, cols, H, W, margin);
    else if (kind == 1)
        hipLaunchKernelGGL(sheet_compose_kernel<1>, grid, block, 0, s, src, Hs, Ws, cells, lut, canvas, rows, cols, H, W, margin);
    else
        hipLaunchKernelGGL(sheet_compose_kernel<2>, grid, block, 0, s, src, Hs, Ws, cells, lut, canvas, rows, cols, H, W, margin);
    return hipGetLastError();
}

// ---- per-render measurements --------------------------------------------------------------------------------------------
// Layout of the CH_SWEEP_STATS int64 columns per render (include/ctrlhair_hip.h):
//   [0] hair pixels   [1..4] sum x, y, x^2, y^2 over hair   [5..8] y_min, y_max, x_min, x_max of hair (-1 without hair)
//   [9..11] sum R, G, B over hair   [12] pixels whose label differs from render ref[n]   [13] hair in both   [14] sum |dR| + |dG| + |dB| over
//   pixels that are hair in either   [15] hair in either   ([12..15] = 0 for ref[n] < 0)
// The minima start as -1 read as unsigned (the largest value) and take an unsigned atomicMin, the maxima start as -1 and take a signed
// atomicMax: a render without hair keeps -1 in all four with no pass over the output afterwards.
constexpr int NSW = SWEEP_NSTAT;

__global__ void sweep_stats_init_kernel(long long* __restrict__ stats, int total) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) {
        const int k = i % NSW;
        stats[i] = (k >= 5 && k <= 8) ? -1 : 0;
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void sweep_stats_kernel(const void* __restrict__ img, const uint8_t* __restrict__ labels,
                                                          const int* __restrict__ ref, int N, int H, int W, int h, int w,
                                                          long long* __restrict__ stats) {
    __shared__ long long part[4][NSW];
    const int n = blockIdx.y;
    int r = ref[n];
    if (r < 0 || r >= N) r = -1;                                            // (the entry point's callers check the range; never index with it)
    const uint8_t* lab = labels + (size_t)n * h * w;
    const uint8_t* labr = labels + (size_t)(r < 0 ? 0 : r) * h * w;
    const double ry = (double)h / (double)H, rx = (double)w / (double)W;
    const bool same = h == H && w == W;
    long long acc[NSW];
#pragma unroll
    for (int k = 0; k < NSW; ++k) acc[k] = 0;
    int ymin = INT_MAX, ymax = -1, xmin = INT_MAX, xmax = -1;
    const int HW = H * W;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += gridDim.x * blockDim.x) {
        const int y = p / W, x = p - y * W;
        const size_t at = same ? (size_t)p : (size_t)nearest(y, ry, h) * w + nearest(x, rx, w);
        const int l = lab[at];
        const bool hair = l == HAIR;
        uint8_t c[3] = {0, 0, 0};
        if (hair) {
            load_rgb<KIND>(img, n, H, W, y, x, c);
            acc[0] += 1;
            acc[1] += x;
            acc[2] += y;
            acc[3] += (long long)x * x;
            acc[4] += (long long)y * y;
            ymin = y < ymin ? y : ymin;
            ymax = y > ymax ? y : ymax;
            xmin = x < xmin ? x : xmin;
            xmax = x > xmax ? x : xmax;
            acc[9] += c[0];
            acc[10] += c[1];
            acc[11] += c[2];
        }
        if (r >= 0) {
            const int lr = labr[at];
            const bool hair_r = lr == HAIR;
            acc[12] += l != lr;
            acc[13] += hair && hair_r;
            if (hair || hair_r) {
                uint8_t e[3];
                if (!hair) load_rgb<KIND>(img, n, H, W, y, x, c);
                load_rgb<KIND>(img, r, H, W, y, x, e);
                acc[14] += abs((int)c[0] - (int)e[0]) + abs((int)c[1] - (int)e[1]) + abs((int)c[2] - (int)e[2]);
                acc[15] += 1;
            }
        }
    }
    acc[5] = ymin;
    acc[6] = ymax;
    acc[7] = xmin;
    acc[8] = xmax;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NSW; ++k) {
        long long v = acc[k];
        for (int off = 32; off > 0; off >>= 1) {
            const long long o = __shfl_xor(v, off, 64);
            v = (k == 5 || k == 7) ? (o < v ? o : v) : (k == 6 || k == 8) ? (o > v ? o : v) : v + o;
        }
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NSW) {
        const int k = threadIdx.x;
        long long t = part[0][k];
        for (int q = 1; q < 4; ++q) {
            const long long o = part[q][k];
            t = (k == 5 || k == 7) ? (o < t ? o : t) : (k == 6 || k == 8) ? (o > t ? o : t) : t + o;
        }
        long long* out = stats + (size_t)n * NSW + k;
        if (k == 5 || k == 7) {
            if (t != INT_MAX) atomicMin(reinterpret_cast<unsigned long long*>(out), (unsigned long long)t);
        } else if (k == 6 || k == 8) {
            if (t >= 0) atomicMax(out, t);
        } else if (t) {
            atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)t);
        }
    }
}

hipError_t sweep_stats(const void* img, int kind, const uint8_t* labels, const int* ref, int N, int H, int W, int h, int w, int64_t* stats,
                       hipStream_t s) {
    long long* out = reinterpret_cast<long long*>(stats);
    const int total = N * NSW;
    hipLaunchKernelGGL(sweep_stats_init_kernel, dim3((total + 255) / 256), dim3(256), 0, s, out, total);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    int64_t nb = ((int64_t)H * W + 256 * 8 - 1) / (256 * 8);                // ~8 pixels per thread
    nb = nb < 1 ? 1 : (nb > 64 ? 64 : nb);
    const dim3 grid((unsigned)nb, N), block(256);
    if (kind == 0)
        hipLaunchKernelGGL(sweep_stats_kernel<0>, grid, block, 0, s, img, labels, ref, N, H, W, h, w, out);
    else
        hipLaunchKernelGGL(sweep_stats_kernel<1>, grid, block, 0, s, img, labels, ref, N, H, W, h, w, out);
    return hipGetLastError();
}

}  // namespace chk
