// color_stats.hip -- hair colour statistics (dataset_scripts/script_get_rgb_hsv_label.py:52-63,
// script_get_color_var_label.py:52-90, hair_editor.py:233-243) on the GPU:
//   resize_linear_u8   cv2.resize(INTER_LINEAR) of uint8 images, OpenCV's fixed-point arithmetic (hostutil.resize_bilinear)
//   hair_erode         nearest resize of the label map (hostutil.resize_nearest), label == 13, cv2.erode with MORPH_ELLIPSE
//   hair_color_stats   exact int64 sums of the masked pixels: count, RGB moments 1-4, RGB cross products, HSV moments 1-2
// Everything is integer arithmetic on uint8 data, so the host can finish the reference's float64 statistics from the sums
// to the last bit (ctrlhair_amd/colorstats.py).  Integer sums make the result independent of the reduction order.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "kernels.h"
#include "linear_tap.h"

namespace chk {

// ---- uint8 bilinear resize (taps and weights of one axis: linear_tap.h) ---------------------------------------------------
// one thread per output pixel, all C channels: rows = a0 * p[x0] + a1 * p[x1] (int32), >> 4, then
// ((b0 * top) >> 16) + ((b1 * bot) >> 16) + 2 >> 2, saturated
__global__ __launch_bounds__(256) void resize_linear_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int Hs,
                                                               int Ws, int C, int Hd, int Wd) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, b = blockIdx.z;
    if (x >= Wd) return;
    int x0, x1, a0, a1, y0, y1, b0, b1;
    linear_tap(x, Wd, Ws, x0, x1, a0, a1);
    linear_tap(y, Hd, Hs, y0, y1, b0, b1);
    const uint8_t* s = src + (size_t)b * Hs * Ws * C;
    const uint8_t* r0 = s + (size_t)y0 * Ws * C;
    const uint8_t* r1 = s + (size_t)y1 * Ws * C;
    uint8_t* d = dst + (((size_t)b * Hd + y) * Wd + x) * C;
    for (int c = 0; c < C; ++c) {
        const int top = (r0[x0 * C + c] * a0 + r0[x1 * C + c] * a1) >> 4;
        const int bot = (r1[x0 * C + c] * a0 + r1[x1 * C + c] * a1) >> 4;
        int v = (((b0 * top) >> 16) + ((b1 * bot) >> 16) + 2) >> 2;
        d[c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

hipError_t resize_linear_u8(const uint8_t* src, uint8_t* dst, int B, int Hs, int Ws, int C, int Hd, int Wd, hipStream_t s) {
    hipLaunchKernelGGL(resize_linear_u8_kernel, dim3((Wd + 255) / 256, Hd, B), dim3(256), 0, s, src, dst, Hs, Ws, C, Hd, Wd);
    return hipGetLastError();
}

// ---- eroded hair mask ---------------------------------------------------------------------------------------------------
// A block owns a TW x TH output tile.  Its hair bits plus an R-pixel halo go to LDS (outside the image = set: cv2's default
// erosion border never erodes).  Horizontal pass: run[y][x] = the largest h <= R with the row segment [x-h, x+h] all set (-1
// when the pixel itself is clear).  Output = AND over dy of run[y+dy][x] >= hw[dy]: the element's row dy is the segment of
// half-width hw[dy].
constexpr int ER_TW = 64, ER_TH = 16;
constexpr int ER_EW = ER_TW + 2 * HAIR_ERODE_MAX_R, ER_EH = ER_TH + 2 * HAIR_ERODE_MAX_R;

__global__ __launch_bounds__(256) void hair_erode_kernel(const uint8_t* __restrict__ labels, int Hl, int Wl, int label,
                                                         HairErodeRows rows, uint8_t* __restrict__ mask, int H, int W) {
    __shared__ uint8_t bit[ER_EH * ER_EW];
    __shared__ int8_t run[ER_EH * ER_TW];
    const int R = rows.r, ew = ER_TW + 2 * R, eh = ER_TH + 2 * R;
    const int tx0 = blockIdx.x * ER_TW, ty0 = blockIdx.y * ER_TH, b = blockIdx.z;
    const uint8_t* lab = labels + (size_t)b * Hl * Wl;
    // hostutil.resize_nearest: src = min((int)(dst * (in / out)), in - 1), the ratio in double
    const double sy = (double)Hl / (double)H, sx = (double)Wl / (double)W;
    for (int i = threadIdx.x; i < eh * ew; i += blockDim.x) {
        const int ey = i / ew, ex = i - ey * ew;
        const int gy = ty0 + ey - R, gx = tx0 + ex - R;
        uint8_t v = 1;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            int ly = (int)(gy * sy), lx = (int)(gx * sx);
            ly = ly < Hl - 1 ? ly : Hl - 1;
            lx = lx < Wl - 1 ? lx : Wl - 1;
            v = lab[(size_t)ly * Wl + lx] == label;
        }
        bit[ey * ER_EW + ex] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < eh * ER_TW; i += blockDim.x) {
        const int ey = i / ER_TW, x = i - ey * ER_TW;
        const uint8_t* row = bit + ey * ER_EW + x + R;
        int h = row[0] ? 0 : -1;
        if (h == 0)
            while (h < R && row[-(h + 1)] && row[h + 1]) ++h;
        run[ey * ER_TW + x] = (int8_t)h;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ER_TH * ER_TW; i += blockDim.x) {
        const int y = i / ER_TW, x = i - y * ER_TW;
        const int gy = ty0 + y, gx = tx0 + x;
        if (gy >= H || gx >= W) continue;
        bool keep = true;
        for (int k = 0; k <= 2 * R && keep; ++k) keep = run[(y + k) * ER_TW + x] >= rows.hw[k];
        mask[((size_t)b * H + gy) * W + gx] = keep ? 1 : 0;
    }
}

hipError_t hair_erode(const uint8_t* labels, int B, int Hl, int Wl, int label, const HairErodeRows& rows, uint8_t* mask, int H, int W,
                      hipStream_t s) {
    hipLaunchKernelGGL(hair_erode_kernel, dim3((W + ER_TW - 1) / ER_TW, (H + ER_TH - 1) / ER_TH, B), dim3(256), 0, s, labels, Hl, Wl,
                       label, rows, mask, H, W);
    return hipGetLastError();
}

// ---- masked colour sums -------------------------------------------------------------------------------------------------
// Layout of the CH_COLOR_STATS int64 sums per image (include/ctrlhair_hip.h):
//   [0] n   [1..3] sum c   [4..6] sum c^2   [7..9] sum c^3   [10..12] sum c^4   [13..15] sum c0c1, c0c2, c1c2
//   [16..21] sum H, H^2, S, S^2, V, V^2   (cv2 RGB2HSV 8-bit: H in [0,180), S, V in [0,255])
constexpr int NSTAT = HAIR_COLOR_NSTAT;

__global__ __launch_bounds__(256) void hair_color_stats_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                               int64_t HW, unsigned long long* __restrict__ sums) {
    // OpenCV's 12-bit division tables of the 8-bit RGB -> HSV path (hostutil._SDIV / _HDIV)
    __shared__ int sdiv[256], hdiv[256];
    __shared__ long long part[4][NSTAT];
    for (int i = threadIdx.x; i < 256; i += blockDim.x) {
        sdiv[i] = i == 0 ? 0 : (int)rint((double)(255 << 12) / (double)i);
        hdiv[i] = i == 0 ? 0 : (int)rint((double)(180 << 12) / (6.0 * (double)i));
    }
    __syncthreads();
    const int b = blockIdx.y;
    const uint8_t* im = img + (size_t)b * HW * 3;
    const uint8_t* mk = mask + (size_t)b * HW;
    long long acc[NSTAT];
#pragma unroll
    for (int k = 0; k < NSTAT; ++k) acc[k] = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < HW; p += (int64_t)gridDim.x * blockDim.x) {
        if (!mk[p]) continue;
        const int c[3] = {im[p * 3], im[p * 3 + 1], im[p * 3 + 2]};
        acc[0] += 1;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const long long c1 = c[j], c2 = c1 * c1;
            acc[1 + j] += c1;
            acc[4 + j] += c2;
            acc[7 + j] += c2 * c1;
            acc[10 + j] += c2 * c2;
        }
        acc[13] += c[0] * c[1];
        acc[14] += c[0] * c[2];
        acc[15] += c[1] * c[2];
        const int r = c[0], g = c[1], bl = c[2];
        const int v = max(r, max(g, bl)), d = v - min(r, min(g, bl));
        int h = v == r ? g - bl : (v == g ? bl - r + 2 * d : r - g + 4 * d);
        h = (h * hdiv[d] + (1 << 11)) >> 12;
        if (h < 0) h += 180;
        const int sat = (d * sdiv[v] + (1 << 11)) >> 12;
        acc[16] += h;
        acc[17] += h * h;
        acc[18] += sat;
        acc[19] += sat * sat;
        acc[20] += v;
        acc[21] += v * v;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NSTAT; ++k) {
        long long a = acc[k];
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
        if (lane == 0) part[wave][k] = a;
    }
    __syncthreads();
    if (threadIdx.x < NSTAT) {
        const long long t = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (t) atomicAdd(sums + (size_t)b * NSTAT + threadIdx.x, (unsigned long long)t);
    }
}

hipError_t hair_color_stats(const uint8_t* img, const uint8_t* mask, int B, int H, int W, int64_t* sums, hipStream_t s) {
    hipError_t e = hipMemsetAsync(sums, 0, sizeof(int64_t) * NSTAT * (size_t)B, s);
    if (e != hipSuccess) return e;
    const int64_t HW = (int64_t)H * W;
    int64_t nb = (HW + 256 * 16 - 1) / (256 * 16);          // ~16 pixels per thread
    nb = nb < 1 ? 1 : (nb > 128 ? 128 : nb);
    hipLaunchKernelGGL(hair_color_stats_kernel, dim3((unsigned)nb, B), dim3(256), 0, s, img, mask, HW,
                       reinterpret_cast<unsigned long long*>(sums));
    return hipGetLastError();
}

}  // namespace chk
