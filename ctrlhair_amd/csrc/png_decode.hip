// ch_png_decode (include/ctrlhair_hip.h): N zlib streams -> N images, two kernels.
//
// png_inflate_kernel: one wavefront (a 64-thread workgroup) per stream.  Lane 0 runs pnginf::step (png_inflate_core.h) -- the bit reader
// over a 4 KiB window of the input in LDS, the Huffman tables in LDS, up to 128 tokens per round, each with its destination and each
// already checked against the bytes produced and the output bound -- and the whole wave carries the round out: literals lane-parallel,
// then the matches in token order, each copied by all lanes (byte i of a match is out[dst - dist + i mod dist], which exists before the
// match starts, so an overlapping match needs no inner order).  The output is the image's slice of the workspace in GLOBAL memory and
// match sources are read back from it: stores and the loads that depend on them are separated by a workgroup-scope fence (one wave, one
// CU, one L1: the fence is the wait for the stores), and the fence is skipped while a match's source lies wholly below the position up
// to which everything is known to be complete.  The Adler-32 is a reduction pass of the wave over the finished slice.
//
// png_unfilter_kernel: one wavefront per image, bands of 64 rows.  Lane j owns row r0 + j and runs one pixel behind lane j - 1: "up"
// arrives by a lane shift of the neighbour's last result, "left" and "up-left" stay in registers; lane 0 reads the last row of the band
// before from the image (fence between bands).  W + 63 steps per band, the filter type a per-lane select.
//
// Integer arithmetic only, no atomics, no communication between workgroups: image n is the same in every batch and every call.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "png_inflate_core.h"

namespace chk {
namespace {
namespace pi = pnginf;

constexpr int WIN = 4096;                  // bytes of input window in LDS (>= 2 * pi::STEP_INPUT)

struct InflateShared {
    pi::State st;
    pi::Token tok[pi::ROUND_TOKENS];
    alignas(16) uint8_t win[WIN];
    uint64_t wbase, wend;
    int result;
    uint32_t red[3][64];
};

__device__ inline void wg_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

__global__ __launch_bounds__(64) void png_inflate_kernel(const uint8_t* __restrict__ streams, const int64_t* __restrict__ offsets,
                                                         uint64_t out_len, uint64_t slice, uint8_t* ws, int32_t* __restrict__ status) {
    __shared__ InflateShared sh;
    const int n = blockIdx.x, lane = threadIdx.x;
    const int64_t lo = offsets[n], hi = offsets[n + 1];
    const uint64_t in_len = hi > lo ? (uint64_t)(hi - lo) : 0;
    const uint8_t* __restrict__ in = streams + lo;         // only [0, in_len) of it is ever read
    uint8_t* out = ws + (uint64_t)n * slice;               // only [0, out_len) of it is ever written
    if (lane == 0) {
        pi::init(sh.st, in_len, out_len);
        sh.wbase = sh.wend = 0;
    }
    __syncthreads();
    uint64_t complete = 0;                                 // every byte of out below this is stored and visible to the wave
    for (;;) {
        if (lane == 0) {
            pi::Window w{sh.win, sh.wbase, sh.wend};
            sh.result = pi::step(sh.st, w, sh.tok);
        }
        __syncthreads();
        const int r = sh.result;
        if (r == pi::DONE) break;
        if (r == pi::NEED_INPUT) {
            const uint64_t base = sh.st.in_pos & ~(uint64_t)3;                 // < in_len: step asks only while bytes are left
            const uint32_t len = (uint32_t)(in_len - base < (uint64_t)WIN ? in_len - base : (uint64_t)WIN);
            for (uint32_t o = lane * 16; o < len; o += 64 * 16) {
                if (o + 16 <= len) {
                    uint4 v;
                    memcpy(&v, in + base + o, 16);
                    *reinterpret_cast<uint4*>(sh.win + o) = v;
                } else {
                    for (uint32_t k = o; k < len; ++k) sh.win[k] = in[base + k];
                }
            }
            if (lane == 0) {
                sh.wbase = base;
                sh.wend = base + len;
            }
        } else if (r == pi::TOKENS) {
            const uint32_t cnt = sh.st.count;
            const uint64_t start = sh.st.out_start;
            for (uint32_t k0 = 0; k0 < cnt; k0 += 64) {
                const uint32_t k = k0 + lane;
                pi::Token t{0, 0, 0};
                if (k < cnt) t = sh.tok[k];
                if (k < cnt && t.len == 0) out[start + t.rel] = (uint8_t)t.val;
                unsigned long long matches = __ballot(k < cnt && t.len != 0);
                while (matches) {
                    const int m = __builtin_ctzll(matches);
                    matches &= matches - 1;
                    const uint32_t len = (uint32_t)__shfl((int)t.len, m), dist = (uint32_t)__shfl((int)t.val, m) + 1;
                    const uint64_t dst = start + (uint32_t)__shfl((int)t.rel, m), src = dst - dist;      // dist <= dst: checked by step
                    if (src + (len < dist ? len : dist) > complete) {
                        wg_fence();                        // everything stored so far (all of it lies below dst) is complete
                        complete = dst;
                    }
                    if (dist >= len) {
                        for (uint32_t i = lane; i < len; i += 64) out[dst + i] = out[src + i];
                    } else {
                        for (uint32_t i = lane; i < len; i += 64) out[dst + i] = out[src + i % dist];
                    }
                }
            }
        } else if (r == pi::STORED) {
            const uint32_t cnt = sh.st.count;
            const uint64_t dst = sh.st.out_start, src = sh.st.src;             // src + cnt <= in_len, dst + cnt <= out_len: checked by step
            for (uint32_t i = lane; i < cnt; i += 64) out[dst + i] = in[src + i];
        }
        __syncthreads();
    }
    int st = sh.st.status;
    if (st == pi::OK) {
        // Adler-32 of out[0, out_len): A = 1 + sum b, B = out_len + sum (out_len - i) b[i]; per 16-byte piece at i0 with s = sum b[k] and
        // q = sum k b[k]: (out_len - i0) s - q
        wg_fence();
        uint64_t sb = 0, p = 0, q = 0;
        uint64_t i0 = (uint64_t)lane * 16;
        uint32_t wgt = i0 < out_len ? (uint32_t)((out_len - i0) % pi::ADLER_MOD) : 0;
        for (; i0 < out_len; i0 += 64 * 16) {
            uint32_t s = 0, qq = 0;
            if (i0 + 16 <= out_len) {
                const uint4 v = *reinterpret_cast<const uint4*>(out + i0);     // the slice starts 16-byte aligned
                const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    const uint32_t b = (wd[k >> 2] >> (8 * (k & 3))) & 255;
                    s += b;
                    qq += k * b;
                }
            } else {
                for (uint32_t k = 0; i0 + k < out_len; ++k) {
                    const uint32_t b = out[i0 + k];
                    s += b;
                    qq += k * b;
                }
            }
            sb += s;
            p += (uint64_t)wgt * s;
            q += qq;
            wgt = wgt >= 1024 ? wgt - 1024 : wgt + pi::ADLER_MOD - 1024;      // (out_len - i0) mod 65521, 1024 bytes further
        }
        sh.red[0][lane] = (uint32_t)(sb % pi::ADLER_MOD);
        sh.red[1][lane] = (uint32_t)(p % pi::ADLER_MOD);
        sh.red[2][lane] = (uint32_t)(q % pi::ADLER_MOD);
        __syncthreads();
        if (lane == 0) {
            uint64_t tsb = 0, tp = 0, tq = 0;
            for (int l = 0; l < 64; ++l) {
                tsb += sh.red[0][l];
                tp += sh.red[1][l];
                tq += sh.red[2][l];
            }
            if (pi::adler_from_sums(tsb, tp % pi::ADLER_MOD + pi::ADLER_MOD - tq % pi::ADLER_MOD, out_len) != sh.st.adler_stored) st = pi::ADLER;
        }
    }
    if (lane == 0) status[n] = st;
}

__device__ inline uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

template <int C>
__global__ __launch_bounds__(64) void png_unfilter_kernel(const uint8_t* __restrict__ ws, uint64_t slice, int H, int W, uint8_t* img,
                                                          int32_t* status) {
    const int n = blockIdx.x, lane = threadIdx.x;
    if (status[n] != pi::OK) return;                       // the slice of a failed stream is not an image
    const uint64_t rb = (uint64_t)W * C, frb = rb + 1;
    const uint8_t* __restrict__ f = ws + (uint64_t)n * slice;
    uint8_t* o = img + (uint64_t)n * (uint64_t)H * rb;
    bool bad = false;
    for (int r0 = 0; r0 < H; r0 += 64) {
        if (r0) wg_fence();                                // row r0 - 1, written by lane 63 of the band before, is read by lane 0
        const int row = r0 + lane;
        const bool active = row < H;
        int ft = active ? f[(uint64_t)row * frb] : 0;
        if (ft > 4) {
            bad = true;
            ft = 0;
        }
        const uint8_t* __restrict__ fr = f + (uint64_t)(active ? row : 0) * frb + 1;
        uint8_t* orow = o + (uint64_t)(active ? row : 0) * rb;
        const uint8_t* prev = o + (uint64_t)(r0 ? r0 - 1 : 0) * rb;
        uint32_t left = 0, upleft = 0, cur = 0;            // pixels, channel c in bits 8c..8c+7
        for (int t = 0; t < W + 63; ++t) {
            const uint32_t above = (uint32_t)__shfl_up((int)cur, 1);           // the neighbour's pixel of step t - 1: this lane's x
            const int x = t - lane;
            const bool on = active && x >= 0 && x < W;
            uint32_t up = above;
            if (lane == 0) {
                up = 0;
                if (r0 && on)
                    for (int c = 0; c < C; ++c) up |= (uint32_t)prev[(uint64_t)x * C + c] << (8 * c);
            }
            if (on) {
                uint32_t res = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const uint32_t raw = fr[(uint64_t)x * C + c];
                    const uint32_t a = (left >> (8 * c)) & 255, b = (up >> (8 * c)) & 255, cc = (upleft >> (8 * c)) & 255;
                    const uint32_t pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : paeth(a, b, cc);
                    const uint32_t v = (raw + pred) & 255;
                    orow[(uint64_t)x * C + c] = (uint8_t)v;
                    res |= v << (8 * c);
                }
                upleft = up;
                left = res;
                cur = res;
            }
        }
    }
    if (bad) status[n] = pi::BAD_FILTER;
}

uint64_t png_decode_slice(int H, int W, int C) { return ((uint64_t)H * (1 + (uint64_t)W * C) + 15) & ~(uint64_t)15; }

}  // namespace

size_t png_decode_workspace_bytes(int N, int H, int W, int C) { return (size_t)N * png_decode_slice(H, W, C); }

hipError_t png_decode(const uint8_t* streams, const int64_t* offsets, int N, int H, int W, int C, uint8_t* img, int32_t* status, void* ws,
                      hipStream_t s) {
    const uint64_t out_len = (uint64_t)H * (1 + (uint64_t)W * C), slice = png_decode_slice(H, W, C);
    uint8_t* w = static_cast<uint8_t*>(ws);
    hipLaunchKernelGGL(png_inflate_kernel, dim3(N), dim3(64), 0, s, streams, offsets, out_len, slice, w, status);
    if (C == 1) hipLaunchKernelGGL(png_unfilter_kernel<1>, dim3(N), dim3(64), 0, s, w, slice, H, W, img, status);
    else if (C == 3) hipLaunchKernelGGL(png_unfilter_kernel<3>, dim3(N), dim3(64), 0, s, w, slice, H, W, img, status);
    else hipLaunchKernelGGL(png_unfilter_kernel<4>, dim3(N), dim3(64), 0, s, w, slice, H, W, img, status);
    return hipGetLastError();
}

}  // namespace chk
