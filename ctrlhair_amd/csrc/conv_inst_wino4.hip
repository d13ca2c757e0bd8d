// conv_inst_wino4.hip -- instantiation + launcher of the Winograd F(4x4,3x3) exact-f32 MFMA kernel (conv_wino4.h)
#include "conv_wino4v.h"
#include "conv_wino4_split.h"
#include "launch.h"

namespace chk {

hipError_t conv_wino4_plain(Wino4Params p, hipStream_t s) {
    if (!wino4_supported(p.H, p.W, p.Cin) || !p.in || !p.wpk || !p.out || (p.reflect && (p.res_up || p.H < 2 || p.W < 2))) return hipErrorInvalidValue;
    wino4_fill_launch(p);
    int cus = 0;
    hipError_t e = dyn_lds<wino4_plain_kernel<0>, wino4_plain_kernel<1>, wino4_plain_split_kernel<0>, wino4_plain_split_kernel<1>>(wino4::LDS_BYTES, &cus);
    if (e != hipSuccess) return e;
    const int grid = persistent_grid(p.ntasks, cus);
    // positions, not rows, split between the two waves of a tile group (conv_wino4_split.h): bit-identical results
    if (p.wpk_split && (p.split > 0 || (p.split < 0 && wino4_split_pays(p)))) {
        if (p.nks & 1) return hipErrorInvalidValue;
        if (p.reflect) hipLaunchKernelGGL(wino4_plain_split_kernel<1>, dim3(grid), dim3(512), wino4::LDS_BYTES, s, p);
        else hipLaunchKernelGGL(wino4_plain_split_kernel<0>, dim3(grid), dim3(512), wino4::LDS_BYTES, s, p);
        return hipGetLastError();
    }
    if (p.reflect) hipLaunchKernelGGL(wino4_plain_kernel<1>, dim3(grid), dim3(512), wino4::LDS_BYTES, s, p);
    else hipLaunchKernelGGL(wino4_plain_kernel<0>, dim3(grid), dim3(512), wino4::LDS_BYTES, s, p);
    return hipGetLastError();
}

hipError_t conv_wino4_ace(Wino4AceParams p, hipStream_t s) {
    if (!wino4_ace_supported(p.H, p.W, p.C) || !p.actv || !p.wpk || !p.out || !p.x || !p.noise) return hipErrorInvalidValue;
    p.nrt = (p.C + 15) / 16;
    p.ntx = p.W / wino4::TS;
    p.nty = p.H / wino4::TS;
    p.ntiles = p.B * p.ntx * p.nty;
    p.ntasks = p.ntiles * p.nrt;
    p.nks = p.wsty ? 38 : 32;
    p.rb = p.nrt >= 4 ? 4 : p.nrt;
    p.tbk = 32 / p.rb;
    int cus = 0;
    hipError_t e = dyn_lds<wino4_ace_kernel<0>>(wino4::LDS_BYTES, &cus);
    if (e != hipSuccess) return e;
    const int grid = persistent_grid(p.ntasks, cus);
    hipLaunchKernelGGL(wino4_ace_kernel<0>, dim3(grid), dim3(512), wino4::LDS_BYTES, s, p);
    return hipGetLastError();
}

// a0 b0 + a1 b1 + a2 b2 of the style-image transform G g G^T, with its roundings spelled out: fma(a2, b2, fma(a0, b0, a1 * b1)) is what
// hipcc made of the plain sum in the per-unit kernel (coefficients in registers); with the coefficients as literals (per-row kernel) it
// contracts the other product first.  Both kernels must give the same words.
__device__ __forceinline__ float wino4_dot3(float a0, float b0, float a1, float b1, float a2, float b2) {
    return __builtin_fmaf(a2, b2, __builtin_fmaf(a0, b0, a1 * b1));
}
// one thread = one 16-byte unit (idx, lane) of a style image: fragments a = 4 idx .. 4 idx + 3 = 36 m + xi of GEMM row 16 m + (lane & 15),
// input "channel" = label j = 4 s + (lane >> 4) (j >= 19, and the sixth image s = 5: zeros)
__global__ __launch_bounds__(256) void wino4_style_pack_kernel(const float* __restrict__ lut, float* __restrict__ wsty, int B, int C, int nrt) {
    const long long n = (long long)B * nrt * 6 * 1152;
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const int lane = (int)(i & 63), idx = (int)((i >> 6) % 18), s = (int)((i / 1152) % 6);
    const int rt = (int)((i / (1152 * 6)) % nrt), b = (int)(i / (1152LL * 6 * nrt));
    const int j = 4 * s + (lane >> 4);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    const int m = (4 * idx) / 36;                    // (36 % 4 == 0: the four fragments of a unit share the half)
    int ch, beta;
    wino4_ace_row(rt * 32 + m * 16 + (lane & 15), ch, beta);
    if (ch < C && j < 19 && s < 5) {
        const float* P = lut + ((long long)(b * 19 + j) * 9) * 2 * C + beta * C + ch;
        float g[3][3];
#pragma unroll
        for (int t = 0; t < 9; ++t) g[t / 3][t % 3] = P[(long long)t * 2 * C];
        const float Gm[6][3] = {{0.25f, 0.f, 0.f}, {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                                {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0.f, 0.f, 1.f}};
        float u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xi = 4 * idx + e - 36 * m, ii = xi / 6, jj = xi % 6;
            float r[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) r[q] = wino4_dot3(Gm[ii][0], g[0][q], Gm[ii][1], g[1][q], Gm[ii][2], g[2][q]);
            u[e] = wino4_dot3(r[0], Gm[jj][0], r[1], Gm[jj][1], r[2], Gm[jj][2]);
        }
        o = make_float4(u[0], u[1], u[2], u[3]);
    }
    reinterpret_cast<float4*>(wsty)[i] = o;
}
// one thread = one (GEMM row 32 rt + 16 m + (lane & 15), label j = 4 s + (lane >> 4)): its nine LUT values once, all 36 G g G^T values
// (each from the expression of the kernel above: the same words), nine 16-byte stores (units 9 m .. 9 m + 8 of its lane: a wave's store
// is a contiguous KB).  The units that are zero whatever B and C (s = 5; s = 4 with lane >= 48, i.e. j >= 19) are not written: their
// place in a [6][1152]-unit image depends on neither, and the buffer is zeroed once before its first use (sean_model.cpp).
__global__ __launch_bounds__(256) void wino4_style_pack_rows_kernel(const float* __restrict__ lut, float* __restrict__ wsty, int B, int C, int nrt) {
    const long long n = (long long)B * nrt * 5 * 128;
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= n) return;
    const int lane = (int)(i & 63), m = (int)((i >> 6) & 1), s = (int)((i >> 7) % 5);
    const int rt = (int)((i / 640) % nrt), b = (int)(i / (640LL * nrt));
    const int j = 4 * s + (lane >> 4);
    if (j >= 19) return;
    float4* dst = reinterpret_cast<float4*>(wsty) + (((long long)b * nrt + rt) * 6 + s) * 1152 + 9 * m * 64 + lane;
    int ch, beta;
    wino4_ace_row(rt * 32 + m * 16 + (lane & 15), ch, beta);
    if (ch >= C) {
#pragma unroll
        for (int k = 0; k < 9; ++k) dst[k * 64] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float* P = lut + ((long long)(b * 19 + j) * 9) * 2 * C + beta * C + ch;
    float g[3][3];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t / 3][t % 3] = P[(long long)t * 2 * C];
    const float Gm[6][3] = {{0.25f, 0.f, 0.f}, {-1.f / 6, -1.f / 6, -1.f / 6}, {-1.f / 6, 1.f / 6, -1.f / 6},
                            {1.f / 24, 1.f / 12, 1.f / 6}, {1.f / 24, -1.f / 12, 1.f / 6}, {0.f, 0.f, 1.f}};
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        float u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xi = 4 * k + e, ii = xi / 6, jj = xi % 6;
            float r[3];
#pragma unroll
            for (int q = 0; q < 3; ++q) r[q] = wino4_dot3(Gm[ii][0], g[0][q], Gm[ii][1], g[1][q], Gm[ii][2], g[2][q]);
            u[e] = wino4_dot3(r[0], Gm[jj][0], r[1], Gm[jj][1], r[2], Gm[jj][2]);
        }
        dst[k * 64] = make_float4(u[0], u[1], u[2], u[3]);
    }
}
// rows: 1 = wino4_style_pack_rows_kernel (wsty was zeroed once by the caller), 0 = one thread per 16-byte unit
hipError_t wino4_style_pack(const float* lut, float* wsty, int B, int C, hipStream_t s, int rows) {
    const int nrt = (C + 15) / 16;
    const long long n = rows ? (long long)B * nrt * 5 * 128 : (long long)B * nrt * 6 * 1152;
    if (rows) hipLaunchKernelGGL(wino4_style_pack_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lut, wsty, B, C, nrt);
    else hipLaunchKernelGGL(wino4_style_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lut, wsty, B, C, nrt);
    return hipGetLastError();
}


// ---- pre-transformed input route (conv_wino4v.h) ---------------------------------------------------------------------------------------
// the kernels' LDS limits from the first call of any of the launchers
static hipError_t wino4v_attr(int& cus) { return dyn_lds<wino4v_kernel<0>, wino4v_kernel<1>, wino4v_kernel<2>>(wino4v::LDS_BYTES, &cus); }
hipError_t wino4v_pack(const Wino4vPackParams& p, hipStream_t s) {
    if (!p.in || !p.v || p.H % 32 || p.W % 32 || p.H < 32 || p.W < 32 || p.nks <= 0 || p.pitch % 4 || p.xoff % 4 || (p.reflect && p.padded) || p.c0 < 0 || p.c0 % 4)
        return hipErrorInvalidValue;
    const long long blocks = (long long)p.B * (p.H / 32) * (p.W / 32) * p.nks;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wino4v_pack_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t conv_wino4v_plain(Wino4Params p, hipStream_t s) {
    if (!wino4_supported(p.H, p.W, p.Cin) || !p.v || !p.wpk || !p.out) return hipErrorInvalidValue;
    wino4_fill_launch(p);
    if (p.nks & 1) return hipErrorInvalidValue;
    // task order: a group of 32 consecutive tasks (one XCD, one L2) = 8 row tiles x 4 spatial tiles -- a V tile is twice an A image, so fewer
    // spatial tiles per group than conv_wino4.h's 4 x 8 (-DW4V_RB=2 / 4 / 8: level to +1 %, profiles/r06_wino4v_tuning.txt)
#ifndef W4V_RB
#define W4V_RB 8
#endif
    p.rb = p.nrt >= W4V_RB ? W4V_RB : p.nrt;
    p.tbk = 32 / p.rb;
    int cus = 0;
    hipError_t e = wino4v_attr(cus);
    if (e != hipSuccess) return e;
    const int grid = persistent_grid(p.ntasks, cus);
    hipLaunchKernelGGL(wino4v_kernel<0>, dim3(grid), dim3(512), wino4v::LDS_BYTES, s, p);
    return hipGetLastError();
}
static void wino4v_ace_fill(Wino4AceParams& p) {
    p.nrt = (p.C + 15) / 16;
    p.ntx = p.W / wino4::TS;
    p.nty = p.H / wino4::TS;
    p.ntiles = p.B * p.ntx * p.nty;
    p.ntasks = p.ntiles * p.nrt;
    p.nks = p.wsty ? 38 : 32;
    p.rb = p.nrt >= 4 ? 4 : p.nrt;
    p.tbk = 32 / p.rb;
}
hipError_t conv_wino4v_ace(Wino4AceParams p, hipStream_t s) {
    if (!wino4_ace_supported(p.H, p.W, p.C) || !p.v || !p.wpk || !p.out || !p.x || !p.noise) return hipErrorInvalidValue;
    wino4v_ace_fill(p);
    int cus = 0;
    hipError_t e = wino4v_attr(cus);
    if (e != hipSuccess) return e;
    const int grid = persistent_grid(p.ntasks, cus);
    hipLaunchKernelGGL(wino4v_kernel<1>, dim3(grid), dim3(512), wino4v::LDS_BYTES, s, p);
    return hipGetLastError();
}
// the same tasks in the same order; the cache is indexed by (spatial tile, row tile), so it must hold every task of the launch
hipError_t conv_wino4v_ace_memo(Wino4AceParams p, long long acc_tasks, hipStream_t s) {
    if (!wino4_ace_supported(p.H, p.W, p.C) || !p.v || !p.wpk || !p.out || !p.x || !p.noise) return hipErrorInvalidValue;
    if (!p.wsty || !p.v1h || !p.acc_cache || !p.memo_mode || (reinterpret_cast<uintptr_t>(p.acc_cache) & 15)) return hipErrorInvalidValue;
    wino4v_ace_fill(p);
    if (acc_tasks < p.ntasks) return hipErrorInvalidValue;
    int cus = 0;
    hipError_t e = wino4v_attr(cus);
    if (e != hipSuccess) return e;
    const int grid = persistent_grid(p.ntasks, cus);
    hipLaunchKernelGGL(wino4v_kernel<2>, dim3(grid), dim3(512), wino4v::LDS_BYTES, s, p);
    return hipGetLastError();
}

}  // namespace chk
