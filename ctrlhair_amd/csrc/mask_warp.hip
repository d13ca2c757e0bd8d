// mask_warp.hip -- hair-shape transfer warp (wrap_codes/mask_adaptor.py:87-143 hair_mask_transfer_wrap), batched:
//   arap_solve_kernel        one workgroup per pair: cotangent weights, vertex adjacency, then 100 x (local rotation fit, global
//                            Jacobi-PCG solve) of the per-element ARAP energy (libigl arap_precomputation / arap_solve, 2-D triangles)
//   uv_render_sample_kernel  one workgroup per 16x16 canvas tile: tile bin list in LDS, first covering triangle in face order,
//                            mesh_core.cpp's float32 barycentrics, edge fix, cv2.remap(INTER_LINEAR) of the padded 0/1 hair mask,
//                            truncation, crop and naive_transfer -> uint8 label map
// This file is compiled with -ffp-contract=off (Makefile): the rasteriser's inside test and colours must round like the reference's
// plain float arithmetic, and the ARAP residual is formed from equal sums that must cancel exactly.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace chk {
namespace {

constexpr int AT = 1024;                       // threads of the ARAP workgroup
constexpr int ROWS = WARP_MAX_V / AT;          // vertex rows a thread owns (row = tid + k * AT)
constexpr int CANVAS = 672, IMG = 512, BG = 80, EXT = 10, HAIR = 13;
constexpr int TILE = 16, TILES = CANVAS / TILE;

// Workspace of one pair (bytes, every part 256-aligned)
constexpr size_t WS_U = 0;                                             // float  [2 * MAX_V]   deformed positions, x then y planes
constexpr size_t WS_WCOT = WS_U + sizeof(float) * 2 * WARP_MAX_V;      // float  [3 * MAX_F]   0.5 * cot of the angle at corner k
constexpr size_t WS_SLOT = WS_WCOT + sizeof(float) * 3 * WARP_MAX_F;   // int    [3 * MAX_F]   vertex -> (triangle * 4 + corner), by row
constexpr size_t WS_COL = WS_SLOT + sizeof(int) * 3 * WARP_MAX_F;      // int    [6 * MAX_F]   two neighbours per slot
constexpr size_t WS_VAL = WS_COL + sizeof(int) * 6 * WARP_MAX_F;       // float  [6 * MAX_F]   their edge weights
constexpr size_t WS_PAIR = WS_VAL + sizeof(float) * 6 * WARP_MAX_F;
static_assert(WS_PAIR % 256 == 0, "per-pair workspace must keep 256-byte alignment");
// The workspace starts with the B descriptors (6 ints per pair, copied there from kernel arguments), then B pair blocks
__host__ __device__ inline size_t ws_head(int B) { return ((size_t)B * 6 * sizeof(int) + 255) / 256 * 256; }

// Descriptors reach the device as kernel arguments, WARP_DESC_PAIRS pairs per launch of this kernel (no host buffer has to
// outlive the call, nothing is copied from pageable memory); every later kernel covers the whole batch in ONE launch.
__global__ void warp_store_desc_kernel(WarpDesc desc, int* __restrict__ dst) {
    const int i = threadIdx.x;
    if (i < desc.n * 6) dst[desc.pair0 * 6 + i] = desc.d[i / 6][i % 6];
}

// ch_mask_warp_batch_dev: the descriptors are in device memory.  Copied to the same place, and validated on the way (the host
// entry point does this before it launches): a pair whose counts or offsets are out of range gets the all-zero descriptor, for
// which the solver does nothing and the renderer draws the identity map.
__global__ void warp_copy_desc_kernel(const int* __restrict__ src, int B, int* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    int d[6];
    for (int k = 0; k < 6; ++k) d[k] = src[6 * i + k];
    const bool ok = d[0] >= 0 && d[2] >= 0 && d[4] >= 0 && d[1] >= 3 && d[1] <= WARP_MAX_V && d[3] >= 1 && d[3] <= WARP_MAX_F &&
                    d[5] >= 0 && d[5] <= WARP_MAX_V;
    for (int k = 0; k < 6; ++k) dst[6 * i + k] = ok ? d[k] : 0;
}

// Sum of two doubles per thread over the workgroup, the same value in every thread: butterfly-free fixed tree (shuffle down
// inside each wave, then the 16 wave sums added in wave order), so the result does not depend on timing.  `buf` alternates
// between calls so that one barrier per reduction is enough.
__device__ inline void block_sum2(double& a, double& b, double (*red)[AT / 64][2], int& buf) {
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[buf][wave][0] = a;
        red[buf][wave][1] = b;
    }
    __syncthreads();
    a = 0.0;
    b = 0.0;
    for (int w = 0; w < AT / 64; ++w) {
        a += red[buf][w][0];
        b += red[buf][w][1];
    }
    buf ^= 1;
}

__global__ __launch_bounds__(AT) void arap_solve_kernel(const float* __restrict__ V, const int* __restrict__ F,
                                                        const int* __restrict__ bidx, const float* __restrict__ bc, int B,
                                                        char* __restrict__ ws, float* __restrict__ U_out, int outer_iters, int max_cg,
                                                        float rel_tol) {
    __shared__ float sUx[WARP_MAX_V], sUy[WARP_MAX_V], sPx[WARP_MAX_V], sPy[WARP_MAX_V];
    __shared__ float2 sRot[WARP_MAX_F];        // (cos, sin) per element; the set-up phase uses it as integer scratch
    __shared__ unsigned char sCon[WARP_MAX_V];
    __shared__ double sRed[2][AT / 64][2];
    __shared__ int sBad;

    const int tid = threadIdx.x;
    const int* d = reinterpret_cast<const int*>(ws) + 6 * blockIdx.x;
    const int nV = d[1], nF = d[3], nB = d[5];
    const float* Vp = V + 2 * (size_t)d[0];
    const int* Fp = F + 3 * (size_t)d[2];
    const int* bp = bidx + d[4];
    const float* bcp = bc + 2 * (size_t)d[4];
    char* wp = ws + ws_head(B) + (size_t)blockIdx.x * WS_PAIR;
    float* Uw = reinterpret_cast<float*>(wp + WS_U);
    float* wcot = reinterpret_cast<float*>(wp + WS_WCOT);
    int* slots = reinterpret_cast<int*>(wp + WS_SLOT);
    int* col = reinterpret_cast<int*>(wp + WS_COL);
    float* val = reinterpret_cast<float*>(wp + WS_VAL);
    float* Uo = U_out ? U_out + 2 * (size_t)d[0] : nullptr;
    int* sCnt = reinterpret_cast<int*>(sRot);  // [MAX_V]     incident triangles per vertex, then the fill cursor
    int* sPtr = sCnt + WARP_MAX_V;             // [MAX_V + 1] exclusive scan of the counts
    static_assert(sizeof(int) * (2 * WARP_MAX_V + 1) <= sizeof(float2) * WARP_MAX_F, "set-up scratch must fit in sRot");

    // ---- validate the indices (memory safety; the host checks the counts) and load the rest pose ------------------------
    if (tid == 0) sBad = 0;
    __syncthreads();
    for (int t = tid; t < nF; t += AT)
        for (int k = 0; k < 3; ++k) {
            const int v = Fp[3 * t + k];
            if (v < 0 || v >= nV) sBad = 1;
        }
    for (int i = tid; i < nB; i += AT)
        if (bp[i] < 0 || bp[i] >= nV) sBad = 1;
    for (int i = tid; i < WARP_MAX_V; i += AT) {
        const bool in = i < nV;
        sUx[i] = in ? Vp[2 * i] : 0.f;
        sUy[i] = in ? Vp[2 * i + 1] : 0.f;
        sPx[i] = 0.f;
        sPy[i] = 0.f;
        sCon[i] = 0;
        sCnt[i] = 0;
    }
    __syncthreads();
    if (sBad) {                                // uniform: a mesh with indices out of range is returned undeformed
        for (int i = tid; i < nV; i += AT) {
            Uw[i] = sUx[i];
            Uw[WARP_MAX_V + i] = sUy[i];
            if (Uo) {
                Uo[2 * i] = sUx[i];
                Uo[2 * i + 1] = sUy[i];
            }
        }
        return;
    }

    // ---- set-up: cotangent weights (f64, rounded once), constraints, vertex -> triangle adjacency in ascending order -----
    for (int t = tid; t < nF; t += AT) {
        int v[3];
        double x[3], y[3];
        for (int k = 0; k < 3; ++k) {
            v[k] = Fp[3 * t + k];
            x[k] = Vp[2 * v[k]];
            y[k] = Vp[2 * v[k] + 1];
            atomicAdd(&sCnt[v[k]], 1);
        }
        const double area2 = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]);
        for (int k = 0; k < 3; ++k) {
            const int a = (k + 1) % 3, b = (k + 2) % 3;
            const double dot = (x[a] - x[k]) * (x[b] - x[k]) + (y[a] - y[k]) * (y[b] - y[k]);
            wcot[3 * t + k] = area2 != 0.0 ? (float)(0.5 * dot / fabs(area2)) : 0.f;
        }
    }
    __syncthreads();
    for (int i = tid; i < nB; i += AT) {       // after the barrier: the weights above are those of the rest pose
        const int v = bp[i];
        sUx[v] = bcp[2 * i];
        sUy[v] = bcp[2 * i + 1];
        sCon[v] = 1;
    }
    if (tid < 64) {                            // exclusive scan of MAX_V counts by one wave: 32 per lane, then across the lanes
        constexpr int PER = WARP_MAX_V / 64;
        int sum = 0;
        for (int j = 0; j < PER; ++j) sum += sCnt[tid * PER + j];
        int incl = sum;
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off);
            if (tid >= off) incl += o;
        }
        int run = incl - sum;
        for (int j = 0; j < PER; ++j) {
            sPtr[tid * PER + j] = run;
            run += sCnt[tid * PER + j];
        }
        if (tid == 63) sPtr[WARP_MAX_V] = run;
    }
    __syncthreads();
    for (int i = tid; i < WARP_MAX_V; i += AT) sCnt[i] = 0;
    __syncthreads();
    for (int t = tid; t < nF; t += AT)
        for (int k = 0; k < 3; ++k) {
            const int v = Fp[3 * t + k];
            slots[sPtr[v] + atomicAdd(&sCnt[v], 1)] = t * 4 + k;
        }
    __syncthreads();
    int rs[ROWS], re[ROWS];
    float diag[ROWS];
    bool fr[ROWS];
    for (int k = 0; k < ROWS; ++k) {
        const int i = tid + k * AT;
        rs[k] = sPtr[i];
        re[k] = sPtr[i + 1];
        fr[k] = i < nV && !sCon[i] && re[k] > rs[k];
        for (int a = rs[k] + 1; a < re[k]; ++a) {      // insertion sort: the order the atomics produced is not repeatable
            const int key = slots[a];
            int b = a - 1;
            while (b >= rs[k] && slots[b] > key) {
                slots[b + 1] = slots[b];
                --b;
            }
            slots[b + 1] = key;
        }
        float dsum = 0.f;
        for (int a = rs[k]; a < re[k]; ++a) {
            const int t = slots[a] >> 2, c = slots[a] & 3, c1 = (c + 1) % 3, c2 = (c + 2) % 3;
            const float w1 = wcot[3 * t + c2], w2 = wcot[3 * t + c1];     // edge (i, j1) faces corner c2, edge (i, j2) corner c1
            col[2 * a] = Fp[3 * t + c1];
            col[2 * a + 1] = Fp[3 * t + c2];
            val[2 * a] = w1;
            val[2 * a + 1] = w2;
            dsum += w1;
            dsum += w2;
        }
        diag[k] = dsum;
        if (!(dsum > 0.f)) fr[k] = false;      // an isolated or degenerate row keeps its rest position
    }
    __syncthreads();                           // sRot is free for the rotations from here on

    int buf = 0;
    const double tol2 = (double)rel_tol * (double)rel_tol;
    for (int outer = 0; outer < outer_iters; ++outer) {
        // ---- local step: R_t = rotation of the polar decomposition of S = sum_e w_e (u_e)(v_e)^T, closed form in 2-D ------
        for (int t = tid; t < nF; t += AT) {
            int v[3];
            float vx[3], vy[3], ux[3], uy[3];
            for (int k = 0; k < 3; ++k) {
                v[k] = Fp[3 * t + k];
                vx[k] = Vp[2 * v[k]];
                vy[k] = Vp[2 * v[k] + 1];
                ux[k] = sUx[v[k]];
                uy[k] = sUy[v[k]];
            }
            float a = 0.f, b = 0.f;            // a = S00 + S11, b = S10 - S01
            for (int k = 0; k < 3; ++k) {
                const int i = (k + 1) % 3, j = (k + 2) % 3;
                const float w = wcot[3 * t + k];
                const float ex = ux[i] - ux[j], ey = uy[i] - uy[j], rx = vx[i] - vx[j], ry = vy[i] - vy[j];
                a += w * (ex * rx + ey * ry);
                b += w * (ey * rx - ex * ry);
            }
            const float n = sqrtf(a * a + b * b);
            sRot[t] = n > 0.f ? make_float2(a / n, b / n) : make_float2(1.f, 0.f);
        }
        __syncthreads();

        // ---- global step: L u = rhs on the free rows, constrained neighbours keep their targets -------------------------
        float rx[ROWS], ry[ROWS], zx[ROWS], zy[ROWS];
        double bb = 0.0, rr = 0.0;
        for (int k = 0; k < ROWS; ++k) {
            rx[k] = ry[k] = 0.f;
            if (!fr[k]) continue;
            const int i = tid + k * AT;
            const float vix = Vp[2 * i], viy = Vp[2 * i + 1], uix = sUx[i], uiy = sUy[i];
            float bx = 0.f, by = 0.f, lx = 0.f, ly = 0.f, cx = 0.f, cy = 0.f;
            for (int a = rs[k]; a < re[k]; ++a) {
                const float2 R = sRot[slots[a] >> 2];
                for (int e = 0; e < 2; ++e) {
                    const int j = col[2 * a + e];
                    const float w = val[2 * a + e];
                    const float dx = vix - Vp[2 * j], dy = viy - Vp[2 * j + 1];
                    bx += w * (R.x * dx - R.y * dy);
                    by += w * (R.y * dx + R.x * dy);
                    lx += w * (uix - sUx[j]);
                    ly += w * (uiy - sUy[j]);
                    if (sCon[j]) {
                        cx += w * sUx[j];
                        cy += w * sUy[j];
                    }
                }
            }
            rx[k] = bx - lx;
            ry[k] = by - ly;
            bb += (double)(bx + cx) * (bx + cx) + (double)(by + cy) * (by + cy);
            rr += (double)rx[k] * rx[k] + (double)ry[k] * ry[k];
        }
        block_sum2(bb, rr, sRed, buf);
        const double thr = tol2 * bb;
        if (rr > thr) {
            double rz = 0.0, dummy = 0.0;
            for (int k = 0; k < ROWS; ++k) {
                if (!fr[k]) continue;
                const int i = tid + k * AT;
                zx[k] = rx[k] / diag[k];
                zy[k] = ry[k] / diag[k];
                sPx[i] = zx[k];
                sPy[i] = zy[k];
                rz += (double)rx[k] * zx[k] + (double)ry[k] * zy[k];
            }
            block_sum2(rz, dummy, sRed, buf);  // its barrier also publishes p
            for (int it = 0; it < max_cg; ++it) {
                float ax[ROWS], ay[ROWS];
                double pAp = 0.0;
                dummy = 0.0;
                for (int k = 0; k < ROWS; ++k) {
                    if (!fr[k]) continue;
                    const int i = tid + k * AT;
                    const float pix = sPx[i], piy = sPy[i];
                    float sx = 0.f, sy = 0.f;
                    for (int a = 2 * rs[k]; a < 2 * re[k]; ++a) {
                        const int j = col[a];
                        const float w = val[a];
                        sx += w * (pix - sPx[j]);          // p is 0 on constrained rows
                        sy += w * (piy - sPy[j]);
                    }
                    ax[k] = sx;
                    ay[k] = sy;
                    pAp += (double)pix * sx + (double)piy * sy;
                }
                block_sum2(pAp, dummy, sRed, buf);         // every read of p is behind this barrier
                if (!(pAp > 0.0)) break;
                const float alpha = (float)(rz / pAp);
                double rz_new = 0.0;
                rr = 0.0;
                for (int k = 0; k < ROWS; ++k) {
                    if (!fr[k]) continue;
                    const int i = tid + k * AT;
                    sUx[i] += alpha * sPx[i];
                    sUy[i] += alpha * sPy[i];
                    rx[k] -= alpha * ax[k];
                    ry[k] -= alpha * ay[k];
                    zx[k] = rx[k] / diag[k];
                    zy[k] = ry[k] / diag[k];
                    rz_new += (double)rx[k] * zx[k] + (double)ry[k] * zy[k];
                    rr += (double)rx[k] * rx[k] + (double)ry[k] * ry[k];
                }
                block_sum2(rz_new, rr, sRed, buf);
                if (rr <= thr) break;
                const float beta = (float)(rz_new / rz);
                rz = rz_new;
                for (int k = 0; k < ROWS; ++k) {
                    if (!fr[k]) continue;
                    const int i = tid + k * AT;
                    sPx[i] = zx[k] + beta * sPx[i];
                    sPy[i] = zy[k] + beta * sPy[i];
                }
                __syncthreads();
            }
        }
        __syncthreads();                       // u complete before the next local step
    }
    for (int i = tid; i < nV; i += AT) {
        Uw[i] = sUx[i];
        Uw[WARP_MAX_V + i] = sUy[i];
        if (Uo) {
            Uo[2 * i] = sUx[i];
            Uo[2 * i + 1] = sUy[i];
        }
    }
}

// U given by the caller (ch_mask_warp_batch U_in): copied into the workspace layout the renderer reads
__global__ void warp_load_u_kernel(const float* __restrict__ U_in, int B, char* __restrict__ ws, float* __restrict__ U_out) {
    const int* d = reinterpret_cast<const int*>(ws) + 6 * blockIdx.y;
    float* Uw = reinterpret_cast<float*>(ws + ws_head(B) + (size_t)blockIdx.y * WS_PAIR + WS_U);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < d[1]; i += gridDim.x * blockDim.x) {
        const float x = U_in[2 * ((size_t)d[0] + i)], y = U_in[2 * ((size_t)d[0] + i) + 1];
        Uw[i] = x;
        Uw[WARP_MAX_V + i] = y;
        if (U_out) {
            U_out[2 * ((size_t)d[0] + i)] = x;
            U_out[2 * ((size_t)d[0] + i) + 1] = y;
        }
    }
}

// mask_adaptor.py:119-131: the 0/1 hair mask on the 672 x 672 canvas, hair that touches an image edge extended 10 px into the border
// (rows first, then columns, so the corners follow the extended rows); 0 outside the canvas (cv2.remap's constant border)
__device__ inline bool rows_mask(const uint8_t* hair, int r, int c) {
    if (c < BG || c >= BG + IMG) return false;
    if (r < BG - EXT || r >= BG + IMG + EXT) return false;
    const int y = r < BG ? 0 : (r >= BG + IMG ? IMG - 1 : r - BG);
    return hair[y * IMG + (c - BG)] == HAIR;
}
__device__ inline bool padded_mask(const uint8_t* hair, int r, int c) {
    if (r < 0 || r >= CANVAS || c < 0 || c >= CANVAS) return false;
    if (c >= BG - EXT && c < BG) return rows_mask(hair, r, BG);
    if (c >= BG + IMG && c < BG + IMG + EXT) return rows_mask(hair, r, BG + IMG - 1);
    return rows_mask(hair, r, c);
}

__global__ __launch_bounds__(TILE* TILE) void uv_render_sample_kernel(const uint8_t* __restrict__ hair_labels,
                                                                     const uint8_t* __restrict__ face_labels,
                                                                     const float* __restrict__ V, const int* __restrict__ F, int B,
                                                                     const char* __restrict__ ws, uint8_t* __restrict__ labels_out,
                                                                     float* __restrict__ uv_out, int tile0) {
    constexpr int NT = TILE * TILE;
    __shared__ float sTri[NT][6];
    __shared__ int sIdx[NT][3];
    __shared__ short sBox[NT][4];              // clipped bounding box of the entry: xmin, xmax, ymin, ymax
    __shared__ int sWave[NT / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = blockIdx.z;
    const int* d = reinterpret_cast<const int*>(ws) + 6 * pair;
    const int nV = d[1], nF = d[3];
    const float* Vp = V + 2 * (size_t)d[0];
    const int* Fp = F + 3 * (size_t)d[2];
    const float* Ux = reinterpret_cast<const float*>(ws + ws_head(B) + (size_t)pair * WS_PAIR + WS_U);
    const float* Uy = Ux + WARP_MAX_V;
    const int x0 = (tile0 + blockIdx.x) * TILE, y0 = (tile0 + blockIdx.y) * TILE;
    const int x = x0 + (tid % TILE), y = y0 + (tid / TILE);
    const float px = (float)x, py = (float)y;

    bool found = false;
    float cu = -1.f, cv = -1.f;                // help_warp.py:17: the image is preset to -1
    for (int base = 0; base < nF; base += NT) {
        // bin: triangle base + tid joins this tile's list when its clipped bounding box (mesh_core.cpp:176-185) meets the tile
        const int t = base + tid;
        bool hit = false;
        float q[6];
        int v[3] = {0, 0, 0};
        int xmin = 0, xmax = -1, ymin = 0, ymax = -1;
        if (t < nF) {
            bool ok = true;
            for (int k = 0; k < 3; ++k) {
                v[k] = Fp[3 * t + k];
                ok = ok && v[k] >= 0 && v[k] < nV;
            }
            if (ok) {
                for (int k = 0; k < 3; ++k) {
                    q[2 * k] = Ux[v[k]];
                    q[2 * k + 1] = Uy[v[k]];
                }
                xmin = max((int)ceilf(fminf(q[0], fminf(q[2], q[4]))), 0);
                xmax = min((int)floorf(fmaxf(q[0], fmaxf(q[2], q[4]))), CANVAS - 1);
                ymin = max((int)ceilf(fminf(q[1], fminf(q[3], q[5]))), 0);
                ymax = min((int)floorf(fmaxf(q[1], fmaxf(q[3], q[5]))), CANVAS - 1);
                hit = xmin <= xmax && ymin <= ymax && xmin < x0 + TILE && xmax >= x0 && ymin < y0 + TILE && ymax >= y0;
            }
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) sWave[wave] = __popcll(m);
        __syncthreads();
        int off = 0, total = 0;
        for (int w = 0; w < NT / 64; ++w) {
            if (w < wave) off += sWave[w];
            total += sWave[w];
        }
        if (hit) {                             // ordered compaction: the list keeps the face order
            const int s = off + __popcll(m & ((1ull << lane) - 1ull));
            for (int k = 0; k < 6; ++k) sTri[s][k] = q[k];
            for (int k = 0; k < 3; ++k) sIdx[s][k] = v[k];
            sBox[s][0] = (short)xmin;
            sBox[s][1] = (short)xmax;
            sBox[s][2] = (short)ymin;
            sBox[s][3] = (short)ymax;
        }
        __syncthreads();
        for (int s = 0; s < total && !found; ++s) {
            // mesh_core.cpp:187-192: only the pixels of the triangle's own clipped box are tested -- a collapsed triangle
            // (den == 0 -> u = v = 0) passes the inside test everywhere and must not paint outside its box
            if (x < sBox[s][0] || x > sBox[s][1] || y < sBox[s][2] || y > sBox[s][3]) continue;
            // mesh_core.cpp:17-43, 45-73 in its operation order (p0, p1, p2 = the triangle's vertices in face order)
            const float p0x = sTri[s][0], p0y = sTri[s][1], p1x = sTri[s][2], p1y = sTri[s][3], p2x = sTri[s][4], p2y = sTri[s][5];
            const float v0x = p2x - p0x, v0y = p2y - p0y, v1x = p1x - p0x, v1y = p1y - p0y, v2x = px - p0x, v2y = py - p0y;
            const float dot00 = v0x * v0x + v0y * v0y, dot01 = v0x * v1x + v0y * v1y, dot02 = v0x * v2x + v0y * v2y;
            const float dot11 = v1x * v1x + v1y * v1y, dot12 = v1x * v2x + v1y * v2y;
            const float den = dot00 * dot11 - dot01 * dot01;
            const float inv = den == 0.f ? 0.f : 1.f / den;
            const float u = (dot11 * dot02 - dot01 * dot12) * inv, vv = (dot00 * dot12 - dot01 * dot02) * inv;
            if (u >= 0.f && vv >= 0.f && u + vv < 1.f) {
                const float w0 = 1.f - u - vv, w1 = vv, w2 = u;
                const int i0 = sIdx[s][0], i1 = sIdx[s][1], i2 = sIdx[s][2];
                // per-vertex colour (V_x / (W - 1), V_y / (H - 1)): my_arap.cpp:130-133
                const float c0x = (float)((double)Vp[2 * i0] / (CANVAS - 1)), c0y = (float)((double)Vp[2 * i0 + 1] / (CANVAS - 1));
                const float c1x = (float)((double)Vp[2 * i1] / (CANVAS - 1)), c1y = (float)((double)Vp[2 * i1 + 1] / (CANVAS - 1));
                const float c2x = (float)((double)Vp[2 * i2] / (CANVAS - 1)), c2y = (float)((double)Vp[2 * i2 + 1] / (CANVAS - 1));
                cu = w0 * c0x + w1 * c1x + w2 * c2x;
                cv = w0 * c0y + w1 * c1y + w2 * c2y;
                found = true;
            }
        }
        if (!__syncthreads_or(!found)) break;  // uniform: the whole tile is covered
    }

    // triangle_wrap_hair.py:77-85 ("fix edge"), assignments in the reference's order; lin = float32(np.linspace(0, 1, 672))
    const float cedge = (float)(1.0 - 1.0 / CANVAS);
    auto lin = [](int i) { return i == CANVAS - 1 ? 1.f : (float)((double)i * (1.0 / (CANVAS - 1))); };
    if (nF == 0) {                             // a descriptor that warp_copy_desc_kernel refused: the identity map (colour = position / 671)
        cu = lin(x);
        cv = lin(y);
    }
    if (y == 0 || y == CANVAS - 1) cu = lin(x);
    if (y == 0) cv = 0.f;
    if (y == CANVAS - 1) cv = cedge;
    if (y == CANVAS - 2) cv = fminf(cv, cedge);
    if (x == 0 || x == CANVAS - 1) cv = lin(y);
    if (x == 0) cu = 0.f;
    if (x == CANVAS - 1) cu = cedge;
    if (x == CANVAS - 2) cu = fminf(cu, cedge);
    if (uv_out) {
        float* o = uv_out + (((size_t)pair * CANVAS + y) * CANVAS + x) * 2;
        o[0] = cu;
        o[1] = cv;
    }
    if (x < BG || x >= BG + IMG || y < BG || y >= BG + IMG) return;    // the crop (mask_adaptor.py:139-140)

    // get_pixelValue.py:34-48 cv2.remap(INTER_LINEAR, constant border 0): coordinates rounded to 1/32 px (cvRound, half to even),
    // tap weights (32 - a)(32 - b) / 1024 ...; the image is 0/1 and the result is truncated to uint8, so the pixel is hair exactly
    // when every tap of non-zero weight is hair.
    const uint8_t* hair = hair_labels + (size_t)pair * IMG * IMG;
    const int sx = __float2int_rn(cu * (float)CANVAS * 32.f), sy = __float2int_rn(cv * (float)CANVAS * 32.f);
    const int ix = sx >> 5, iy = sy >> 5, ax = sx & 31, ay = sy & 31;
    bool warped = padded_mask(hair, iy, ix);
    if (ax) warped = warped && padded_mask(hair, iy, ix + 1);
    if (ay) warped = warped && padded_mask(hair, iy + 1, ix);
    if (ax && ay) warped = warped && padded_mask(hair, iy + 1, ix + 1);
    // naive_transfer (mask_adaptor.py:63-73)
    const size_t o = ((size_t)pair * IMG + (y - BG)) * IMG + (x - BG);
    const uint8_t f = face_labels[o];
    labels_out[o] = warped ? (uint8_t)HAIR : (f == HAIR ? (uint8_t)255 : f);
}

}  // namespace

size_t mask_warp_workspace_bytes(int B) { return B > 0 ? ws_head(B) + (size_t)B * WS_PAIR : 0; }

// the launches behind both entry points, once the descriptors are at the head of the workspace
static hipError_t warp_launch(const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int* F, const int* bidx,
                              const float* bc, const float* U_in, uint8_t* labels_out, float* uv_out, float* U_out, char* w, int B,
                              int outer_iters, int max_cg, float rel_tol, hipStream_t s) {
    if (U_in)
        warp_load_u_kernel<<<dim3(4, B), 256, 0, s>>>(U_in, B, w, U_out);
    else
        arap_solve_kernel<<<B, AT, 0, s>>>(V, F, bidx, bc, B, w, U_out, outer_iters, max_cg, rel_tol);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    // without a UV output only the tiles of the cropped 512 x 512 window are rendered (80 = 5 tiles)
    const int tile0 = uv_out ? 0 : BG / TILE, nt = uv_out ? TILES : IMG / TILE;
    uv_render_sample_kernel<<<dim3(nt, nt, B), TILE * TILE, 0, s>>>(hair_labels, face_labels, V, F, B, w, labels_out, uv_out, tile0);
    return hipGetLastError();
}

hipError_t mask_warp_batch_dev(const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int* F, const int* bidx,
                               const float* bc, const int* desc_dev, const float* U_in, uint8_t* labels_out, float* uv_out, float* U_out,
                               void* ws, int B, int outer_iters, int max_cg, float rel_tol, hipStream_t s) {
    char* w = static_cast<char*>(ws);
    warp_copy_desc_kernel<<<(B + 255) / 256, 256, 0, s>>>(desc_dev, B, reinterpret_cast<int*>(w));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return warp_launch(hair_labels, face_labels, V, F, bidx, bc, U_in, labels_out, uv_out, U_out, w, B, outer_iters, max_cg, rel_tol, s);
}

hipError_t mask_warp_batch(const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int* F, const int* bidx,
                           const float* bc, const int* desc_host, const float* U_in, uint8_t* labels_out, float* uv_out, float* U_out,
                           void* ws, int B, int outer_iters, int max_cg, float rel_tol, hipStream_t s) {
    char* w = static_cast<char*>(ws);
    for (int p0 = 0; p0 < B; p0 += WARP_DESC_PAIRS) {
        WarpDesc desc;
        desc.n = B - p0 < WARP_DESC_PAIRS ? B - p0 : WARP_DESC_PAIRS;
        desc.pair0 = p0;
        for (int i = 0; i < WARP_DESC_PAIRS; ++i)
            for (int k = 0; k < 6; ++k) desc.d[i][k] = i < desc.n ? desc_host[6 * (p0 + i) + k] : 0;
        warp_store_desc_kernel<<<1, WARP_DESC_PAIRS * 6, 0, s>>>(desc, reinterpret_cast<int*>(w));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return warp_launch(hair_labels, face_labels, V, F, bidx, bc, U_in, labels_out, uv_out, U_out, w, B, outer_iters, max_cg, rel_tol, s);
}

}  // namespace chk
