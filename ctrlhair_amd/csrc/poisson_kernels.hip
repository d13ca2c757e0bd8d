// poisson_kernels.hip -- the blending step that follows the generator (hair_editor.py:285-310, poisson_blending.py:29-87)
// on the GPU: the reference assembles a (HW)^2 sparse matrix with a Python double loop and calls a sparse direct solver
// three times (seconds per image); here the same linear system is solved matrix-free by conjugate gradients.
//
// System (per colour channel, gamma space v = u8^(1/2.2)):  unknowns U = {mask != 0} + {border pixels} (the reference leaves
// border pixels outside the mask as Laplacian rows with the target value as right-hand side, poisson_blending.py:48-56);
// known K = interior pixels with mask == 0, x = target.  For k in U:
//      4 x_k - sum_{n in N4(k), in image, n in U} x_n  =  base_k + sum_{n in N4(k), n in K} target_n
//      base_k = (L source)_k  if mask_k != 0  else target_k,      (L s)_k = 4 s_k - sum_{n in N4(k), in image} s_n
// Symmetric positive definite -> CG; all vectors in f64 (condition number ~ (2N/pi)^2 ~ 1e5 at 512 px: an f32 CG stalls at
// ~1e-2 relative error, more than one uint8 level after the gamma power).  L2-resident streaming kernels, 2 launches per iteration
// (Chronopoulos-Gear CG), scalars (alpha, beta, convergence) stay on the device.  Dot products are two-level and
// deterministic: per-block partial sums, re-reduced in a fixed order by every block that needs the scalar (no atomics).
//
// Batched: every kernel runs on a grid of (blocks per image, B).  blockIdx.y selects the image; each image has its own
// vectors, partials and PoissonCG state and keeps the block partition of a single-image solve, so image i of a batch is
// bit-identical to the same image solved alone (iteration count included) and the single-image call is the B = 1 case.
// At 256 px the solve is bound by its two launches per iteration, not by bandwidth: a batch shares them.
#include <hip/hip_runtime.h>

#include <climits>
#include <stdint.h>
#include <vector>

#include "kernels.h"
#include "wave_ops.h"

namespace chk {

// sum of v over the 256-thread block, returned to every thread (fixed order -> run-to-run deterministic)
__device__ __forceinline__ double pb_block_sum(double v, double* sh) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// total of the per-block partials part[0 .. n) (every block computes the same value in the same order)
__device__ __forceinline__ double pb_total(const double* __restrict__ part, int n, double* sh) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) v += part[i];
    return pb_block_sum(v, sh);
}

__device__ __forceinline__ bool pb_unknown(const uint8_t* m, int y, int x, int H, int W) {
    return m[y * W + x] != 0 || y == 0 || x == 0 || y == H - 1 || x == W - 1;
}

constexpr int PB_MAXBLK = 512;      // CG kernels: grid-stride over at most this many blocks per image

struct PoissonCG {
    double gamma[2][3], alpha[2][3], gamma0[3];
    int done, iters;
};

// Workspace of a batch: PoissonCG[B] (contiguous, so the host reads every flag with one copy; B slots of PB_CG_SLOT bytes are
// reserved), then per image `stride` bytes holding X, R, P, S, W (3 HW doubles each), partG, partD (3 PB_MAXBLK doubles each)
// and the unknown map U (HW bytes).
constexpr size_t PB_CG_SLOT = 256;
static_assert(sizeof(PoissonCG) <= PB_CG_SLOT, "PoissonCG outgrew its slot");

struct PoissonVec {
    double *X, *R, *P, *S, *Wv, *partG, *partD;
    uint8_t* U;
};

__host__ __device__ inline size_t pb_vec_stride(size_t HW) {
    const size_t n = 5 * 3 * HW * sizeof(double) + 2 * 3 * PB_MAXBLK * sizeof(double) + HW;
    return (n + 255) / 256 * 256;
}

__device__ __forceinline__ PoissonVec pb_vectors(char* vecs, int img, int HW) {
    PoissonVec v;
    v.X = reinterpret_cast<double*>(vecs + (size_t)img * pb_vec_stride((size_t)HW));
    v.R = v.X + 3 * (size_t)HW;
    v.P = v.R + 3 * (size_t)HW;
    v.S = v.P + 3 * (size_t)HW;
    v.Wv = v.S + 3 * (size_t)HW;
    v.partG = v.Wv + 3 * (size_t)HW;
    v.partD = v.partG + 3 * (size_t)PB_MAXBLK;
    v.U = reinterpret_cast<uint8_t*>(v.partD + 3 * (size_t)PB_MAXBLK);
    return v;
}

// The kernels below are thin: they pick the image of blockIdx.y and call a per-image body whose pointer PARAMETERS carry
// __restrict__ (the qualifier is only honoured on parameters; without it the update kernel's loads of one channel wait for
// the stores of the previous one: +5 % per solve, measured).

// gamma transform, right-hand side, initial guess x0 = target, r0 = b - A x0, p = s = 0
__device__ __forceinline__ void pb_setup_image(const uint8_t* __restrict__ src, const uint8_t* __restrict__ tgt,
                                               const uint8_t* __restrict__ mask, double* __restrict__ X, double* __restrict__ R,
                                               double* __restrict__ P, double* __restrict__ S, uint8_t* __restrict__ U, int H, int W,
                                               float inv_gamma) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const int HW = H * W;
    if (k < HW) {
        const int y = k / W, x = k % W;
        const bool unk = pb_unknown(mask, y, x, H, W);
        U[k] = unk ? 1 : 0;
        const int ny[4] = {y, y, y + 1, y - 1}, nx[4] = {x + 1, x - 1, x, x};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double t = pow((double)tgt[k * 3 + c], (double)inv_gamma);
            X[c * HW + k] = t;
            double r = 0.0;
            if (unk) {
                // b_k
                double b;
                if (mask[k] != 0) {
                    b = 4.0 * pow((double)src[k * 3 + c], (double)inv_gamma);
                    for (int q = 0; q < 4; ++q)
                        if ((unsigned)ny[q] < (unsigned)H && (unsigned)nx[q] < (unsigned)W)
                            b -= pow((double)src[(ny[q] * W + nx[q]) * 3 + c], (double)inv_gamma);
                } else {
                    b = t;
                }
                // r0 = b + sum_{known nbrs} t_n - (4 t_k - sum_{unknown nbrs} t_n) = b - 4 t_k + sum_{all in-image nbrs} t_n
                r = b - 4.0 * t;
                for (int q = 0; q < 4; ++q)
                    if ((unsigned)ny[q] < (unsigned)H && (unsigned)nx[q] < (unsigned)W)
                        r += pow((double)tgt[(ny[q] * W + nx[q]) * 3 + c], (double)inv_gamma);
            }
            R[c * HW + k] = r;
            P[c * HW + k] = 0.0;
            S[c * HW + k] = 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void pb_setup_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ tgt,
                                                       const uint8_t* __restrict__ mask, char* __restrict__ vecs, int H, int W,
                                                       float inv_gamma) {
    const size_t HW = (size_t)H * W;
    const PoissonVec pv = pb_vectors(vecs, blockIdx.y, H * W);
    pb_setup_image(src + blockIdx.y * HW * 3, tgt + blockIdx.y * HW * 3, mask + blockIdx.y * HW, pv.X, pv.R, pv.P, pv.S, pv.U, H, W,
                   inv_gamma);
}

// ---- CG in the Chronopoulos-Gear form: one matvec and ONE fused pair of dot products per iteration, hence two kernel
// launches per iteration (the solver is launch-bound: the vectors of a 512x512 image live in L2):
//      w = A r,  gamma = r.r,  delta = r.w                                        (pb_matvec_kernel)
//      beta = gamma / gamma_prev,  alpha = gamma / (delta - beta gamma / alpha_prev)   [beta = 0, alpha = gamma/delta at i = 0]
//      p = r + beta p;  s = w + beta s;  x += alpha p;  r -= alpha s              (pb_update_kernel)
// Every block re-reduces the per-block partials in the same order, so all blocks agree bit for bit on the scalars and on
// convergence (no flag race); the previous iteration's scalars sit in a ping-pong slot written by block 0.
// Ragged convergence: every image stops on its own criterion; the blocks of a finished image return at the top of both kernels.
__global__ void pb_init_cg_kernel(PoissonCG* cgs) {
    PoissonCG* cg = cgs + blockIdx.x;
    for (int q = 0; q < 2; ++q)
        for (int c = 0; c < 3; ++c) cg->gamma[q][c] = cg->alpha[q][c] = 0.0;
    for (int c = 0; c < 3; ++c) cg->gamma0[c] = 0.0;
    cg->done = 0;
    cg->iters = 0;
}

// w = A r on the unknowns; partG[c][block] = partial r.r, partD[c][block] = partial r.w
__device__ __forceinline__ void pb_matvec_image(const double* __restrict__ R, double* __restrict__ Wv,
                                                const uint8_t* __restrict__ U, const PoissonCG* cg,
                                                double* __restrict__ partG, double* __restrict__ partD, int H, int W, double* sh) {
    if (cg->done) return;
    const int HW = H * W;
    double g[3] = {0.0, 0.0, 0.0}, d[3] = {0.0, 0.0, 0.0};
    // grid-stride: at most PB_MAXBLK blocks, so that the per-block partials every block re-reduces stay a few KiB
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < HW; k += gridDim.x * blockDim.x) {
        if (!U[k]) continue;
        const int y = k / W, x = k % W;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double* r = R + c * HW;
            double v = 4.0 * r[k];
            if (x + 1 < W && U[k + 1]) v -= r[k + 1];
            if (x > 0 && U[k - 1]) v -= r[k - 1];
            if (y + 1 < H && U[k + W]) v -= r[k + W];
            if (y > 0 && U[k - W]) v -= r[k - W];
            Wv[c * HW + k] = v;
            g[c] += r[k] * r[k];
            d[c] += r[k] * v;
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double tg = pb_block_sum(g[c], sh), td = pb_block_sum(d[c], sh);
        if (threadIdx.x == 0) {
            partG[c * gridDim.x + blockIdx.x] = tg;
            partD[c * gridDim.x + blockIdx.x] = td;
        }
    }
}

__global__ __launch_bounds__(256) void pb_matvec_kernel(char* __restrict__ vecs, const PoissonCG* cgs, int H, int W) {
    __shared__ double sh[4];
    const PoissonVec pv = pb_vectors(vecs, blockIdx.y, H * W);
    pb_matvec_image(pv.R, pv.Wv, pv.U, cgs + blockIdx.y, pv.partG, pv.partD, H, W, sh);
}

__device__ __forceinline__ void pb_update_image(double* __restrict__ X, double* __restrict__ R, double* __restrict__ P,
                                                double* __restrict__ S, const double* __restrict__ Wv,
                                                const uint8_t* __restrict__ U, PoissonCG* cg, const double* __restrict__ partG,
                                                const double* __restrict__ partD, int HW, int iter, double rel_tol2, double* sh) {
    if (cg->done) return;
    const int q = iter & 1;
    double alpha[3], beta[3], gam[3];
    bool live[3], any = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        gam[c] = pb_total(partG + c * gridDim.x, gridDim.x, sh);
        const double del = pb_total(partD + c * gridDim.x, gridDim.x, sh);
        const double g0 = iter == 0 ? gam[c] : cg->gamma0[c];
        live[c] = gam[c] > rel_tol2 * g0 && gam[c] > 1e-24;      // channel not yet converged
        if (iter == 0) {
            beta[c] = 0.0;
            alpha[c] = del > 0.0 ? gam[c] / del : 0.0;
        } else {
            const double gp = cg->gamma[q ^ 1][c], ap = cg->alpha[q ^ 1][c];
            beta[c] = gp > 0.0 ? gam[c] / gp : 0.0;
            const double den = del - (ap != 0.0 ? beta[c] * gam[c] / ap : 0.0);
            alpha[c] = den > 0.0 ? gam[c] / den : 0.0;
        }
        if (!live[c]) alpha[c] = beta[c] = 0.0;
        any = any || live[c];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {                     // bookkeeping for the next iteration / the host
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            cg->gamma[q][c] = live[c] ? gam[c] : cg->gamma[q ^ 1][c];
            cg->alpha[q][c] = live[c] ? alpha[c] : cg->alpha[q ^ 1][c];
            if (iter == 0) cg->gamma0[c] = gam[c];
        }
        if (any) cg->iters = iter + 1;
        else cg->done = 1;
    }
    if (!any) return;                                              // same decision in every block
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < HW; k += gridDim.x * blockDim.x) {
        if (!U[k]) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (!live[c]) continue;                                // a converged channel keeps its solution
            const int i = c * HW + k;
            const double p = R[i] + beta[c] * P[i];
            const double s = Wv[i] + beta[c] * S[i];
            P[i] = p;
            S[i] = s;
            X[i] += alpha[c] * p;
            R[i] -= alpha[c] * s;
        }
    }
}

__global__ __launch_bounds__(256) void pb_update_kernel(char* __restrict__ vecs, PoissonCG* cgs, int HW, int iter,
                                                        double rel_tol2) {
    __shared__ double sh[4];
    const PoissonVec pv = pb_vectors(vecs, blockIdx.y, HW);
    pb_update_image(pv.X, pv.R, pv.P, pv.S, pv.Wv, pv.U, cgs + blockIdx.y, pv.partG, pv.partD, HW, iter, rel_tol2, sh);
}

// Residual check after the LAST allowed update (the update kernel only learns at the top of the following iteration that the
// previous one met the tolerance): sums the partials of a final mat-vec and sets the flag.  One block per image.  nparts =
// blocks per image of that mat-vec.  With no iteration done (max_iters = 0) there is no ||r0|| on file: only an exactly solved
// system counts.  An image that is already done ran no final mat-vec (its partials are those of its last iteration): skipped.
__global__ __launch_bounds__(256) void pb_final_check_kernel(char* __restrict__ vecs, PoissonCG* __restrict__ cgs, int HW, int nparts,
                                                             double rel_tol2) {
    PoissonCG* __restrict__ cg = cgs + blockIdx.y;
    if (cg->done) return;
    const double* __restrict__ partG = pb_vectors(vecs, blockIdx.y, HW).partG;
    __shared__ double sh[4];
    bool any = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double gam = pb_total(partG + c * nparts, nparts, sh);
        const double g0 = cg->gamma0[c];
        any = any || (gam > rel_tol2 * g0 && gam > 1e-24);
    }
    if (threadIdx.x == 0 && !any) cg->done = 1;
}

// out = clamp(x^gamma) truncated to uint8 (poisson_blending.py:81-86); NaN (negative base) -> 0
__global__ void pb_finish_kernel(char* __restrict__ vecs, uint8_t* __restrict__ out_b, int HW, float gamma) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= HW) return;
    const double* __restrict__ X = pb_vectors(vecs, blockIdx.y, HW).X;
    uint8_t* __restrict__ out = out_b + (size_t)blockIdx.y * HW * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double x = X[c * HW + k];
        double v = x < 0.0 ? 0.0 : pow(x, (double)gamma);
        v = v > 255.0 ? 255.0 : v;
        out[k * 3 + c] = (uint8_t)v;
    }
}

size_t poisson_workspace_bytes(int H, int W) { return PB_CG_SLOT + pb_vec_stride((size_t)H * W); }

hipError_t poisson_blend_batch(const uint8_t* src, const uint8_t* tgt, const uint8_t* mask, uint8_t* out, int B, int H, int W,
                               int with_gamma, int max_iters, double rel_tol, void* ws, int* iters_out, hipStream_t s) {
    const int HW = H * W;
    PoissonCG* cgs = static_cast<PoissonCG*>(ws);
    char* vecs = static_cast<char*>(ws) + (size_t)B * PB_CG_SLOT;
    const int nb = (HW + 255) / 256, ncg = nb < PB_MAXBLK ? nb : PB_MAXBLK;
    const float gamma = with_gamma ? 2.2f : 1.0f;
    const dim3 g(nb, B), gc(ncg, B), b(256);
    std::vector<PoissonCG> host(B);
    auto poll = [&]() -> hipError_t {      // every image's state in ONE copy
        hipError_t e = hipMemcpyAsync(host.data(), cgs, (size_t)B * sizeof(PoissonCG), hipMemcpyDeviceToHost, s);
        return e != hipSuccess ? e : hipStreamSynchronize(s);
    };
    hipLaunchKernelGGL(pb_init_cg_kernel, dim3(B), dim3(1), 0, s, cgs);
    hipLaunchKernelGGL(pb_setup_kernel, g, b, 0, s, src, tgt, mask, vecs, H, W, 1.0f / gamma);
    bool done = false;
    for (int it = 0; it < max_iters && !done; ++it) {
        hipLaunchKernelGGL(pb_matvec_kernel, gc, b, 0, s, vecs, cgs, H, W);
        hipLaunchKernelGGL(pb_update_kernel, gc, b, 0, s, vecs, cgs, HW, it, rel_tol * rel_tol);
        if ((it & 63) == 63) {        // poll the device flags every 64 iterations (launching stops once every image is done)
            const hipError_t e = poll();
            if (e != hipSuccess) return e;
            done = true;
            for (int i = 0; i < B; ++i) done = done && host[i].done != 0;
        }
    }
    if (!done) {           // did the last allowed update reach the tolerance?  (mat-vec + reduction only, no update)
        hipLaunchKernelGGL(pb_matvec_kernel, gc, b, 0, s, vecs, cgs, H, W);
        hipLaunchKernelGGL(pb_final_check_kernel, dim3(1, B), b, 0, s, vecs, cgs, HW, ncg, rel_tol * rel_tol);
    }
    hipLaunchKernelGGL(pb_finish_kernel, g, b, 0, s, vecs, out, HW, gamma);
    if (iters_out) {       // iteration counts; negated (INT_MIN for zero iterations) when rel_tol was not reached
        const hipError_t e = poll();
        if (e != hipSuccess) return e;
        for (int i = 0; i < B; ++i) iters_out[i] = host[i].done ? host[i].iters : (host[i].iters > 0 ? -host[i].iters : INT_MIN);
    }
    return hipGetLastError();
}

// ---- blending mask (hair_editor.py:297-305) ------------------------------------------------------------------------
// res = dilate13(hair) outside the target's background, dilate5(hair) on it; hair = (target == 13) | (face == 13).
// Structuring elements: OpenCV MORPH_ELLIPSE rows, half-widths per |dy| passed in constant tables.
__constant__ int c_hw13[13] = {0, 3, 4, 5, 6, 6, 6, 6, 6, 5, 4, 3, 0};
__constant__ int c_hw5[5] = {0, 2, 2, 2, 0};

__global__ void blend_mask_kernel(const uint8_t* __restrict__ tp_b, const uint8_t* __restrict__ fp_b, uint8_t* __restrict__ out_b,
                                  int H, int W) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= H * W) return;
    const size_t img = (size_t)blockIdx.y * H * W;
    const uint8_t* __restrict__ tp = tp_b + img;
    const uint8_t* __restrict__ fp = fp_b + img;
    uint8_t* __restrict__ out = out_b + img;
    const int y = k / W, x = k % W;
    const bool bg = tp[k] == 0;
    const int r = bg ? 2 : 6;
    uint8_t v = 0;
    for (int dy = -r; dy <= r && !v; ++dy) {
        const int yy = y + dy;
        if ((unsigned)yy >= (unsigned)H) continue;
        const int hw = bg ? c_hw5[dy + 2] : c_hw13[dy + 6];
        for (int dx = -hw; dx <= hw; ++dx) {
            const int xx = x + dx;
            if ((unsigned)xx >= (unsigned)W) continue;
            const int q = yy * W + xx;
            if (tp[q] == 13 || fp[q] == 13) { v = 1; break; }
        }
    }
    out[k] = v;
}

hipError_t blend_mask_batch(const uint8_t* target_parsing, const uint8_t* face_parsing, uint8_t* out, int B, int H, int W,
                            hipStream_t s) {
    hipLaunchKernelGGL(blend_mask_kernel, dim3((H * W + 255) / 256, B), dim3(256), 0, s, target_parsing, face_parsing, out, H, W);
    return hipGetLastError();
}

}  // namespace chk
