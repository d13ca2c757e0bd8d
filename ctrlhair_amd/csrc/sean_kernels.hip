// sean_kernels.hip -- the small HBM/LDS-bound kernels around the MFMA convs of the SEAN generator path.
// gfx950 only (wave64).  Every kernel is predicated for arbitrary shapes.
#include "kernels.h"
#include "sh16.h"
#include "launch.h"

namespace chk {

// ---------------------------------------------------------------------------------------------------------
// ace_finish_f32 (kernels.h): one thread = one pixel x AF_CG channels; block = 256 consecutive pixels of a sample.
constexpr int AF_CG = 8;
__global__ __launch_bounds__(256) void ace_finish_f32_kernel(const float* __restrict__ gb, int rowsP, const float* __restrict__ x, int x_up,
                                                             const float* __restrict__ bias_g, const float* __restrict__ bias_b,
                                                             const float* __restrict__ bn_a, const float* __restrict__ bn_d,
                                                             const float* __restrict__ nv, const float* __restrict__ noise, long long noise_bstride,
                                                             const uint8_t* __restrict__ lab, const float* __restrict__ lut, float* __restrict__ out,
                                                             int B, int C, int H, int W, int act) {
    const int HW = H * W, ppb = (HW + 255) / 256;
    const int b = blockIdx.x / ppb, pix = (blockIdx.x - b * ppb) * 256 + threadIdx.x;
    if (pix >= HW) return;
    const int y = pix / W, xx = pix - y * W;
    const int c0 = blockIdx.y * AF_CG;
    const int xW = W >> x_up, xHW = xW * (H >> x_up);
    const float nz = noise[(long long)b * noise_bstride + (long long)xx * H + y];          // plane layout [W][H]
    const float* xp = x + ((long long)b * C + c0) * xHW + (y >> x_up) * xW + (xx >> x_up);
    const float* gp = gb + (long long)b * rowsP * HW + pix;
    float* op = out + ((long long)b * C + c0) * HW + pix;
    unsigned lo[9];
    unsigned lmask = 0;                   // bit t: the tap carries a style term (inside the image, label < 19)
    const float* Lb = lut ? lut + (long long)b * 19 * 9 * 2 * C : nullptr;
    if (Lb) {
        const uint8_t* lb = lab + (long long)b * HW;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, x2 = xx + t % 3 - 1;
            const bool in = (unsigned)yy < (unsigned)H && (unsigned)x2 < (unsigned)W;
            const unsigned jv = lb[in ? yy * W + x2 : 0];
            const bool on = in && jv < 19u;
            lmask |= on ? 1u << t : 0u;
            lo[t] = ((on ? jv : 0u) * 9u + (unsigned)t) * 2u * (unsigned)C;
        }
    }
#pragma unroll
    for (int i = 0; i < AF_CG; ++i) {
        const int c = c0 + i;
        if (c >= C) break;
        const int rg = (c >> 5) * 64 + (c & 31);           // gamma row of channel c in the packed image's order; beta: + 32
        float sg = 0.f, sb = 0.f;
        if (Lb) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float w = ((lmask >> t) & 1u) ? 1.f : 0.f;
                sg += w * Lb[lo[t] + c];
                sb += w * Lb[lo[t] + C + c];
            }
        }
        const float gam = gp[(long long)rg * HW] + (bias_g[c] + sg);
        const float bet = gp[(long long)(rg + 32) * HW] + (bias_b[c] + sb);
        const float nrm = bn_a[c] * xp[(long long)i * xHW] + nv[c] * nz + bn_d[c];
        float o = nrm * (1.f + gam) + bet;
        if (act == 1) o = fmaxf(o, 0.2f * o);              // ACT_LRELU
        else if (act == 2) o = fmaxf(o, 0.f);              // ACT_RELU
        op[(long long)i * HW] = o;
    }
}
hipError_t ace_finish_f32(const float* gb, int rowsP, const float* x, int x_up, const float* bias_g, const float* bias_b, const float* bn_a,
                          const float* bn_d, const float* nv, const float* noise, long long noise_bstride, const uint8_t* lab, const float* lut,
                          float* out, int B, int C, int H, int W, int act, hipStream_t s) {
    if (act < 0 || act > 2) return hipErrorInvalidValue;
    const int ppb = (H * W + 255) / 256;
    hipLaunchKernelGGL(ace_finish_f32_kernel, dim3((unsigned)(B * ppb), (unsigned)((C + AF_CG - 1) / AF_CG)), dim3(256), 0, s, gb, rowsP, x, x_up, bias_g, bias_b,
                       bn_a, bn_d, nv, noise, noise_bstride, lab, lut, out, B, C, H, W, act);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// F.interpolate(seg, size, mode='nearest') on the label map (generator.py:75, normalization.py:115):
// src = floor(dst * in/out); in/out is an integer here (S / r).
__global__ void label_down_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int B, int S, int r, const int* __restrict__ memo_hit) {
    if (memo_hit && *memo_hit) return;      // (label memo: the map of the previous call stands)
    const long long n = (long long)B * r * r;
    const int f = S / r;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % r), y = (int)((i / r) % r);
        const long long b = i / ((long long)r * r);
        out[i] = in[(b * S + (long long)y * f) * S + (long long)x * f];
    }
}

hipError_t label_downsample(const uint8_t* in, uint8_t* out, int B, int S, int r, hipStream_t s, const int* memo_hit) {
    const long long n = (long long)B * r * r;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(label_down_kernel, dim3(grid), dim3(256), 0, s, in, out, B, S, r, memo_hit);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Label memo (sean_model.h SeanModel::memo_state): does this chunk bring the label maps of the previous one?  The compare kernel reads the
// incoming maps and the handle's copy in 16-byte words; a word that differs is written into the copy and marks `diff`.  The one-thread
// decision kernel then sets hit = valid && !diff && (the key of this enqueue == the stored key), re-arms the state and counts.  Every
// memoized kernel reads `hit` once, at its top.  Nothing here depends on a value the host learns per call: the same sequence replays in a graph.
__global__ __launch_bounds__(256) void label_memo_compare_kernel(const uint4* __restrict__ in, uint4* __restrict__ copy, long long n16, int* __restrict__ state) {
    bool d = false;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) {
        const uint4 a = in[i], c = copy[i];
        if (a.x != c.x || a.y != c.y || a.z != c.z || a.w != c.w) {
            copy[i] = a;
            d = true;
        }
    }
    if (__any(d) && (threadIdx.x & 63) == 0) atomicOr(state + MEMO_DIFF, 1);
}
__global__ void label_memo_decide_kernel(int* __restrict__ state, int B, int S, int epoch, int spade) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int hit = (state[MEMO_VALID] == 1 && state[MEMO_DIFF] == 0 && state[MEMO_KEY] == B && state[MEMO_KEY + 1] == S && state[MEMO_KEY + 2] == epoch) ? 1 : 0;
    state[MEMO_HIT] = hit;
    state[MEMO_VALID] = 1;
    state[MEMO_DIFF] = 0;
    state[MEMO_KEY] = B;
    state[MEMO_KEY + 1] = S;
    state[MEMO_KEY + 2] = epoch;
    state[MEMO_CALLS] += 1;
    state[MEMO_HITS] += hit;
    // SPADE memo (kernels.h): the accumulators are stored on the second sight of a label set, so a run of changing maps never pays for stores
    const int mode = (spade && hit) ? (state[MEMO_ACC_VALID] == 1 ? SPADE_LOAD : SPADE_STORE) : SPADE_PLAIN;
    state[MEMO_SPADE_MODE] = mode;
    state[MEMO_ACC_VALID] = mode != SPADE_PLAIN ? 1 : 0;
    state[MEMO_STORES] += mode == SPADE_STORE;
    state[MEMO_LOADS] += mode == SPADE_LOAD;
}
__global__ void label_memo_invalidate_kernel(int* __restrict__ state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[MEMO_VALID] = state[MEMO_HIT] = state[MEMO_ACC_VALID] = state[MEMO_SPADE_MODE] = 0;
}
hipError_t label_memo_begin(const uint8_t* labels, uint8_t* copy, long long bytes, int* state, int B, int S, int epoch, hipStream_t s, int spade) {
    if (!labels || !copy || !state || bytes <= 0 || (bytes & 15) || (reinterpret_cast<uintptr_t>(labels) & 15) || (reinterpret_cast<uintptr_t>(copy) & 15))
        return hipErrorInvalidValue;
    const long long n16 = bytes >> 4;
    const int grid = (int)((n16 + 255) / 256 < 2048 ? (n16 + 255) / 256 : 2048);
    hipLaunchKernelGGL(label_memo_compare_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint4*>(labels), reinterpret_cast<uint4*>(copy), n16, state);
    hipLaunchKernelGGL(label_memo_decide_kernel, dim3(1), dim3(64), 0, s, state, B, S, epoch, spade);
    return hipGetLastError();
}
hipError_t label_memo_invalidate(int* state, hipStream_t s) {
    if (!state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(label_memo_invalidate_kernel, dim3(1), dim3(64), 0, s, state);
    return hipGetLastError();
}

// Code memo (sean_model.h SeanModel::code_state): does this chunk bring the style codes of the previous one?  The compare kernel above reads
// the codes as integer words (equal bits are a hit whatever they encode: NaN payloads, -0.0) and marks CODE_DIFF, which sits where MEMO_DIFF
// does; the decision is the label memo's without the SPADE mode, keyed on (B, epoch).
static_assert((int)CODE_DIFF == (int)MEMO_DIFF, "label_memo_compare_kernel marks word MEMO_DIFF of the state it is given");
__global__ void code_memo_decide_kernel(int* __restrict__ state, int B, int epoch) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int hit = (state[CODE_VALID] == 1 && state[CODE_DIFF] == 0 && state[CODE_KEY] == B && state[CODE_KEY + 1] == epoch) ? 1 : 0;
    state[CODE_HIT] = hit;
    state[CODE_VALID] = 1;
    state[CODE_DIFF] = 0;
    state[CODE_KEY] = B;
    state[CODE_KEY + 1] = epoch;
    state[CODE_CALLS] += 1;
    state[CODE_HITS] += hit;
}
__global__ void code_memo_invalidate_kernel(int* __restrict__ state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[CODE_VALID] = state[CODE_HIT] = 0;
}
hipError_t code_memo_begin(const float* codes, float* copy, long long bytes, int* state, int B, int epoch, hipStream_t s) {
    if (!codes || !copy || !state || bytes <= 0 || (bytes & 15) || (reinterpret_cast<uintptr_t>(codes) & 15) || (reinterpret_cast<uintptr_t>(copy) & 15))
        return hipErrorInvalidValue;
    const long long n16 = bytes >> 4;
    const int grid = (int)((n16 + 255) / 256 < 2048 ? (n16 + 255) / 256 : 2048);
    hipLaunchKernelGGL(label_memo_compare_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint4*>(codes), reinterpret_cast<uint4*>(copy), n16, state);
    hipLaunchKernelGGL(code_memo_decide_kernel, dim3(1), dim3(64), 0, s, state, B, epoch);
    return hipGetLastError();
}
hipError_t code_memo_invalidate(int* state, hipStream_t s) {
    if (!state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(code_memo_invalidate_kernel, dim3(1), dim3(64), 0, s, state);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// 3x3 conv on a one-hot map == 9-tap table gather (exact):  out[b,k,p] = act(bias[k] + sum_t T[label(p+t)][t][k])
// Used for SPADE.mlp_shared (normalization.py:239-242,253) and the generator's `fc` conv (generator.py:33,76).
// Table layout T[(j*9+t)*K + k].  One block = 256 consecutive pixels x KC channels; the table slice for the KC
// channels sits in LDS.
constexpr int OH_KC = 32;

__global__ __launch_bounds__(256) void onehot_conv3x3_kernel(const uint8_t* __restrict__ lab,
                                                             const float* __restrict__ table,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             int B, int H, int W, int K, int relu, int c4,
                                                             const uint8_t* __restrict__ need, int kout) {
    // Table slice in LDS with a padded row pitch (36 floats: lanes that hold different labels start 4 banks apart) and one
    // all-zero row that taps outside the image (and labels >= 19) point at: every lane issues the same 9 ds_read_b128 per 4
    // channels, no predication (as 288 ds_read_b32 per pixel the kernel was bound by its LDS reads, not by its stores).
    constexpr int RS = OH_KC + 4, ZROW = 19 * 9;
    __shared__ __attribute__((aligned(16))) float T[(ZROW + 1) * RS];
    __shared__ __attribute__((aligned(16))) float bs[OH_KC];
    const int k0 = blockIdx.y * OH_KC;
    bool wanted = true;
    if (need) {       // exact SPADE-interior reduction: only pixels next to a boundary pixel are ever read (ace_sparse.h)
        const long long pq = blockIdx.x * 256LL + threadIdx.x;
        wanted = pq < (long long)B * H * W && need[pq];
        // aligned groups of 8 pixels (32-byte sectors of the NCHW planes) are written whole or not at all
        const unsigned long long wm = __ballot(wanted);
        wanted = pq < (long long)B * H * W && ((wm >> ((threadIdx.x & 63) & ~7)) & 0xFFull) != 0ull;
        if (__syncthreads_or(wanted) == 0) return;
    }
    for (int i = threadIdx.x; i < (ZROW + 1) * OH_KC; i += 256) {
        const int jt = i / OH_KC, kk = i % OH_KC;
        T[jt * RS + kk] = (jt < ZROW && k0 + kk < K) ? table[(long long)jt * K + k0 + kk] : 0.f;
    }
    if (threadIdx.x < OH_KC) bs[threadIdx.x] = (k0 + threadIdx.x < K) ? bias[k0 + threadIdx.x] : 0.f;
    __syncthreads();
    const long long HW = (long long)H * W;
    const long long pix = blockIdx.x * 256LL + threadIdx.x;
    if (pix >= B * HW || !wanted) return;
    const int b = (int)(pix / HW);
    const int y = (int)((pix % HW) / W), x = (int)(pix % W);
    int jt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        const int j = lab[b * HW + (in ? (long long)yy * W + xx : 0)];
        jt[t] = (in && j < 19 ? j * 9 + t : ZROW) * RS;        // labels >= 19 ("no class", e.g. 255): all-zero one-hot
    }
    const long long p = pix % HW;
#pragma unroll
    for (int gq = 0; gq < OH_KC / 4; ++gq) {
        const int k = k0 + gq * 4;
        if (k >= K) break;
        float4 a = *reinterpret_cast<const float4*>(bs + gq * 4);
#pragma unroll
        for (int t = 0; t < 9; ++t) {                          // bias first, then the taps in order (+0.f outside the image)
            const float4 r = *reinterpret_cast<const float4*>(T + jt[t] + gq * 4);
            a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w;
        }
        if (relu) {
            a.x = a.x > 0.f ? a.x : 0.f; a.y = a.y > 0.f ? a.y : 0.f;
            a.z = a.z > 0.f ? a.z : 0.f; a.w = a.w > 0.f ? a.w : 0.f;
        }
        if (c4 && k + 3 < K) {                                 // [B][K/4][HW][4]
            *reinterpret_cast<float4*>(out + (((long long)b * (K >> 2) + (k >> 2)) * HW + p) * 4) = a;
        } else {
            const float v[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (k + e >= K) break;
                if (c4) out[(((long long)b * (K >> 2) + ((k + e) >> 2)) * HW + p) * 4 + ((k + e) & 3)] = v[e];
                else out[((long long)b * kout + k + e) * HW + p] = v[e];
            }
        }
    }
}

hipError_t onehot_conv3x3(const uint8_t* lab, const float* table, const float* bias, float* out, int B, int H, int W,
                          int K, int relu, hipStream_t s, int c4, const uint8_t* need, int kout) {
    const long long npix = (long long)B * H * W;
    if (kout && (kout < K || c4)) return hipErrorInvalidValue;
    dim3 grid((unsigned)((npix + 255) / 256), (unsigned)((K + OH_KC - 1) / OH_KC));
    hipLaunchKernelGGL(onehot_conv3x3_kernel, grid, dim3(256), 0, s, lab, table, bias, out, B, H, W, K, relu, c4, need, kout ? kout : K);
    return hipGetLastError();
}

// planes k0 .. k0 + 19 of an NCHW tensor with kout planes per sample: the one-hot label map (labels >= 19: all zero) + a zero plane
__global__ __launch_bounds__(256) void label_onehot_planes_kernel(const uint8_t* __restrict__ lab, float* __restrict__ out, long long HW,
                                                                  long long npix, int kout, int k0) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= npix) return;
    const long long b = i / HW, p = i - b * HW;
    const int j = lab[i];
    float* o = out + (b * kout + k0) * HW + p;
#pragma unroll
    for (int q = 0; q < 20; ++q) o[q * HW] = q == j ? 1.f : 0.f;
}
hipError_t label_onehot_planes(const uint8_t* lab, float* out, int B, int H, int W, int kout, int k0, hipStream_t s) {
    const long long HW = (long long)H * W, npix = B * HW;
    if (k0 + 20 > kout) return hipErrorInvalidValue;
    hipLaunchKernelGGL(label_onehot_planes_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, lab, out, HW, npix, kout, k0);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// SPADE hidden activations for the Winograd ACE kernels (conv_wino.h), written ONLY where a boundary quad's 4 x 4 patch reads
// them (normalization.py:249-251 mlp_shared + relu), with the one-hot label planes of the styled ACEs behind
// the 128 hidden channels in the same pass.
//   * Persistent blocks of 1024 threads, one per CU: the WHOLE label table (171 rows x 128 channels, padded pitch, + a zero row)
//     and the 19 pre-summed rows A[j] = relu(bias + sum_t T[j][t]) sit in LDS for the block's lifetime (101 KB).
//   * Task = 1024 pixels as TR rows x TC columns with TC = min(W, 512): ROW-SHAPED, and block i takes tasks i, i + G, ... -- the
//     blocks running at the same time write neighbouring runs of the same rows of a plane.  (Tiles of 32 x 32 were measured first,
//     tools/hidden_bench.hip: 0.8 TB/s -- 256 CUs each scattering 128-byte pieces over a whole 1 MB plane, 148 planes at a time.)
//   * A pixel is WANTED when one of the (at most four) quads whose patch holds it is a boundary quad (some pixel of the quad has
//     u5 == 255; u5 == nullptr: every quad).  Wanted pixels are compacted in raster order into ONE list; work items = 64 list
//     entries x 16 channels, taken round-robin by the 16 waves: full waves, stores in runs of consecutive pixels.  A pixel whose
//     3 x 3 label neighbourhood is uniform (inside the image, label < 19) could read ONE pre-summed row instead of nine table rows
//     -- the same adds in the same order, bit-identical -- and does so when all 64 pixels of its item are of that kind.
// Pixels outside every boundary quad's patch keep whatever the buffer held: nothing reads them.
namespace hid {
constexpr int K = 128, RS = K + 4, ZROW = 19 * 9;
constexpr int T_FLOATS = (ZROW + 1) * RS, A_FLOATS = 19 * RS;
constexpr int LP_BYTES = 2304, QF_BYTES = 1024;      // label patch (TR + 2) x (TC + 4) <= 4 x 516 / 34 x 36; quad flags (TR/2 + 2) x (TC/2 + 2)
constexpr int LDS_BYTES = (T_FLOATS + A_FLOATS + K) * 4 + LP_BYTES + QF_BYTES + 1088 * 2 + 16 * 4 + 64;
}  // namespace hid

#ifndef HID_DBG
#define HID_DBG 0      // tools/hidden_bench.hip: 1 = no stores, 2 = no work items (timing ablations)
#endif
// the work of block `blk` of `nblk` (one launch per ACE: the grid; the grouped launch of the ACE prologue: the blocks of this ACE's entry)
__device__ __forceinline__ void spade_hidden_wq_block(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ u5,
                                                      const float* __restrict__ table, const float* __restrict__ bias,
                                                      float* __restrict__ out, int B, int H, int W, int kout, int onehot,
                                                      int tcs,        // tcs = log2(TC)
                                                      int pitch, int xoff,        // output planes: H rows of `pitch` floats, image column x at x + xoff
                                                      int blk, int nblk) {
    using namespace hid;
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    float* T = hsm;
    float* A = T + T_FLOATS;
    float* bs = A + A_FLOATS;
    uint8_t* Lp = reinterpret_cast<uint8_t*>(bs + K);
    uint8_t* qf = Lp + LP_BYTES;
    uint16_t* lst = reinterpret_cast<uint16_t*>(qf + QF_BYTES);      // wanted pixels of the task, raster order: tid | uniform << 15
    int* wc = reinterpret_cast<int*>(lst + 1088);                    // per-wave counts
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < (ZROW + 1) * K; i += 1024) {
        const int jt = i / K, kk = i % K;
        T[jt * RS + kk] = jt < ZROW ? table[(long long)jt * K + kk] : 0.f;
    }
    if (tid < K) bs[tid] = bias[tid];
    __syncthreads();
    for (int i = tid; i < 19 * K; i += 1024) {
        const int j = i / K, k = i % K;
        float a = bs[k];
#pragma unroll
        for (int t = 0; t < 9; ++t) a += T[(j * 9 + t) * RS + k];    // bias first, then the taps in order: as the per-pixel sum below
        A[j * RS + k] = a > 0.f ? a : 0.f;
    }
    const int TC = 1 << tcs, TR = 1024 >> tcs;
    const int LPW = TC + 4, LPH = TR + 2, QW = (TC >> 1) + 2, QH = (TR >> 1) + 2;
    const int txn = W >> tcs, tyn = H / TR, ntasks = B * txn * tyn;
    const long long HW = (long long)H * W;
    const long long PL = (long long)H * pitch;                       // floats per output plane
    for (int task = blk; task < ntasks; task += nblk) {
        const int b = task / (txn * tyn), tr = task - b * (txn * tyn);
        const int y0 = (tr / txn) * TR, x0 = (tr % txn) << tcs;
        const uint8_t* lb = lab + (long long)b * HW;
        __syncthreads();                                             // (the previous task's lists / the A rows above)
        for (int i = tid; i < LPH * (TC + 2); i += 1024) {
            const int py = i / (TC + 2), px = i - py * (TC + 2);
            const int y = y0 - 1 + py, x = x0 - 1 + px;
            Lp[py * LPW + px] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? lb[(long long)y * W + x] : (uint8_t)255;
        }
        for (int q = tid; q < QH * QW; q += 1024) {                  // boundary flags of the quads of the task + a ring of one quad
            const int qy = q / QW, qx = q - qy * QW;
            const int y = y0 + 2 * (qy - 1), x = x0 + 2 * (qx - 1);
            uint8_t f = 0;
            if ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) {      // (H, W even: a quad is inside or outside as a whole)
                if (u5) {
                    const uint8_t* up = u5 + (long long)b * HW + (long long)y * W + x;
                    const unsigned short r0 = *reinterpret_cast<const unsigned short*>(up), r1 = *reinterpret_cast<const unsigned short*>(up + W);
                    f = ((r0 & 0xFF) == 255 || (r0 >> 8) == 255 || (r1 & 0xFF) == 255 || (r1 >> 8) == 255) ? 1 : 0;
                } else {
                    f = 1;
                }
            }
            qf[q] = f;
        }
        __syncthreads();
        const int ty = tid >> tcs, tx = tid & (TC - 1);
        const int r0 = (ty + 1) >> 1, c0 = (tx + 1) >> 1;            // pixel (ty, tx) lies in the patches of quads r0 - 1 .. r0, c0 - 1 .. c0 (+ 1: ring)
        bool wanted = (qf[r0 * QW + c0] | qf[r0 * QW + c0 + 1] | qf[(r0 + 1) * QW + c0] | qf[(r0 + 1) * QW + c0 + 1]) != 0;
        const uint8_t* lc = Lp + ty * LPW + tx;                      // 3 x 3 neighbourhood: rows ty .. ty + 2, columns tx .. tx + 2 of the patch
        const uint8_t cl = lc[LPW + 1];
        bool uni = cl < 19;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) uni = uni && lc[dy * LPW + dx] == cl;
        // Written at the granularity of aligned groups of 16 pixels (64 bytes, one full write request): 32-byte pieces -- the 8-pixel
        // bands along vertical region edges -- cost more than they save (tools/hidden_bench.hip, 512^2 on the benchmark labels:
        // 40 % of the bytes in 1039 us at pixel granularity against 471 us for ALL of them).  The extra pixels get their true values.
        const unsigned long long m1 = __ballot(wanted);
        wanted = ((m1 >> (lane & 48)) & 0xFFFFull) != 0ull;          // (TC >= 32: the 16 lanes of a group are 16 consecutive pixels of a row)
        const unsigned long long mW = __ballot(wanted);
        if (lane == 0) wc[wave] = __popcll(mW);
        __syncthreads();
        int base = 0, n = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            if (w < wave) base += wc[w];
            n += wc[w];
        }
        if (wanted) lst[base + __popcll(mW & ((1ull << lane) - 1ull))] = (uint16_t)(tid | (uni ? 0x8000 : 0));
        __syncthreads();
        // Work items: 64 consecutive list entries (raster order: a wave's stores are runs of consecutive pixels, as long as the
        // wanted band is wide) x half a slab of 16 channels.  The channel slabs are the OUTER loop: at any time the 16 waves of the
        // block -- and the blocks running in step with it -- write the same 32 planes.  (Measured first, tools/hidden_bench.hip: one
        // list per kind of pixel.  The non-uniform pixels are 2-pixel strips at the region edges; listed apart they become 8-byte
        // stores and cut the uniform runs into unaligned pieces -- 8 write requests per wave store instead of 4, 0.8 TB/s.)
        // A chunk whose pixels all have a uniform neighbourhood reads ONE pre-summed row per pixel; any other chunk the nine rows.
        const int nch = (n + 63) >> 6;
        for (int pass = 0; pass < ((HID_DBG & 2) ? 0 : (onehot ? 5 : 4)); ++pass) {
            for (int it = wave; it < 2 * nch; it += 16) {
                const int c = it >> 1, half = it & 1;
                const int e = c * 64 + lane;
                const bool valid = (HID_DBG & 1) ? (e < -1) : e < n;
                const int ent = valid ? lst[e] : 0x8000;
                const int pid = ent & 1023;
                const int py = pid >> tcs, px = pid & (TC - 1);
                const uint8_t* ll = Lp + py * LPW + px;
                const int jc = ll[LPW + 1];
                const long long pofs = (long long)(y0 + py) * pitch + xoff + x0 + px;
                if (pass == 4) {                                     // one-hot planes K + 10 half .. K + 10 half + 9 (plane K + 19 stays zero)
                    float* oh = out + ((long long)b * kout + K + half * 10) * PL + pofs;
                    if (valid) {
#pragma unroll
                        for (int q = 0; q < 10; ++q) oh[q * PL] = (half * 10 + q == jc && jc < 19) ? 1.f : 0.f;
                    }
                    continue;
                }
                const int k0 = pass * 32 + half * 16;
                float* op = out + ((long long)b * kout + k0) * PL + pofs;
                if (!__all((ent & 0x8000) != 0)) {
                    int jt[9];
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        const int j = ll[(t / 3) * LPW + t % 3];     // 255 outside the image; labels >= 19: all-zero one-hot
                        jt[t] = (j < 19 ? j * 9 + t : ZROW) * RS + k0;
                    }
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        float4 a = *reinterpret_cast<const float4*>(bs + k0 + gq * 4);
#pragma unroll
                        for (int t = 0; t < 9; ++t) {
                            const float4 r = *reinterpret_cast<const float4*>(T + jt[t] + gq * 4);
                            a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w;
                        }
                        a.x = a.x > 0.f ? a.x : 0.f; a.y = a.y > 0.f ? a.y : 0.f;
                        a.z = a.z > 0.f ? a.z : 0.f; a.w = a.w > 0.f ? a.w : 0.f;
                        if (valid) {                                 // (one running pointer: hoisted plane addresses cost two registers each)
                            op[0] = a.x; op[PL] = a.y; op[2 * PL] = a.z; op[3 * PL] = a.w;
                        }
                        op += 4 * PL;
                        __builtin_amdgcn_sched_barrier(0);           // one group of table reads in flight, not all of them (128 registers)
                    }
                } else {
                    const float* ar = A + (jc < 19 ? jc : 0) * RS + k0;
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        const float4 a = *reinterpret_cast<const float4*>(ar + gq * 4);
                        if (valid) {
                            op[0] = a.x; op[PL] = a.y; op[2 * PL] = a.z; op[3 * PL] = a.w;
                        }
                        op += 4 * PL;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(1024) void spade_hidden_wq_kernel(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ u5,
                                                               const float* __restrict__ table, const float* __restrict__ bias,
                                                               float* __restrict__ out, int B, int H, int W, int kout, int onehot, int tcs,
                                                               int pitch, int xoff,
                                                               const int* __restrict__ skip_if_patch) {      // device flag: 1 = spade_hidden_patch serves this level
    if (skip_if_patch && *skip_if_patch == 1) return;
    spade_hidden_wq_block(lab, u5, table, bias, out, B, H, W, kout, onehot, tcs, pitch, xoff, (int)blockIdx.x, (int)gridDim.x);
}

// ACE prologue (sean_model.cpp): the hidden planes of several ACEs from one launch -- block -> (entry, block of the entry); a block
// keeps ONE label table in LDS, so the entries own disjoint runs of blocks
__global__ __launch_bounds__(1024) void spade_hidden_wq_grouped_kernel(HiddenGroup g) {
    if (g.memo_hit && *g.memo_hit) return;      // (label memo: every entry writes its own buffer, which still holds these planes)
    int k = 0;
    while (k + 1 < g.n && (int)blockIdx.x >= g.e[k + 1].start) ++k;
    const HiddenGroup::Entry& e = g.e[k];
    spade_hidden_wq_block(e.lab, e.u5, e.table, e.bias, e.out, g.B, e.H, e.W, e.kout, e.onehot, e.tcs, e.pitch, e.xoff, (int)blockIdx.x - e.start,
                          e.nblk);
}

bool spade_hidden_wq_supported(int H, int W) {
    if (H % 32 || W % 32 || H < 32 || W < 32) return false;
    const int TC = (W & (W - 1)) ? 32 : (W < 512 ? W : 512), TR = 1024 / TC;      // (widths that are not powers of two: tiles of 32 x 32)
    return H % TR == 0;
}

__global__ void spade_hidden_level_kernel(const uint8_t* lab, const uint8_t* u5, const unsigned* gq, const int* gq_n, int gq_cap, const int* chunk_base,
                                          const int* mode, const float* table, const float* bias, float* out, float* patch, int B, int H, int W, int kout,
                                          int onehot, int tcs, int pitch, int xoff, const int* memo_hit);      // (below, beside the patch kernel)
// LDS limit of the three kernels, once per device: the first call of any of their launchers sets all three
static hipError_t spade_hidden_wq_attr(int& ncu) {
    return dyn_lds<spade_hidden_wq_kernel, spade_hidden_wq_grouped_kernel, spade_hidden_level_kernel>(hid::LDS_BYTES, &ncu);
}
static int spade_hidden_wq_tcs(int W) {
    const int TC = (W & (W - 1)) ? 32 : (W < 512 ? W : 512);
    int tcs = 0;
    while ((1 << tcs) < TC) ++tcs;
    return tcs;
}

hipError_t spade_hidden_wq(const uint8_t* lab, const uint8_t* u5, const float* table, const float* bias, float* out, int B, int H, int W,
                           int kout, int onehot, hipStream_t s, int pitch, int xoff, const int* skip_if_patch) {
    if (!spade_hidden_wq_supported(H, W) || kout < hid::K + (onehot ? 20 : 0)) return hipErrorInvalidValue;
    if (pitch <= 0) { pitch = W; xoff = 0; }
    if (xoff < 0 || (xoff > 0 && pitch < W + xoff + 1)) return hipErrorInvalidValue;
    int ncu = 0;
    if (hipError_t e = spade_hidden_wq_attr(ncu)) return e;
    const int tcs = spade_hidden_wq_tcs(W);
    const int ntasks = B * (H * W / 1024);
    const int grid = persistent_grid(ntasks, ncu);
    hipLaunchKernelGGL(spade_hidden_wq_kernel, dim3(grid), dim3(1024), hid::LDS_BYTES, s, lab, u5, table, bias, out, B, H, W, kout, onehot, tcs,
                       pitch, xoff, skip_if_patch);
    return hipGetLastError();
}

// every entry gets the blocks its own launch would get (one per task, at most one per CU); the entries' runs of blocks follow each other
hipError_t spade_hidden_wq_grouped(HiddenGroup& g, hipStream_t s) {
    if (g.n < 0 || g.n > HiddenGroup::MAX || g.B < 1) return hipErrorInvalidValue;
    if (g.n == 0) return hipSuccess;
    int ncu = 0;
    if (hipError_t e = spade_hidden_wq_attr(ncu)) return e;
    int grid = 0;
    for (int k = 0; k < g.n; ++k) {
        HiddenGroup::Entry& e = g.e[k];
        if (!spade_hidden_wq_supported(e.H, e.W) || e.kout < hid::K + (e.onehot ? 20 : 0) || !e.lab || !e.table || !e.bias || !e.out) return hipErrorInvalidValue;
        if (e.pitch <= 0) { e.pitch = e.W; e.xoff = 0; }
        if (e.xoff < 0 || (e.xoff > 0 && e.pitch < e.W + e.xoff + 1)) return hipErrorInvalidValue;
        e.tcs = spade_hidden_wq_tcs(e.W);
        const int ntasks = g.B * (e.H * e.W / 1024);
        e.start = grid;
        e.nblk = ntasks < ncu ? ntasks : ncu;
        grid += e.nblk;
    }
    hipLaunchKernelGGL(spade_hidden_wq_grouped_kernel, dim3(grid), dim3(1024), hid::LDS_BYTES, s, g);
    return hipGetLastError();
}

// ---- the same hidden activations as pre-gathered PATCHES of the boundary quads (conv_wino.h WinoAceParams::patch) ---------------------------
// For levels that the straight-edge reduction leaves with few, scattered boundary quads.  Block = one chunk of 64 consecutive quads of a
// sample's list (clamped like the gather kernel's task_quad), thread = (patch row py, slot, patch column px): its pixel's 128 hidden
// channels (bias + nine table rows in tap order + ReLU: the arithmetic of spade_hidden_wq_kernel, bit for bit) and, for a styled ACE, the
// 20 one-hot planes -- written as [channel][py][slot][px]: 256 consecutive threads store one contiguous KB.  A pixel outside the image
// is zero in every channel (the zero padding of the gamma / beta conv).  Runs only when *mode == 1 (wino_chunk_base).
__device__ __forceinline__ void spade_hidden_patch_block(const uint8_t* __restrict__ lab, const unsigned* __restrict__ gq, const int* __restrict__ gq_n,
                                                         int gq_cap, const int* __restrict__ chunk_base,
                                                         const float* __restrict__ table, const float* __restrict__ bias, float* __restrict__ patch,
                                                         int B, int H, int W, int kout, int blk, int nblk) {
    using namespace hid;
    extern __shared__ __attribute__((aligned(16))) float hsm[];
    float* T = hsm;
    float* bs = T + T_FLOATS;
    __shared__ int cb[34];
    const int tid = threadIdx.x;
    for (int i = tid; i < (ZROW + 1) * K; i += 1024) {
        const int jt = i / K, kk = i % K;
        T[jt * RS + kk] = jt < ZROW ? table[(long long)jt * K + kk] : 0.f;
    }
    if (tid < K) bs[tid] = bias[tid];
    if (tid <= B) cb[tid] = chunk_base[tid];
    __syncthreads();
    const int py = tid >> 8, slot = (tid >> 2) & 63, px = tid & 3;
    const int total = cb[B];
    const long long HW = (long long)H * W;
    for (int g = blk; g < total; g += nblk) {
        int b = 0;
        while (b + 1 < B && cb[b + 1] <= g) ++b;
        const int chunk = g - cb[b], nq = gq_n[b];
        int qi = chunk * 64 + slot;
        qi = qi < nq ? qi : nq - 1;
        const unsigned q = gq[(long long)b * gq_cap + qi];
        const int Y = (int)(q >> 16) - 1 + py, X = (int)(q & 0xFFFFu) - 1 + px;
        const bool in = (unsigned)Y < (unsigned)H && (unsigned)X < (unsigned)W;
        const uint8_t* lb = lab + (long long)b * HW;
        int jt[9], jc = 255;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int yy = Y + t / 3 - 1, xx = X + t % 3 - 1;
            const int j = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? lb[(long long)yy * W + xx] : 255;
            if (t == 4) jc = j;
            jt[t] = (j < 19 ? j * 9 + t : ZROW) * RS;
        }
        float* op = patch + (long long)g * kout * 1024 + (py * 64 + slot) * 4 + px;        // channel c at + c * 1024
#pragma unroll 2
        for (int k0 = 0; k0 < K; k0 += 4) {
            float4 a = *reinterpret_cast<const float4*>(bs + k0);
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float4 r = *reinterpret_cast<const float4*>(T + jt[t] + k0);
                a.x += r.x; a.y += r.y; a.z += r.z; a.w += r.w;
            }
            a.x = (in && a.x > 0.f) ? a.x : 0.f; a.y = (in && a.y > 0.f) ? a.y : 0.f;
            a.z = (in && a.z > 0.f) ? a.z : 0.f; a.w = (in && a.w > 0.f) ? a.w : 0.f;
            op[0] = a.x; op[1024] = a.y; op[2048] = a.z; op[3072] = a.w;
            op += 4096;
        }
        if (kout > K) {
#pragma unroll
            for (int j = 0; j < 20; ++j) op[j * 1024] = (in && j == jc && jc < 19) ? 1.f : 0.f;      // (plane K + 19 stays zero)
        }
    }
}
__global__ __launch_bounds__(1024) void spade_hidden_patch_kernel(const uint8_t* __restrict__ lab, const unsigned* __restrict__ gq, const int* __restrict__ gq_n,
                                                                  int gq_cap, const int* __restrict__ chunk_base, const int* __restrict__ mode,
                                                                  const float* __restrict__ table, const float* __restrict__ bias, float* __restrict__ patch,
                                                                  int B, int H, int W, int kout) {
    if (*mode != 1) return;
    spade_hidden_patch_block(lab, gq, gq_n, gq_cap, chunk_base, table, bias, patch, B, H, W, kout, (int)blockIdx.x, (int)gridDim.x);
}
// Both sources of a gather-mode level from ONE launch (chunks with the ACE prologue): the device flag picks the body -- *mode == 1 the
// pre-gathered patches, else the padded planes -- where the two kernels above are launched one after the other and one returns at once.
// One block per CU, as both take when the level has at least that many tasks; a block beyond the planes' task count only loads its table.
__global__ __launch_bounds__(1024) void spade_hidden_level_kernel(const uint8_t* __restrict__ lab, const uint8_t* __restrict__ u5, const unsigned* __restrict__ gq,
                                                                  const int* __restrict__ gq_n, int gq_cap, const int* __restrict__ chunk_base,
                                                                  const int* __restrict__ mode, const float* __restrict__ table,
                                                                  const float* __restrict__ bias, float* __restrict__ out, float* __restrict__ patch, int B,
                                                                  int H, int W, int kout, int onehot, int tcs, int pitch, int xoff,
                                                                  const int* __restrict__ memo_hit) {
    // label memo: `patch` is this ACE's own buffer and still holds the patches of these labels; the planes are shared by the level, so they are rebuilt
    if (*mode == 1 && memo_hit && *memo_hit) return;
    if (*mode == 1) spade_hidden_patch_block(lab, gq, gq_n, gq_cap, chunk_base, table, bias, patch, B, H, W, kout, (int)blockIdx.x, (int)gridDim.x);
    else spade_hidden_wq_block(lab, u5, table, bias, out, B, H, W, kout, onehot, tcs, pitch, xoff, (int)blockIdx.x, (int)gridDim.x);
}
hipError_t spade_hidden_level(const uint8_t* lab, const uint8_t* u5, const unsigned* gq, const int* gq_n, int gq_cap, const int* chunk_base, const int* mode,
                              const float* table, const float* bias, float* out, float* patch, int B, int H, int W, int kout, int onehot, int pitch,
                              int xoff, hipStream_t s, const int* memo_hit) {
    if (B < 1 || B > 32 || kout != hid::K + (onehot ? 20 : 0) || !spade_hidden_wq_supported(H, W) || !mode || !chunk_base || !gq || !gq_n || !patch || !out)
        return hipErrorInvalidValue;
    if (pitch <= 0) { pitch = W; xoff = 0; }
    if (xoff < 0 || (xoff > 0 && pitch < W + xoff + 1)) return hipErrorInvalidValue;
    int ncu = 0;
    if (hipError_t e = spade_hidden_wq_attr(ncu)) return e;
    hipLaunchKernelGGL(spade_hidden_level_kernel, dim3(ncu), dim3(1024), hid::LDS_BYTES, s, lab, u5, gq, gq_n, gq_cap, chunk_base, mode, table, bias,
                       out, patch, B, H, W, kout, onehot, spade_hidden_wq_tcs(W), pitch, xoff, memo_hit);
    return hipGetLastError();
}
hipError_t spade_hidden_patch(const uint8_t* lab, const unsigned* gq, const int* gq_n, int gq_cap, const int* chunk_base, const int* mode,
                              const float* table, const float* bias, float* patch, int B, int H, int W, int kout, hipStream_t s) {
    if (B < 1 || B > 32 || (kout != hid::K && kout != hid::K + 20)) return hipErrorInvalidValue;
    constexpr int LDS = (hid::T_FLOATS + hid::K) * 4;
    int ncu = 0;
    if (hipError_t e = dyn_lds<spade_hidden_patch_kernel>(LDS, &ncu)) return e;
    hipLaunchKernelGGL(spade_hidden_patch_kernel, dim3(ncu), dim3(1024), LDS, s, lab, gq, gq_n, gq_cap, chunk_base, mode, table, bias, patch, B,
                       H, W, kout);
    return hipGetLastError();
}
// chunk_base[b] = chunks of 64 quads of the samples before b (chunk_base[B]: all); *mode = 1 when they fit `cap_chunks` (and there are any)
__global__ void wino_chunk_base_kernel(const int* __restrict__ gq_n, int B, int cap_chunks, int* __restrict__ chunk_base, int* __restrict__ mode) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int o = 0;
    for (int b = 0; b < B; ++b) {
        chunk_base[b] = o;
        o += (gq_n[b] + 63) >> 6;
    }
    chunk_base[B] = o;
    *mode = (o > 0 && o <= cap_chunks) ? 1 : 0;
}
hipError_t wino_chunk_base(const int* gq_n, int B, int cap_chunks, int* chunk_base, int* mode, hipStream_t s) {
    hipLaunchKernelGGL(wino_chunk_base_kernel, dim3(1), dim3(64), 0, s, gq_n, B, cap_chunks, chunk_base, mode);
    return hipGetLastError();
}

// Same computation, output in the SH16 layout of conv_sh16.h: [B][K/8][2][H*W][8] _Float16 (hi plane, lo plane).
// One thread = one pixel x 32 channels = 4 groups; every store is one aligned 16-byte unit, lanes on consecutive
// pixels -> 1 KiB contiguous per wave store.
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256) void onehot_conv3x3_sh16_kernel(const uint8_t* __restrict__ lab,
                                                                  const float* __restrict__ table,
                                                                  const float* __restrict__ bias, uint4* __restrict__ out,
                                                                  int B, int H, int W, int K, int relu, float scale, int bf16,
                                                                  const uint8_t* __restrict__ need, const int* __restrict__ tcnt) {
    // Table slice in LDS with a padded row pitch (36 floats: consecutive (label, tap) rows start 4 banks apart, so lanes
    // that hold different labels do not collide on the same banks) and one extra all-zero row that taps outside the image
    // point at -- every lane then issues the same 9 x 2 ds_read_b128 per 8 channels, no predication.
    constexpr int RS = OH_KC + 4, ZROW = 19 * 9;
    bool wanted = true;
    if (need) {       // exact SPADE-interior reduction: only pixels next to a boundary pixel are ever read (ace_sparse.h)
        const long long pq = blockIdx.x * 256LL + threadIdx.x;
        wanted = pq < (long long)B * H * W && need[pq];
        if (__syncthreads_or(wanted) == 0) return;
    }
    if (tcnt) {       // tile-skip mode (f16x3 path): the conv only stages the tiles of 32 x 16 that hold a boundary pixel, plus a
                      // one-pixel ring around them -- pixels further inside skipped tiles are never read
        const long long pq = blockIdx.x * 256LL + threadIdx.x;
        wanted = false;
        if (pq < (long long)B * H * W) {
            const long long hw = (long long)H * W;
            const int bq = (int)(pq / hw), yq = (int)((pq % hw) / W), xq = (int)(pq % W);
            const int ttx = (W + 31) >> 5, tty = (H + 15) >> 4;
            const int ya = (yq > 0 ? yq - 1 : 0) >> 4, yb = (yq + 1 < H ? yq + 1 : H - 1) >> 4;
            const int xa = (xq > 0 ? xq - 1 : 0) >> 5, xb = (xq + 1 < W ? xq + 1 : W - 1) >> 5;
            const int* tc = tcnt + (long long)bq * tty * ttx;
            wanted = (tc[ya * ttx + xa] | tc[ya * ttx + xb] | tc[yb * ttx + xa] | tc[yb * ttx + xb]) != 0;
        }
        if (__syncthreads_or(wanted) == 0) return;
    }
    sh16_mode_on();       // (the scale comes from a bound of the table sums: nothing can saturate; kept for uniformity)
    __shared__ __attribute__((aligned(16))) float T[(ZROW + 1) * RS];
    __shared__ __attribute__((aligned(16))) float bs[OH_KC];
    const int k0 = blockIdx.y * OH_KC;
    for (int i = threadIdx.x; i < (ZROW + 1) * OH_KC; i += 256) {
        const int jt = i / OH_KC, kk = i % OH_KC;
        T[jt * RS + kk] = (jt < ZROW && k0 + kk < K) ? table[(long long)jt * K + k0 + kk] : 0.f;
    }
    if (threadIdx.x < OH_KC) bs[threadIdx.x] = (k0 + threadIdx.x < K) ? bias[k0 + threadIdx.x] : 0.f;
    __syncthreads();
    const long long HW = (long long)H * W;
    const long long pix = blockIdx.x * 256LL + threadIdx.x;
    if (pix >= B * HW || !wanted) return;
    const int b = (int)(pix / HW);
    const int y = (int)((pix % HW) / W), x = (int)(pix % W);
    int jt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
        const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        const int j = lab[b * HW + (in ? (long long)yy * W + xx : 0)];
        jt[t] = (in && j < 19 ? j * 9 + t : ZROW) * RS;         // labels >= 19 ("no class"): all-zero one-hot
    }
    const int G = (K + 7) / 8;
#pragma unroll
    for (int gq = 0; gq < OH_KC / 8; ++gq) {
        const int g = k0 / 8 + gq;
        if (g >= G) break;
        float4 a0 = *reinterpret_cast<const float4*>(bs + gq * 8), a1 = *reinterpret_cast<const float4*>(bs + gq * 8 + 4);
#pragma unroll
        for (int t = 0; t < 9; ++t) {                       // same summation order as the f32 kernel (+0.f for outside taps)
            const float4* r = reinterpret_cast<const float4*>(T + jt[t] + gq * 8);
            const float4 r0 = r[0], r1 = r[1];
            a0.x += r0.x; a0.y += r0.y; a0.z += r0.z; a0.w += r0.w;
            a1.x += r1.x; a1.y += r1.y; a1.z += r1.z; a1.w += r1.w;
        }
        const float v8[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        h8 vh, vl;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = v8[e];
            if (relu) v = v > 0.f ? v : 0.f;
            if (k0 + gq * 8 + e >= K) v = 0.f;
            _Float16 h, l;
            sh16_split_any(v, scale, bf16, h, l);
            vh[e] = h;
            vl[e] = l;
        }
        const long long unit = (((long long)b * G + g) * 2) * HW + (pix % HW);
        // streaming stores: the planes are consumed by the next kernel from HBM/L2, never re-read here
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, vh), reinterpret_cast<u32x4*>(out + unit));
        __builtin_nontemporal_store(__builtin_bit_cast(u32x4, vl), reinterpret_cast<u32x4*>(out + unit + HW));
    }
}

// Persistent variant for the `need`-masked launches of the exact SPADE-interior reduction (tools/interior_bench.hip measures
// both).  The kernel above stages its 25 KB table slice once per 256 pixels -- 22 KB of table reads for at most 32 KB of
// output, and for far less where only the pixels next to a boundary are wanted.  Here a block keeps its slice in LDS and walks
// over blocks of 32 x 8 pixels (grid-stride); a wave whose 2 x 32 pixels hold no wanted pixel moves on without a barrier.
__global__ __launch_bounds__(256) void onehot_conv3x3_sh16_need_kernel(const uint8_t* __restrict__ lab,
                                                                       const float* __restrict__ table,
                                                                       const float* __restrict__ bias, uint4* __restrict__ out,
                                                                       int B, int H, int W, int K, int relu, float scale, int bf16,
                                                                       const uint8_t* __restrict__ need) {
    constexpr int RS = OH_KC + 4, ZROW = 19 * 9;
    sh16_mode_on();
    __shared__ __attribute__((aligned(16))) float T[(ZROW + 1) * RS];
    __shared__ __attribute__((aligned(16))) float U[19 * RS];          // U[j] = bias + T[j][0] + ... + T[j][8], added in tap order
    __shared__ __attribute__((aligned(16))) float bs[OH_KC];
    const int k0 = blockIdx.y * OH_KC;
    for (int i = threadIdx.x; i < (ZROW + 1) * (OH_KC / 4); i += 256) {
        const int jt = i / (OH_KC / 4), kk = (i % (OH_KC / 4)) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (jt < ZROW) {
            if (k0 + kk + 3 < K && (K & 3) == 0) {
                v = *reinterpret_cast<const float4*>(table + (long long)jt * K + k0 + kk);
            } else {
                const float* tp = table + (long long)jt * K + k0 + kk;
                v.x = k0 + kk < K ? tp[0] : 0.f; v.y = k0 + kk + 1 < K ? tp[1] : 0.f;
                v.z = k0 + kk + 2 < K ? tp[2] : 0.f; v.w = k0 + kk + 3 < K ? tp[3] : 0.f;
            }
        }
        *reinterpret_cast<float4*>(T + jt * RS + kk) = v;
    }
    if (threadIdx.x < OH_KC) bs[threadIdx.x] = (k0 + threadIdx.x < K) ? bias[k0 + threadIdx.x] : 0.f;
    __syncthreads();
    // A pixel whose 3x3 neighbourhood is inside the image and holds one label j < 19 sums the nine rows of that label: the same
    // adds in the same order are done once here, and a wave whose wanted pixels are all of that kind reads 2 x 16 bytes of LDS
    // per 8 channels instead of 18 x 16 (the kernel is bound by its LDS reads).  Bit-identical by construction.
    for (int i = threadIdx.x; i < 19 * OH_KC; i += 256) {
        const int j = i / OH_KC, kk = i % OH_KC;
        float a = bs[kk];
#pragma unroll
        for (int t = 0; t < 9; ++t) a += T[(j * 9 + t) * RS + kk];
        U[j * RS + kk] = a;
    }
    __syncthreads();
    // Blocks of 32 x 32 pixels.  The wanted pixels are thin bands (the 3-pixel neighbourhood of label boundaries): taken as they
    // lie, nearly every wave of 64 consecutive pixels holds a few of them and runs the whole gather for 3 active lanes -- the
    // masked launch then costs what the dense one does (measured: 495 vs 518 us at 512^2 with 18 % of the pixels wanted).  So the
    // block first compacts its wanted pixels into an LDS list (four independent `need` loads per thread, ballot + one LDS atomic
    // per wave), then walks the list with full waves.
    __shared__ unsigned short plist[1024];
    __shared__ int pcount;
    if (threadIdx.x == 0) pcount = 0;
    __syncthreads();
    const int HW = H * W, tpr = (W + 31) >> 5, tpc = (H + 31) >> 5, ntile = B * tpr * tpc;
    const int G = (K + 7) / 8, lane = threadIdx.x & 63;
    for (int tl = blockIdx.x; tl < ntile; tl += gridDim.x) {
        const int b = tl / (tpr * tpc), r = tl - b * (tpr * tpc), tyi = r / tpr;
        const int x0 = (r - tyi * tpr) * 32, y0 = tyi * 32;
        const uint8_t* lb = lab + (long long)b * HW;
        bool wanted[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x0 + (threadIdx.x & 31), y = y0 + (threadIdx.x >> 5) + 8 * i;
            wanted[i] = x < W && y < H && need[(long long)b * HW + y * W + x];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned long long m = __ballot(wanted[i]);
            if (m == 0ull) continue;
            int base = 0;
            if (lane == 0) base = atomicAdd(&pcount, __popcll(m));
            base = __shfl(base, 0, 64);
            if (wanted[i])
                plist[base + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)((((threadIdx.x >> 5) + 8 * i) << 5) | (threadIdx.x & 31));
        }
        __syncthreads();
        const int n = pcount;
        for (int e = threadIdx.x; e < n; e += 256) {
            const int pl = plist[e];
            const int x = x0 + (pl & 31), y = y0 + (pl >> 5), pix = y * W + x;
            int jt[9];
            const int jc = lb[pix];
            bool uni = jc < 19;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
                const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                const int j = lb[in ? yy * W + xx : 0];
                jt[t] = (in && j < 19 ? j * 9 + t : ZROW) * RS;     // labels >= 19 ("no class"): all-zero one-hot
                uni = uni && in && j == jc;
            }
            const bool fast = __ballot(!uni) == 0ull;              // (only lanes with a list entry are active)
#pragma unroll
            for (int gq = 0; gq < OH_KC / 8; ++gq) {
                const int g = k0 / 8 + gq;
                if (g >= G) break;
                float4 a0, a1;
                if (fast) {
                    a0 = *reinterpret_cast<const float4*>(U + jc * RS + gq * 8);
                    a1 = *reinterpret_cast<const float4*>(U + jc * RS + gq * 8 + 4);
                } else {
                    a0 = *reinterpret_cast<const float4*>(bs + gq * 8);
                    a1 = *reinterpret_cast<const float4*>(bs + gq * 8 + 4);
#pragma unroll
                    for (int t = 0; t < 9; ++t) {               // same summation order as the kernels above
                        const float4* rr = reinterpret_cast<const float4*>(T + jt[t] + gq * 8);
                        const float4 r0 = rr[0], r1 = rr[1];
                        a0.x += r0.x; a0.y += r0.y; a0.z += r0.z; a0.w += r0.w;
                        a1.x += r1.x; a1.y += r1.y; a1.z += r1.z; a1.w += r1.w;
                    }
                }
                const float v8[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                h8 vh, vl;
#pragma unroll
                for (int e2 = 0; e2 < 8; ++e2) {
                    float v = v8[e2];
                    if (relu) v = v > 0.f ? v : 0.f;
                    if (k0 + gq * 8 + e2 >= K) v = 0.f;
                    _Float16 h, l;
                    sh16_split_any(v, scale, bf16, h, l);
                    vh[e2] = h;
                    vl[e2] = l;
                }
                const long long unit = (((long long)b * G + g) * 2) * HW + pix;
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                __builtin_nontemporal_store(__builtin_bit_cast(u32x4, vh), reinterpret_cast<u32x4*>(out + unit));
                __builtin_nontemporal_store(__builtin_bit_cast(u32x4, vl), reinterpret_cast<u32x4*>(out + unit + HW));
            }
        }
        __syncthreads();                                          // every wave has read the list
        if (threadIdx.x == 0) pcount = 0;
        // (the next iteration's atomics come after its own barrier-free ballot phase: order them behind the reset)
        __syncthreads();
    }
}

// need_impl 0: the compacting kernel where the wanted pixels are sparse (levels of 512^2 and up: at 256^2 and below most pixels
// of a segmentation map are within 3 pixels of a boundary and the plain kernel is faster), 1 = never, 2 = always (A/B)
hipError_t onehot_conv3x3_sh16(const uint8_t* lab, const float* table, const float* bias, void* out, int B, int H, int W,
                               int K, int relu, float scale, hipStream_t s, int bf16, const uint8_t* need, const int* tile_cnt,
                               int need_impl) {
    if (need && !tile_cnt && (need_impl == 0 ? W >= 512 : need_impl == 2)) {
        const int ntile = B * ((W + 31) / 32) * ((H + 31) / 32), ky = (K + OH_KC - 1) / OH_KC;
        int gx = 1280 / ky;                                   // 5 blocks of 28 KB LDS per CU
        if (gx > ntile) gx = ntile;
        hipLaunchKernelGGL(onehot_conv3x3_sh16_need_kernel, dim3((unsigned)gx, (unsigned)ky), dim3(256), 0, s, lab, table, bias,
                           static_cast<uint4*>(out), B, H, W, K, relu, scale, bf16, need);
        return hipGetLastError();
    }
    const long long npix = (long long)B * H * W;
    dim3 grid((unsigned)((npix + 255) / 256), (unsigned)((K + OH_KC - 1) / OH_KC));
    hipLaunchKernelGGL(onehot_conv3x3_sh16_kernel, grid, dim3(256), 0, s, lab, table, bias, static_cast<uint4*>(out), B, H,
                       W, K, relu, scale, bf16, need, tile_cnt);
    return hipGetLastError();
}

// SH16 -> f32 NCHW (test taps only).  single: the single-term paths read the hi plane alone, so that is what the tap shows (their interior pass
// does not even write the lo plane)
__global__ void sh16_decode_kernel(const _Float16* __restrict__ in, float* __restrict__ out, int B, int C, long long HW,
                                   float inv_scale, const unsigned* __restrict__ amax, int bf16, int single) {
    if (amax) inv_scale /= sh16_dyn_extra(*amax);
    const long long n = (long long)B * C * HW;
    const int G = (C + 7) / 8;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long p = i % HW;
        const int c = (int)((i / HW) % C), b = (int)(i / (HW * C));
        const long long unit = (((long long)b * G + c / 8) * 2) * HW + p;
        if (bf16) out[i] = (float)__builtin_bit_cast(__bf16, in[unit * 8 + (c & 7)]) * inv_scale;
        else if (single) out[i] = (float)in[unit * 8 + (c & 7)] * inv_scale;
        else out[i] = ((float)in[unit * 8 + (c & 7)] + (float)in[(unit + HW) * 8 + (c & 7)]) * inv_scale;
    }
}
hipError_t sh16_decode(const void* in, float* out, int B, int C, long long HW, float scale, const unsigned* amax,
                       hipStream_t s, int bf16, int single) {
    hipLaunchKernelGGL(sh16_decode_kernel, dim3(4096), dim3(256), 0, s, static_cast<const _Float16*>(in), out, B, C, HW,
                       1.f / scale, amax, bf16, single);
    return hipGetLastError();
}

// C4 [B][C/4][HW][4] -> f32 NCHW (test taps only)
__global__ void c4_decode_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int C, long long HW) {
    const long long n = (long long)B * C * HW;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long p = i % HW;
        const int c = (int)((i / HW) % C), b = (int)(i / (HW * C));
        out[i] = in[(((long long)b * (C >> 2) + (c >> 2)) * HW + p) * 4 + (c & 3)];
    }
}
hipError_t c4_decode(const float* in, float* out, int B, int C, long long HW, hipStream_t s) {
    hipLaunchKernelGGL(c4_decode_kernel, dim3(4096), dim3(256), 0, s, in, out, B, C, HW);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Per-region style projection: mu[b,j,:] = relu(fc_mu_j(code[b,j]))  (normalization.py:134,146 + :191-215).
// Weight-bandwidth bound (19 x 1 MB per ACE).  One wave per 4 output features; lanes split the 512-long dot
// product (8 floats each, two float4 loads), wave shuffle reduction, up to FCMU_BT samples per pass.
// Output is written as the [512][Npad] "image" the LUT GEMM (1x1 conv, NHWC epilogue) consumes: column b*19+j.
// TR: the wave's 32 partial sums (4 features x 8 samples) go through ONE transposed butterfly instead of 32 independent ones: at
// offset 32 the lanes below 32 keep values 0..15 and send 16..31 (the upper lanes the reverse), then 8, 4, 2, 1 values per lane at
// offsets 16 .. 2, and a plain exchange at offset 1: 32 shuffles instead of 192.  Every sum still adds lane l and lane l ^ off in the
// order 32, 16, .., 1 (the same additions, commuted: the same bits); lane l ends with value l >> 1 and the even lanes store.
constexpr int FCMU_BT = 8;

template <bool TR>
__device__ __forceinline__ void fc_mu_body(const float* __restrict__ codes, const float* __restrict__ Wt,
                                           const float* __restrict__ bias, float* __restrict__ mu_img, int B, int Npad,
                                           float* __restrict__ mu_rows, int sh16, int bs, float scale,
                                           unsigned* __restrict__ amax, int pass, int bf16, int bx, int j) {
    // SH16 output (f16x3 LUT GEMM): first pass writes with `scale` and records max |mu * scale|; the second pass returns
    // at once unless that maximum left the f16 window, else rewrites with the corrected scale (sh16.h)
    sh16_mode_on();
    if (sh16 == 1 && amax && pass == 1) {
        const float e = sh16_dyn_extra(*amax);
        if (e == 1.f) return;
        scale *= e;
    }
    float vmax = 0.f;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int o0 = (bx * 4 + wave) * 4;                   // 4 output features per wave
    const float* Wj = Wt + (long long)j * 512 * 512;
    float4 w[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4* wr = reinterpret_cast<const float4*>(Wj + (long long)(o0 + i) * 512 + lane * 8);
        w[i][0] = wr[0];
        w[i][1] = wr[1];
    }
    for (int bb = 0; bb < B; bb += FCMU_BT) {
        float part[4][FCMU_BT];
#pragma unroll
        for (int t = 0; t < FCMU_BT; ++t) {
            float4 c0 = make_float4(0, 0, 0, 0), c1 = c0;
            if (bb + t < B) {
                const float4* cr =
                    reinterpret_cast<const float4*>(codes + ((long long)(bb + t) * 19 + j) * 512 + lane * 8);
                c0 = cr[0];
                c1 = cr[1];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                // the roundings of the eight-term sum spelled out (one product, seven fused multiply-adds in order: what hipcc made of the
                // plain sum before the reduction was templated; left to the compiler, the two instantiations contract different products first)
                float d = w[i][0].x * c0.x;
                d = __builtin_fmaf(w[i][0].y, c0.y, d);
                d = __builtin_fmaf(w[i][0].z, c0.z, d);
                d = __builtin_fmaf(w[i][0].w, c0.w, d);
                d = __builtin_fmaf(w[i][1].x, c1.x, d);
                d = __builtin_fmaf(w[i][1].y, c1.y, d);
                d = __builtin_fmaf(w[i][1].z, c1.z, d);
                part[i][t] = __builtin_fmaf(w[i][1].w, c1.w, d);
            }
        }
        // one result: feature o0 + i of sample bb + t, in all five output layouts
        auto emit = [&](int i, int t, float sum) {
            const float v = sum + bias[j * 512 + o0 + i];
            const float r = v > 0.f ? v : 0.f;
            const int o = o0 + i, n = (bb + t) * bs + j;      // bs = 19, or 20 with a zero column per sample
            if (bs > 19 && j == 0) {   // (re)write the zero column: the image pitch Npad changes with the batch
                const int nz = (bb + t) * bs + 19;
                if (mu_rows) mu_rows[(long long)nz * 512 + o] = 0.f;
                else if (sh16 == 1) {
                    _Float16* mh = reinterpret_cast<_Float16*>(mu_img);
                    mh[(((long long)(o >> 3) * 2 + 0) * Npad + nz) * 8 + (o & 7)] = (_Float16)0.f;
                    mh[(((long long)(o >> 3) * 2 + 1) * Npad + nz) * 8 + (o & 7)] = (_Float16)0.f;
                }
            }
            if (mu_rows) mu_rows[(long long)n * 512 + o] = r;   // [N][512] for the GEMV path
            else if (sh16 == 2)   // A-fragment order of the grouped LUT build (conv_pw.h pack_pw_A: row n, input channel o)
                mu_img[((long long)(n >> 5) * 32 + (o >> 4)) * 512 + ((n & 31) + 32 * (o & 1)) * 8 + ((o & 15) >> 1)] = r;
            else if (sh16) {   // split-operand image [512/8][hi|lo][Npad][8] for the f16x3 LUT GEMM
                _Float16* mh = reinterpret_cast<_Float16*>(mu_img);
                _Float16 h, l;
                sh16_split_any(r, scale, bf16, h, l);
                vmax = fmaxf(vmax, r * scale);
                mh[(((long long)(o >> 3) * 2 + 0) * Npad + n) * 8 + (o & 7)] = h;
                mh[(((long long)(o >> 3) * 2 + 1) * Npad + n) * 8 + (o & 7)] = l;
            } else mu_img[(long long)o * Npad + n] = r;
        };
        if constexpr (TR) {
            float q16[16], q8[8], q4[4], q2[2];
            const bool u5 = lane & 32, u4 = lane & 16, u3 = lane & 8, u2 = lane & 4, u1 = lane & 2;
#pragma unroll
            for (int v = 0; v < 16; ++v) {      // value v = 8 i + t
                const float lo = part[v >> 3][v & 7], hi = part[(v + 16) >> 3][v & 7];
                q16[v] = (u5 ? hi : lo) + __shfl_xor(u5 ? lo : hi, 32, 64);
            }
#pragma unroll
            for (int v = 0; v < 8; ++v) q8[v] = (u4 ? q16[v + 8] : q16[v]) + __shfl_xor(u4 ? q16[v] : q16[v + 8], 16, 64);
#pragma unroll
            for (int v = 0; v < 4; ++v) q4[v] = (u3 ? q8[v + 4] : q8[v]) + __shfl_xor(u3 ? q8[v] : q8[v + 4], 8, 64);
#pragma unroll
            for (int v = 0; v < 2; ++v) q2[v] = (u2 ? q4[v + 2] : q4[v]) + __shfl_xor(u2 ? q4[v] : q4[v + 2], 4, 64);
            float q1 = (u1 ? q2[1] : q2[0]) + __shfl_xor(u1 ? q2[0] : q2[1], 2, 64);
            q1 += __shfl_xor(q1, 1, 64);
            const int v = lane >> 1;
            if (!(lane & 1) && bb + (v & 7) < B) emit(v >> 3, v & 7, q1);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < FCMU_BT; ++t) {
                    float v = part[i][t];
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
                    part[i][t] = v;
                }
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int t = 0; t < FCMU_BT; ++t)
                        if (bb + t < B) emit(i, t, part[i][t]);
            }
        }
    }
    if constexpr (TR) {      // the results sit in the even lanes: their maximum, as lane 0 found it before
        if (sh16 == 1 && amax && pass == 0)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
    }
    if (sh16 == 1 && amax && pass == 0 && lane == 0) sh16_slot_max(amax, vmax);
}
template <bool TR>
__global__ __launch_bounds__(256) void fc_mu_kernel(const float* __restrict__ codes, const float* __restrict__ Wt,
                                                    const float* __restrict__ bias, float* __restrict__ mu_img, int B,
                                                    int Npad, float* __restrict__ mu_rows, int sh16, int bs, float scale,
                                                    unsigned* __restrict__ amax, int pass, int bf16) {
    fc_mu_body<TR>(codes, Wt, bias, mu_img, B, Npad, mu_rows, sh16, bs, scale, amax, pass, bf16, blockIdx.x, blockIdx.y);
}
// All styled ACE layers of the generator in ONE launch (blockIdx.z = ACE index; a null weight pointer = unstyled layer): 15
// launches of 608 blocks streaming 20 MB each ran at 0.9 TB/s, latency bound.  SH16 output into mu_base + a * mu_stride, slot
// 2a + 1 of amax_slots (sean_model.cpp); the second pass works as in fc_mu_kernel.
template <bool TR>
__global__ __launch_bounds__(256) void fc_mu_batched_kernel(const float* __restrict__ codes, const float* const* __restrict__ Wts,
                                                            const float* const* __restrict__ biases, float* __restrict__ mu_base,
                                                            long long mu_stride, int B, int Npad, int bs, float scale,
                                                            unsigned* __restrict__ amax_slots, int pass, int bf16, int sh16,
                                                            const int* __restrict__ skip) {
    if (skip && *skip) return;      // (code memo: mu_base still holds the projections of these codes)
    const int a = blockIdx.z;
    const float* Wt = Wts[a];
    if (!Wt) return;
    fc_mu_body<TR>(codes, Wt, biases[a], mu_base + a * mu_stride, B, Npad, nullptr, sh16, bs, scale, sh16 == 1 ? amax_slots + 2 * a + 1 : nullptr, pass,
               bf16, blockIdx.x, blockIdx.y);
}
// sh16 = 0: f32 images [512][Npad] (exact-f32 path; no scale protocol, one pass); sh16 = 2: f32 in the A-fragment order of conv_pw.h
hipError_t fc_mu_batched(const float* codes, const float* const* Wts, const float* const* biases, float* mu_base,
                         long long mu_stride, int n_aces, int B, int Npad, int bs, float scale, unsigned* amax_slots, int pass,
                         int bf16, hipStream_t s, int sh16, int transposed, const int* skip) {
    hipLaunchKernelGGL(transposed ? fc_mu_batched_kernel<true> : fc_mu_batched_kernel<false>, dim3(512 / 16, 19, n_aces), dim3(256), 0, s, codes, Wts, biases, mu_base, mu_stride, B,
                       Npad, bs, scale, amax_slots, pass, bf16, sh16, skip);
    return hipGetLastError();
}

hipError_t fc_mu(const float* codes, const float* Wt, const float* bias, float* mu_img, int B, int Npad,
                 hipStream_t s, float* mu_rows, int sh16, int bs, float scale, unsigned* amax, int pass, int bf16, int transposed) {
    hipLaunchKernelGGL(transposed ? fc_mu_kernel<true> : fc_mu_kernel<false>, dim3(512 / 16, 19), dim3(256), 0, s, codes, Wt, bias, mu_img, B, Npad, mu_rows, sh16, bs,
                       scale, amax, pass, bf16);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// conv_img(leaky_relu(x, 0.2)) then tanh (generator.py:107-108): Cin -> 3, 3x3, zero pad.  Three output rows
// are far too few for the matrix cores; this is a direct VALU conv, 32x8 pixel tile, input staged through LDS
// in chunks of 8 channels with the leaky_relu applied on the way in.
constexpr int CI_TW = 32, CI_TH = 8, CI_CK = 8;

__global__ __launch_bounds__(256) void conv_img_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out, int B,
                                                       int Cin, int H, int W, int c4) {
    __shared__ float patch[CI_CK][CI_TH + 2][CI_TW + 2];
    const int tx = threadIdx.x % CI_TW, ty = threadIdx.x / CI_TW;
    const int x0 = blockIdx.x * CI_TW, y0 = blockIdx.y * CI_TH, b = blockIdx.z;
    const long long HW = (long long)H * W;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int c0 = 0; c0 < Cin; c0 += CI_CK) {
        __syncthreads();
        for (int e = threadIdx.x; e < CI_CK * (CI_TH + 2) * (CI_TW + 2); e += 256) {
            const int c = e / ((CI_TH + 2) * (CI_TW + 2)), rem = e % ((CI_TH + 2) * (CI_TW + 2));
            const int py = rem / (CI_TW + 2), px = rem % (CI_TW + 2);
            const int yy = y0 + py - 1, xx = x0 + px - 1;
            float v = 0.f;
            if (c0 + c < Cin && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) {
                const int ch = c0 + c;
                v = c4 ? x[(((long long)b * (Cin >> 2) + (ch >> 2)) * HW + (long long)yy * W + xx) * 4 + (ch & 3)]
                       : x[((long long)b * Cin + ch) * HW + (long long)yy * W + xx];
                v = v > 0.f ? v : 0.2f * v;
            }
            patch[c][py][px] = v;
        }
        __syncthreads();
        // weights: wave-uniform addresses -> scalar loads, SGPR operands of the FMAs (as LDS broadcasts they were 3 of the 4
        // LDS reads per tap and made the kernel LDS-issue bound); Cin % CI_CK == 0 or the tail channels hold zeros in `patch`
        const float* w0 = w + (long long)c0 * 9;
#pragma unroll
        for (int c = 0; c < CI_CK; ++c) {
            if (c0 + c >= Cin) break;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const float v = patch[c][ty + t / 3][tx + t % 3];
                a0 += w0[c * 9 + t] * v;
                a1 += w0[(long long)Cin * 9 + c * 9 + t] * v;
                a2 += w0[(long long)Cin * 18 + c * 9 + t] * v;
            }
        }
    }
    const int xx = x0 + tx, yy = y0 + ty;
    if (xx < W && yy < H) {
        float* o = out + (long long)b * 3 * HW + (long long)yy * W + xx;
        o[0] = tanhf(a0 + bias[0]);
        o[HW] = tanhf(a1 + bias[1]);
        o[2 * HW] = tanhf(a2 + bias[2]);
    }
}

// Same op for the C4 activation layout [B][Cin/4][H][W][4] (f16x3 path): one float4 = 4 channels of a pixel, so the
// staging loads are 16 B per lane and every LDS read feeds 12 FMAs.  Channel groups are double-buffered in LDS with the
// next group's loads in flight during the current group's FMAs; the weights, packed on the host as [group][tap][co] float4
// (w4), arrive through wave-uniform scalar loads and enter the FMAs as SGPR operands (as LDS broadcasts they took 27 of the
// 36 LDS reads per group and made the kernel LDS-issue bound).  HBM-read bound: x is read once (+ halo).
// NCHW = true: the same kernel over the planar f32 layout of the exact-f32 path -- a thread gathers the four channels of its patch
// elements from four planes (dword loads, coalesced along x) into the float4 the compute loop reads (the planar kernel below it
// replaces spent 72 ds_read_b32 per 216 FMAs: 0.62 ms at B = 16, 512^2, LDS-issue bound).
template <bool NCHW>
__global__ __launch_bounds__(256) void conv_img_c4_kernel(const float4* __restrict__ x, const float4* __restrict__ w4,
                                                          const float* __restrict__ bias, float* __restrict__ out, int B,
                                                          int Cin, int H, int W) {
    constexpr int PW = CI_TW + 2, PH = CI_TH + 2, NP = PW * PH;
    __shared__ float4 patch[2][NP];
    const int G = Cin >> 2;
    const int tx = threadIdx.x % CI_TW, ty = threadIdx.x / CI_TW;
    const int x0 = blockIdx.x * CI_TW, y0 = blockIdx.y * CI_TH, b = blockIdx.z;
    const long long HW = (long long)H * W;
    int off[2];                       // this thread's (up to) two patch elements: pixel offset or -1 (outside / none)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = threadIdx.x + i * 256;
        const int py = e / PW, px = e % PW, yy = y0 + py - 1, xx = x0 + px - 1;
        off[i] = (e < NP && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? yy * W + xx : -1;
    }
    const float4* xb = x + (long long)b * G * HW;
    const float* xp = reinterpret_cast<const float*>(x) + (long long)b * Cin * HW;      // NCHW view of the same pointer
    float4 r[2];
    auto fetch = [&](int g) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float4 v;
            if constexpr (NCHW) {
                const float* q = xp + (long long)(4 * g) * HW + (off[i] >= 0 ? off[i] : 0);
                v = make_float4(q[0], q[HW], q[2 * HW], q[3 * HW]);
            } else {
                v = xb[(long long)g * HW + (off[i] >= 0 ? off[i] : 0)];
            }
            r[i] = off[i] >= 0 ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stash = [&](int st) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = threadIdx.x + i * 256;
            if (e < NP) {
                float4 v = r[i];
                v.x = fmaxf(v.x, 0.2f * v.x); v.y = fmaxf(v.y, 0.2f * v.y);
                v.z = fmaxf(v.z, 0.2f * v.z); v.w = fmaxf(v.w, 0.2f * v.w);
                patch[st][e] = v;
            }
        }
    };
    fetch(0);
    stash(0);
    __syncthreads();
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int g = 0; g < G; ++g) {
        if (g + 1 < G) fetch(g + 1);
        const float4* pp = patch[g & 1] + ty * PW + tx;
        const float4* wg = w4 + g * 27;                  // wave-uniform: scalar loads
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float4 v = pp[(t / 3) * PW + t % 3];
            const float4 w0 = wg[t * 3 + 0], w1 = wg[t * 3 + 1], w2 = wg[t * 3 + 2];
            a0 += w0.x * v.x + w0.y * v.y + w0.z * v.z + w0.w * v.w;
            a1 += w1.x * v.x + w1.y * v.y + w1.z * v.z + w1.w * v.w;
            a2 += w2.x * v.x + w2.y * v.y + w2.z * v.z + w2.w * v.w;
        }
        if (g + 1 < G) stash((g + 1) & 1);
        __syncthreads();
    }
    const int xx = x0 + tx, yy = y0 + ty;
    if (xx < W && yy < H) {
        float* o = out + (long long)b * 3 * HW + (long long)yy * W + xx;
        o[0] = tanhf(a0 + bias[0]);
        o[HW] = tanhf(a1 + bias[1]);
        o[2 * HW] = tanhf(a2 + bias[2]);
    }
}

hipError_t conv_img_tanh(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W,
                         hipStream_t s, int c4, const float* w4) {
    dim3 grid((W + CI_TW - 1) / CI_TW, (H + CI_TH - 1) / CI_TH, B);
    if (c4 && w4 && Cin % 4 == 0) {
        hipLaunchKernelGGL(conv_img_c4_kernel<false>, grid, dim3(256), 0, s, reinterpret_cast<const float4*>(x),
                           reinterpret_cast<const float4*>(w4), bias, out, B, Cin, H, W);
        return hipGetLastError();
    }
    if (!c4 && w4 && Cin % 4 == 0) {
        hipLaunchKernelGGL(conv_img_c4_kernel<true>, grid, dim3(256), 0, s, reinterpret_cast<const float4*>(x),
                           reinterpret_cast<const float4*>(w4), bias, out, B, Cin, H, W);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(conv_img_kernel, grid, dim3(256), 0, s, x, w, bias, out, B, Cin, H, W, c4);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------
// Device noise (used only when the caller passes noise == NULL): counter-based, one N(0,1) per element via a
// 64-bit mix (splitmix64) + Box-Muller.  The reference draws torch.randn (normalization.py:111) from an
// unseeded global generator, so there is nothing to be bit-compatible with; parity tests pass explicit planes.
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void noise_kernel(float* __restrict__ out, long long n, uint64_t seed) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const uint64_t h = mix64(seed ^ mix64((uint64_t)i));
        const float u1 = ((uint32_t)(h >> 40) + 1) * (1.0f / 16777217.0f);        // (0,1]
        const float u2 = (uint32_t)((h >> 8) & 0xFFFFFF) * (1.0f / 16777216.0f);  // [0,1)
        out[i] = sqrtf(-2.f * __logf(u1)) * __cosf(6.28318530718f * u2);
    }
}

hipError_t gen_noise(float* out, long long n, uint64_t seed, hipStream_t s) {
    hipLaunchKernelGGL(noise_kernel, dim3(2048), dim3(256), 0, s, out, n, seed);
    return hipGetLastError();
}

}  // namespace chk
