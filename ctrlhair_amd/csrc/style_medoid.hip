// style_medoid.hip -- per-region medoid and mean of style codes (sean_codes/get_mean_code.py) for R segments in one call.
//   medoid_pairs_kernel    all-pairs Euclidean distances of one segment, tiled; the n x n matrix is never stored.  A block owns a
//                          128-row tile and a range of 128-column tiles; K slabs of both tiles go through LDS, a lane owns 8 x 8 pairs.
//   medoid_finish_kernel   combines the column-range partials in ascending order, writes the row sums, picks the first minimum
//   medoid_mean_kernel     float64 column means
// Arithmetic contract (include/ctrlhair_hip.h): d_ij^2 = sum_k (x_ik - x_jk)^2 in float32, difference before squaring (so d_ii is
// exactly 0 and saturated codes do not cancel, unlike the reference's Gram identity), d_ij = sqrtf, S_i = sum_j d_ij in float64.
// No floating-point atomics and fixed reduction trees: a segment's sums depend on its own rows and its split count only.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <vector>

#include "kernels.h"

namespace chk {

namespace {
typedef float v2f __attribute__((ext_vector_type(2)));
constexpr int MD_TILE = 128;              // rows / columns of a block's tile
constexpr int MD_KS = 16;                 // K slab
constexpr int MD_LD = MD_TILE + 4;        // LDS row pitch in floats: the transposing stores of a wave conflict 2-way at most
constexpr int MD_THREADS = 256;
constexpr int MD_KUNROLL = 4;             // k steps unrolled: 16 ds_read_b128 in flight, 159 VGPRs, 3 waves per SIMD
constexpr int MD_SPLIT_BLOCKS = 1024;     // auto split: about this many blocks for one segment (a function of n alone)

struct MedoidSeg {                        // one segment, in the workspace
    long long row_off;                    // first row in codes
    long long part_off;                   // first double of its partials [n_split][n]
    int n, n_split, tiles, block0;        // rows, column ranges, ceil(n / MD_TILE), first block of the pairs kernel
};

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

inline int split_for(long long n, int n_split) {
    const long long tiles = (n + MD_TILE - 1) / MD_TILE;
    if (tiles < 1) return 1;
    long long ns = n_split > 0 ? n_split : (MD_SPLIT_BLOCKS + tiles - 1) / tiles;
    return (int)(ns < 1 ? 1 : (ns > tiles ? tiles : ns));
}

// global -> registers: this thread's float4 of the slab (row t / 4, k quarter t % 4) of two 64-row halves of a 128-row tile; rows
// >= n and k >= dim read as zero (a zero difference adds exactly nothing to a pair's sum; such rows are masked from the results)
__device__ __forceinline__ void load_slab(const float* __restrict__ x, int n, int dim, int row0, int k0, float4 (&r)[2]) {
    const int t = threadIdx.x, k = k0 + (t & 3) * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int row = row0 + (t >> 2) + 64 * h;
        r[h] = (row < n && k < dim) ? *reinterpret_cast<const float4*>(x + (size_t)row * dim + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// registers -> LDS, transposed to [k][row]
__device__ __forceinline__ void store_slab(float* __restrict__ s, const float4 (&r)[2]) {
    const int t = threadIdx.x, kq = (t & 3) * 4;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        float* p = s + kq * MD_LD + (t >> 2) + 64 * h;
        p[0] = r[h].x;
        p[MD_LD] = r[h].y;
        p[2 * MD_LD] = r[h].z;
        p[3 * MD_LD] = r[h].w;
    }
}
}  // namespace

__global__ __launch_bounds__(MD_THREADS, 3) void medoid_pairs_kernel(const float* __restrict__ codes, const MedoidSeg* __restrict__ segs, int R,
                                                                  int dim, double* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[2][MD_KS * MD_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][MD_KS * MD_LD];
    // the segment of this block: the last one whose block0 <= blockIdx.x (empty segments own no block)
    int lo = 0, hi = R - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].block0 <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const MedoidSeg sg = segs[lo];
    const int local = (int)blockIdx.x - sg.block0;
    const int rt = local / sg.n_split, sp = local - rt * sg.n_split;
    const int n = sg.n, row0 = rt * MD_TILE;
    const int ct0 = (int)((long long)sp * sg.tiles / sg.n_split), ct1 = (int)((long long)(sp + 1) * sg.tiles / sg.n_split);
    const float* __restrict__ x = codes + (size_t)sg.row_off * dim;
    const int nslab = (dim + MD_KS - 1) / MD_KS;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;       // the lane's pairs: rows ty*4 + {0..3, 64..67}, columns tx*4 + {0..3, 64..67}

    double rowsum[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) rowsum[i] = 0.0;

    float4 ra[2], rb[2];
    load_slab(x, n, dim, row0, 0, ra);
    load_slab(x, n, dim, ct0 * MD_TILE, 0, rb);
    store_slab(As[0], ra);
    store_slab(Bs[0], rb);
    __syncthreads();

    int buf = 0;
    for (int ct = ct0; ct < ct1; ++ct) {                          // column tiles in ascending order
        // pairs of adjacent columns as 2-vectors: v_pk_add_f32 (the row operand broadcast by op_sel, the column pair negated) and
        // v_pk_fma_f32.  Measured against the scalar v_sub_f32 / v_fma_f32 form: 20.1 ms against 24.0 ms for one 30 000-row segment
        v2f acc[8][4];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = v2f{0.f, 0.f};
        for (int sl = 0; sl < nslab; ++sl) {
            // the next slab (of this column tile or the first of the next one) travels to registers underneath the arithmetic
            const bool last_slab = sl + 1 == nslab;
            const int nct = last_slab ? ct + 1 : ct, nk = last_slab ? 0 : (sl + 1) * MD_KS;
            const bool more = nct < ct1;
            if (more) {
                load_slab(x, n, dim, row0, nk, ra);
                load_slab(x, n, dim, nct * MD_TILE, nk, rb);
            }
            const float* __restrict__ a_s = As[buf] + ty * 4;
            const float* __restrict__ b_s = Bs[buf] + tx * 4;
#pragma unroll MD_KUNROLL
            for (int k = 0; k < MD_KS; ++k) {
                const float4 a0 = *reinterpret_cast<const float4*>(a_s + k * MD_LD), a1 = *reinterpret_cast<const float4*>(a_s + k * MD_LD + 64);
                const float4 b0 = *reinterpret_cast<const float4*>(b_s + k * MD_LD), b1 = *reinterpret_cast<const float4*>(b_s + k * MD_LD + 64);
                const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const v2f b[4] = {v2f{b0.x, b0.y}, v2f{b0.z, b0.w}, v2f{b1.x, b1.y}, v2f{b1.z, b1.w}};
#pragma unroll
                for (int i = 0; i < 8; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const v2f d = v2f{a[i], a[i]} - b[j];
                        acc[i][j] = __builtin_elementwise_fma(d, d, acc[i][j]);
                    }
            }
            if (more) {
                store_slab(As[buf ^ 1], ra);
                store_slab(Bs[buf ^ 1], rb);
            }
            __syncthreads();           // the other buffer was last read one slab ago: every wave is past that
            buf ^= 1;
        }
        // this column tile's share of the row sums: sqrt, columns past n masked, the lane's 8 columns in ascending order, then a fixed
        // butterfly over the 16 lanes that share the rows
        const int col0 = ct * MD_TILE + tx * 4;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int col = col0 + (j & 3) + 64 * (j >> 2);
                s += col < n ? (double)sqrtf(acc[i][j >> 1][j & 1]) : 0.0;
            }
#pragma unroll
            for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            rowsum[i] += s;
        }
    }
    if (tx == 0) {
        double* __restrict__ p = part + sg.part_off + (size_t)sp * n;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = row0 + ty * 4 + (i & 3) + 64 * (i >> 2);
            if (row < n) p[row] = rowsum[i];
        }
    }
}

// one block per segment: S_i = partials in ascending split order; the first index of the smallest S_i (numpy argmin)
__global__ __launch_bounds__(1024) void medoid_finish_kernel(const MedoidSeg* __restrict__ segs, const double* __restrict__ part,
                                                             double* __restrict__ sums, int* __restrict__ index) {
    __shared__ double bv[16];
    __shared__ int bi[16];
    const MedoidSeg sg = segs[blockIdx.x];
    const int n = sg.n;
    if (n == 0) {
        if (threadIdx.x == 0) index[blockIdx.x] = -1;
        return;
    }
    const double* __restrict__ p = part + sg.part_off;
    double best = 0.0;
    int arg = -1;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {           // ascending i: a strict < keeps the first minimum
        double s = p[i];
        for (int k = 1; k < sg.n_split; ++k) s += p[(size_t)k * n + i];
        if (sums) sums[sg.row_off + i] = s;
        if (arg < 0 || s < best) best = s, arg = i;
    }
    auto take = [&](double v, int a) {
        if (a >= 0 && (arg < 0 || v < best || (v == best && a < arg))) best = v, arg = a;
    };
    for (int off = 32; off > 0; off >>= 1) take(__shfl_xor(best, off, 64), __shfl_xor(arg, off, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) bv[wave] = best, bi[wave] = arg;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int w = 1; w < nw; ++w) take(bv[w], bi[w]);
        index[blockIdx.x] = arg;
    }
}

// block (segment, 64 columns): 16 row lanes stride the rows, float64 sums combined in lane order, rounded once
__global__ __launch_bounds__(1024) void medoid_mean_kernel(const float* __restrict__ codes, const MedoidSeg* __restrict__ segs, int dim,
                                                           float* __restrict__ mean) {
    __shared__ double acc[16][64];
    const MedoidSeg sg = segs[blockIdx.x];
    const int c = threadIdx.x & 63, rl = threadIdx.x >> 6, col = blockIdx.y * 64 + c;
    double s = 0.0;
    if (col < dim) {
        const float* __restrict__ x = codes + (size_t)sg.row_off * dim + col;
        for (int i = rl; i < sg.n; i += 16) s += (double)x[(size_t)i * dim];
    }
    acc[rl][c] = s;
    __syncthreads();
    if (rl == 0 && col < dim) {
        for (int k = 1; k < 16; ++k) s += acc[k][c];
        mean[(size_t)blockIdx.x * dim + col] = sg.n > 0 ? (float)(s / (double)sg.n) : 0.f;
    }
}

size_t style_medoid_workspace_bytes(const int64_t* seg_offsets, int R, int n_split) {
    size_t doubles = 0;
    for (int r = 0; r < R; ++r) {
        const long long n = seg_offsets[r + 1] - seg_offsets[r];
        doubles += (size_t)n * split_for(n, n_split);
    }
    return up256(sizeof(MedoidSeg) * (size_t)R) + up256(doubles * sizeof(double));
}

hipError_t style_medoid(const float* codes, const int64_t* seg_offsets, int R, int dim, int n_split, int* index, double* sums, float* mean,
                        void* ws, hipStream_t s) {
    std::vector<MedoidSeg> segs((size_t)R);
    long long part_off = 0, blocks = 0;
    for (int r = 0; r < R; ++r) {
        const long long n = seg_offsets[r + 1] - seg_offsets[r];
        MedoidSeg& g = segs[(size_t)r];
        g.row_off = seg_offsets[r];
        g.part_off = part_off;
        g.n = (int)n;
        g.n_split = split_for(n, n_split);
        g.tiles = (int)((n + MD_TILE - 1) / MD_TILE);
        g.block0 = (int)blocks;
        part_off += n * g.n_split;
        blocks += (long long)g.tiles * g.n_split;
    }
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    MedoidSeg* dsegs = reinterpret_cast<MedoidSeg*>(ws);
    double* part = reinterpret_cast<double*>(static_cast<char*>(ws) + up256(sizeof(MedoidSeg) * (size_t)R));
    hipError_t e = hipMemcpyAsync(dsegs, segs.data(), sizeof(MedoidSeg) * (size_t)R, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    if (blocks > 0) hipLaunchKernelGGL(medoid_pairs_kernel, dim3((unsigned)blocks), dim3(MD_THREADS), 0, s, codes, dsegs, R, dim, part);
    hipLaunchKernelGGL(medoid_finish_kernel, dim3(R), dim3(1024), 0, s, dsegs, part, sums, index);
    hipLaunchKernelGGL(medoid_mean_kernel, dim3(R, (dim + 63) / 64), dim3(1024), 0, s, codes, dsegs, dim, mean);
    return hipGetLastError();
}

}  // namespace chk
