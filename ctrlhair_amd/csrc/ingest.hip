// ingest.hip -- decoded uint8 images -> network inputs, for a RAGGED batch (every image has its own size) in a fixed number of launches:
//   ingest_images   mode 0: Pillow's Image.resize((P, P), BILINEAR) of 8-bit data (ImagingResample: antialiased, 22-bit coefficient
//                   tables built on the host, horizontal pass into a uint8 intermediate, then the vertical pass); mode 1: cv2's two-tap
//                   INTER_LINEAR (linear_tap.h, the arithmetic of resize_linear_u8).  Either way the resized byte indexes a float table
//                   [3][256] and lands in planar float32 [N,3,P,P]: the table holds whatever normalisation the caller evaluated once.
//   ingest_labels   hostutil.resize_nearest of uint8 label maps into uint8 [N,S,S]
// Integer accumulation only, no atomics, no workgroup waits on another; the image index is a grid dimension, so image n of a batch is
// computed exactly as in a call of its own.  The batch (descriptors, then coefficient tables; include/ctrlhair_hip.h) is checked on the
// host entry by entry before anything is launched, and the kernels clamp what they read from it by the descriptor's own H and W again.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "ingest_batch.h"
#include "kernels.h"
#include "launch.h"
#include "linear_tap.h"

namespace chk {

namespace {

constexpr int BLK = 256;
constexpr int PRECISION_BITS = 22;           // Pillow: 32 - 8 - 2
constexpr int H_ROWS = 8;                    // most source rows one workgroup of the horizontal pass filters
constexpr int H_LDS_TARGET = 24576;          // bytes of source rows it stages while a row is narrower than that
constexpr int H_LDS_MAX = INGEST_MAX_SIDE * 3 + 16;

inline size_t up256(size_t v) { return ingest_up256(v); }

// source rows per workgroup of the horizontal pass: as many as fit the target, one when a single row is wider
__host__ __device__ inline int h_rows(int W) {
    const int r = H_LDS_TARGET / (W * 3);
    return r < 1 ? 1 : (r > H_ROWS ? H_ROWS : r);
}

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= PRECISION_BITS;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// ---- mode 0, horizontal pass ------------------------------------------------------------------------------------------------------
// One workgroup per (image, run of R = h_rows(W) source rows).  The rows are one contiguous span of the image: it goes to LDS with
// 16-byte loads between its own first and last byte (bytes before the first 16-byte boundary and after the last one singly), at the
// same misalignment, so nothing outside the span is read.  A thread owns an output column: bounds and each coefficient (table stored
// [ksize][P]: adjacent lanes, adjacent words) are read once and serve all R rows.
__global__ __launch_bounds__(BLK) void ingest_h_kernel(const IngestImage* __restrict__ desc, const int32_t* __restrict__ batch,
                                                       uint8_t* __restrict__ inter, int P) {
    extern __shared__ __align__(16) uint8_t lds[];
    const IngestImage d = desc[blockIdx.y];
    if (d.htab < 0) return;                                   // W == P: the vertical pass reads the image itself
    const int R0 = h_rows(d.W), r0 = blockIdx.x * R0;
    if (r0 >= d.H) return;
    const int R = min(R0, d.H - r0), rowb = d.W * 3, total = R * rowb;
    const uint8_t* g = reinterpret_cast<const uint8_t*>(d.src) + (size_t)r0 * rowb;
    const int mis = (int)(reinterpret_cast<uintptr_t>(g) & 15);
    const int head = mis ? min(16 - mis, total) : 0;
    const int nvec = (total - head) >> 4;
    for (int i = threadIdx.x; i < head; i += BLK) lds[mis + i] = g[i];
    const uint4* gv = reinterpret_cast<const uint4*>(g + head);
    uint4* lv = reinterpret_cast<uint4*>(lds + mis + head);
    for (int i = threadIdx.x; i < nvec; i += BLK) lv[i] = gv[i];
    for (int i = head + (nvec << 4) + threadIdx.x; i < total; i += BLK) lds[mis + i] = g[i];
    __syncthreads();

    const int32_t* tab = batch + d.htab;                      // {in, out, ksize, layout} | bounds [P][2] | k [ksize][P]
    const int ksize = tab[2];
    const int32_t* bounds = tab + 4;
    const int32_t* kt = bounds + 2 * P;
    const uint8_t* rows = lds + mis;
    uint8_t* out = inter + d.inter + (size_t)r0 * P * 3;
    for (int x = threadIdx.x; x < P; x += BLK) {
        int xmin = bounds[2 * x], cnt = bounds[2 * x + 1];
        xmin = xmin < 0 ? 0 : (xmin > d.W ? d.W : xmin);
        cnt = min(cnt, min(ksize, d.W - xmin));
        int acc[H_ROWS][3];
#pragma unroll
        for (int r = 0; r < H_ROWS; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 1 << (PRECISION_BITS - 1);
        const uint8_t* p = rows + xmin * 3;
        for (int k = 0; k < cnt; ++k, p += 3) {
            const int c = kt[(size_t)k * P + x];
#pragma unroll
            for (int r = 0; r < H_ROWS; ++r)
                if (r < R) {
                    acc[r][0] += c * p[r * rowb];
                    acc[r][1] += c * p[r * rowb + 1];
                    acc[r][2] += c * p[r * rowb + 2];
                }
        }
#pragma unroll
        for (int r = 0; r < H_ROWS; ++r)
            if (r < R) {
                uint8_t* o = out + ((size_t)r * P + x) * 3;
                o[0] = clip8(acc[r][0]);
                o[1] = clip8(acc[r][1]);
                o[2] = clip8(acc[r][2]);
            }
    }
}

// ---- the shared tail: PX pixels of one output row -> table -> three planes -----------------------------------------------------------
// PX * 3 bytes at p.  PX == 4 and p 4-byte aligned: three dwords (the caller guarantees 12 readable bytes: x + 4 <= row length)
template <int PX>
__device__ __forceinline__ void load_px(const uint8_t* p, bool aligned, int (&b)[PX * 3]) {
    if (PX == 4 && aligned) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const uint32_t v = q[j];
            b[4 * j] = v & 255, b[4 * j + 1] = (v >> 8) & 255, b[4 * j + 2] = (v >> 16) & 255, b[4 * j + 3] = v >> 24;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PX * 3; ++j) b[j] = p[j];
    }
}

// v: PX pixels x 3 channels of resized bytes -> out[n][c][y][x .. x + PX) = tl[c][byte]; PX == 4: one 16-byte store per plane
template <int PX>
__device__ __forceinline__ void store_px(const float* tl, const int (&v)[PX * 3], float* __restrict__ out, int n, int y, int x, int P) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float* o = out + (((size_t)n * 3 + c) * P + y) * P + x;
        if (PX == 4) {
            *reinterpret_cast<float4*>(o) = make_float4(tl[c * 256 + v[c]], tl[c * 256 + v[3 + c]], tl[c * 256 + v[6 + c]], tl[c * 256 + v[9 + c]]);
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j) o[j] = tl[c * 256 + v[j * 3 + c]];
        }
    }
}

// ---- mode 0, vertical pass + table ----------------------------------------------------------------------------------------------------
// Lanes run along x, PX pixels each (PX == 4 only when P % 4 == 0, so a lane's pixels never straddle a row end); a workgroup covers BLK
// consecutive lanes of the image's P rows.  The row's coefficients (table stored [P][ksize]) are the same words for a whole row.
template <int PX>
__global__ __launch_bounds__(BLK) void ingest_v_kernel(const IngestImage* __restrict__ desc, const int32_t* __restrict__ batch,
                                                       const uint8_t* __restrict__ inter, const float* __restrict__ lut,
                                                       float* __restrict__ out, int P) {
    __shared__ float tl[768];
    for (int i = threadIdx.x; i < 768; i += BLK) tl[i] = lut[i];
    __syncthreads();
    const int n = blockIdx.y;
    const IngestImage d = desc[n];
    const int lanes = (P + PX - 1) / PX;
    const int item = blockIdx.x * BLK + threadIdx.x, y = item / lanes, x = (item - y * lanes) * PX;
    if (y >= P) return;
    // the horizontal pass wrote [H][P][3] into the workspace; without one the image is [H][P][3] itself
    const uint8_t* src = d.htab >= 0 ? inter + d.inter : reinterpret_cast<const uint8_t*>(d.src);
    const bool aligned = (reinterpret_cast<uintptr_t>(src) & 3) == 0;
    const size_t stride = (size_t)P * 3;
    int v[PX * 3];
    if (d.vtab < 0) {                                         // H == P: no vertical pass, the row itself
        load_px<PX>(src + (size_t)y * stride + x * 3, aligned, v);
    } else {
        const int32_t* tab = batch + d.vtab;                  // {in, out, ksize, layout} | bounds [P][2] | k [P][ksize]
        const int ksize = tab[2];
        int ymin = tab[4 + 2 * y], cnt = tab[4 + 2 * y + 1];
        ymin = ymin < 0 ? 0 : (ymin > d.H ? d.H : ymin);
        cnt = min(cnt, min(ksize, d.H - ymin));
        const int32_t* kk = tab + 4 + 2 * P + (size_t)y * ksize;
        int acc[PX * 3];
#pragma unroll
        for (int j = 0; j < PX * 3; ++j) acc[j] = 1 << (PRECISION_BITS - 1);
        const uint8_t* p = src + (size_t)ymin * stride + x * 3;
        for (int k = 0; k < cnt; ++k, p += stride) {
            const int c = kk[k];
            int b[PX * 3];
            load_px<PX>(p, aligned, b);
#pragma unroll
            for (int j = 0; j < PX * 3; ++j) acc[j] += c * b[j];
        }
#pragma unroll
        for (int j = 0; j < PX * 3; ++j) v[j] = clip8(acc[j]);
    }
    store_px<PX>(tl, v, out, n, y, x, P);
}

// ---- mode 1: cv2.resize(INTER_LINEAR), the arithmetic of resize_linear_u8_kernel, + table --------------------------------------------
template <int PX>
__global__ __launch_bounds__(BLK) void ingest_cv2_kernel(const IngestImage* __restrict__ desc, const float* __restrict__ lut,
                                                         float* __restrict__ out, int P) {
    __shared__ float tl[768];
    for (int i = threadIdx.x; i < 768; i += BLK) tl[i] = lut[i];
    __syncthreads();
    const int n = blockIdx.y;
    const IngestImage d = desc[n];
    const int lanes = (P + PX - 1) / PX;
    const int item = blockIdx.x * BLK + threadIdx.x, y = item / lanes, x = (item - y * lanes) * PX;
    if (y >= P) return;
    int y0, y1, b0, b1;
    linear_tap(y, P, d.H, y0, y1, b0, b1);
    const uint8_t* s = reinterpret_cast<const uint8_t*>(d.src);
    const uint8_t* r0 = s + (size_t)y0 * d.W * 3;
    const uint8_t* r1 = s + (size_t)y1 * d.W * 3;
    int v[PX * 3];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        int x0, x1, a0, a1;
        linear_tap(x + j, P, d.W, x0, x1, a0, a1);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int top = (r0[x0 * 3 + c] * a0 + r0[x1 * 3 + c] * a1) >> 4;
            const int bot = (r1[x0 * 3 + c] * a0 + r1[x1 * 3 + c] * a1) >> 4;
            const int q = (((b0 * top) >> 16) + ((b1 * bot) >> 16) + 2) >> 2;
            v[j * 3 + c] = q < 0 ? 0 : (q > 255 ? 255 : q);
        }
    }
    store_px<PX>(tl, v, out, n, y, x, P);
}

// ---- labels: hostutil.resize_nearest, src = min((int)(dst * (in / out)), in - 1), the ratio in double ----------------------------------
__global__ __launch_bounds__(BLK) void ingest_labels_kernel(const IngestImage* __restrict__ desc, uint8_t* __restrict__ out, int S) {
    const int x = blockIdx.x * BLK + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
    if (x >= S) return;
    const IngestImage d = desc[n];
    const double sy = (double)d.H / (double)S, sx = (double)d.W / (double)S;
    int ly = (int)(y * sy), lx = (int)(x * sx);
    ly = ly < d.H - 1 ? ly : d.H - 1;
    lx = lx < d.W - 1 ? lx : d.W - 1;
    out[((size_t)n * S + y) * S + x] = reinterpret_cast<const uint8_t*>(d.src)[(size_t)ly * d.W + lx];
}

// the device copy of the batch sits at the start of the workspace, the intermediates behind it
const IngestImage* upload(const void* batch_host, size_t bytes, void* ws, hipStream_t s, hipError_t& e) {
    e = hipMemcpyAsync(ws, batch_host, bytes, hipMemcpyHostToDevice, s);
    return static_cast<const IngestImage*>(ws);
}

}  // namespace

hipError_t ingest_images(const void* batch, size_t batch_bytes, int N, int P, int mode, const float* lut, float* out, void* ws,
                         hipStream_t s) {
    // the library's part of the descriptors: where each image's intermediate starts
    std::vector<char> host(static_cast<const char*>(batch), static_cast<const char*>(batch) + batch_bytes);
    IngestImage* d = reinterpret_cast<IngestImage*>(host.data());
    size_t cur = 0;
    int h_blocks = 0, h_lds = 0;
    for (int n = 0; n < N; ++n) {
        d[n].inter = (int64_t)cur;
        if (d[n].htab < 0) continue;
        cur += up256((size_t)d[n].H * P * 3);
        const int R = h_rows(d[n].W);
        h_blocks = std::max(h_blocks, (d[n].H + R - 1) / R);
        h_lds = std::max(h_lds, R * d[n].W * 3 + 16);
    }
    hipError_t e;
    const IngestImage* desc = upload(host.data(), batch_bytes, ws, s, e);
    if (e != hipSuccess) return e;
    const int32_t* b32 = static_cast<const int32_t*>(ws);
    uint8_t* inter = static_cast<uint8_t*>(ws) + up256(batch_bytes);
    const bool vec = P % 4 == 0;
    const unsigned blocks = (unsigned)(((size_t)P * (vec ? P / 4 : P) + BLK - 1) / BLK);
    if (mode == INGEST_CV2) {
        if (vec) ingest_cv2_kernel<4><<<dim3(blocks, N), BLK, 0, s>>>(desc, lut, out, P);
        else ingest_cv2_kernel<1><<<dim3(blocks, N), BLK, 0, s>>>(desc, lut, out, P);
        return hipGetLastError();
    }
    if (h_blocks) {
        e = dyn_lds<ingest_h_kernel>(H_LDS_MAX);
        if (e != hipSuccess) return e;
        ingest_h_kernel<<<dim3(h_blocks, N), BLK, h_lds, s>>>(desc, b32, inter, P);
    }
    if (vec) ingest_v_kernel<4><<<dim3(blocks, N), BLK, 0, s>>>(desc, b32, inter, lut, out, P);
    else ingest_v_kernel<1><<<dim3(blocks, N), BLK, 0, s>>>(desc, b32, inter, lut, out, P);
    return hipGetLastError();
}

hipError_t ingest_labels(const void* batch, size_t batch_bytes, int N, int S, uint8_t* out, void* ws, hipStream_t s) {
    hipError_t e;
    const IngestImage* desc = upload(batch, batch_bytes, ws, s, e);
    if (e != hipSuccess) return e;
    ingest_labels_kernel<<<dim3((S + BLK - 1) / BLK, S, N), BLK, 0, s>>>(desc, out, S);
    return hipGetLastError();
}

}  // namespace chk
