// orient.hip -- EXIF orientations 1..8 of uint8 images [H][W][C], C = 1 / 3 / 4, for a RAGGED batch (every image has its own size,
// channel count and orientation) in ONE launch: grid (tiles, N), one workgroup per 64 x 64-pixel tile of the STORED image.
//
// With T = the orientation transposes (5..8), FY / FX = it reverses the stored rows / columns, upright pixel (yd, xd) is stored pixel
//     T ? (FY ? H-1-xd : xd,  FX ? W-1-yd : yd)  :  (FY ? H-1-yd : yd,  FX ? W-1-xd : xd)
// (orientation: T FY FX -- 1: 000, 2: 001, 3: 011, 4: 010, 5: 100, 6: 110, 7: 111, 8: 101), so a stored tile is an upright tile, and
// its pixels only move inside it.  A workgroup
//   1. brings the tile's stored rows to LDS as they are: every row is one run of tw * C bytes of the image; the run is cut at the 16-byte
//      boundaries of its OWN global address, whole 16-byte windows are one load each, the bytes before the first and after the last
//      boundary go singly, one lane each (a lane that walked them would wait for one load after the other).  Nothing outside the run
//      is read.
//   2. writes the tile's upright rows in the same way: a lane owns one 16-byte window of one upright row, gathers its bytes from LDS
//      (that is where the transpose happens, on LDS bytes), and stores it whole; heads and tails go singly.  Nothing outside the run
//      is written, so neighbouring tiles, and neighbouring images of the batch, never touch each other's bytes.
// Both global sides are walked along their own rows; there is no per-byte strided global access.  The LDS row pitch is 69 words (odd):
// a transposed gather walks a column, 64 rows apart by 69 words each, which are 64 different banks.
// No atomics, no workgroup waits on another, the image index is a grid dimension: image n of a batch is computed exactly as alone.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "orient_batch.h"

namespace chk {

namespace {

constexpr int BLK = 256;
constexpr int TILE = ORIENT_TILE;
constexpr int PITCH = 276;                   // LDS bytes per stored row: 3 (alignment) + 64 * 4 <= 276 = 69 words

// The 16-byte windows of a run of nb bytes at global address g: window k covers [base + 16 k, base + 16 k + 16), base = g rounded
// down to 16.  -> the byte range [lo, hi) of the RUN (0 <= lo < hi <= nb) inside window k, hi - lo == 16 for a whole window.
__device__ __forceinline__ void window(uintptr_t g, int nb, int k, int& lo, int& hi) {
    const int mis = (int)(g & 15);
    lo = max(k * 16 - mis, 0);
    hi = min(k * 16 - mis + 16, nb);
}

// The first (which = 0) or last (which = 1) window of that run, when it is a partial one: false for a whole window, and for "the last"
// of a run that lies in one window (it is the first)
__device__ __forceinline__ bool edge(uintptr_t g, int nb, int which, int& lo, int& hi) {
    const int nwin = ((int)(g & 15) + nb + 15) >> 4;
    if (which && nwin == 1) return false;
    window(g, nb, which ? nwin - 1 : 0, lo, hi);
    return hi - lo != 16;
}

template <int C>
__device__ __forceinline__ void turn_tile(const OrientImage& d, uint8_t* __restrict__ dstbuf, uint8_t* lds) {
    const int tiles_x = (d.W + TILE - 1) / TILE;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int sy0 = ty * TILE, sx0 = tx * TILE;
    if (sy0 >= d.H) return;                                            // the grid is the batch's largest image
    const int th = min(TILE, d.H - sy0), tw = min(TILE, d.W - sx0);
    const int o = d.orient;
    const bool T = o >= 5, FY = o == 3 || o == 4 || o == 6 || o == 7, FX = o == 2 || o == 3 || o == 7 || o == 8;
    constexpr int NWIN = (15 + TILE * C + 15) / 16;                    // windows a run of up to 64 pixels can touch
    constexpr int VEC_ITER = (TILE * NWIN + BLK - 1) / BLK, EDGE_ITER = TILE * 32 / BLK;

    // ---- 1. stored rows -> LDS.  Row r sits at lds + r * PITCH + (its global address & 3): a whole window is then 4-byte aligned in LDS.
    // Fixed trip counts, so that a lane's loads are all in flight before the first is waited for.
    const size_t spitch = (size_t)d.W * C;
    const uintptr_t s0 = (uintptr_t)d.src + (size_t)sy0 * spitch + (size_t)sx0 * C;
    {
        const int nb = tw * C;
#pragma unroll
        for (int it = 0; it < VEC_ITER; ++it) {                        // whole windows: one 16-byte load each
            const int item = it * BLK + threadIdx.x, r = item / NWIN, k = item - r * NWIN;
            if (r >= th) continue;
            const uintptr_t g = s0 + (size_t)r * spitch;
            int lo, hi;
            window(g, nb, k, lo, hi);
            if (hi - lo != 16) continue;
            const uint4 v = *reinterpret_cast<const uint4*>(g + lo);
            uint32_t* lw = reinterpret_cast<uint32_t*>(lds + r * PITCH + (int)(g & 3) + lo);
            lw[0] = v.x, lw[1] = v.y, lw[2] = v.z, lw[3] = v.w;
        }
#pragma unroll
        for (int it = 0; it < EDGE_ITER; ++it) {                       // the first and the last window of a row where they are partial:
            const int item = it * BLK + threadIdx.x, r = item >> 5;    // one byte per lane (row, head | tail, byte of the window)
            if (r >= th) continue;
            const uintptr_t g = s0 + (size_t)r * spitch;
            int lo, hi;
            if (!edge(g, nb, (item >> 4) & 1, lo, hi) || lo + (item & 15) >= hi) continue;
            const int i = lo + (item & 15);
            lds[r * PITCH + (int)(g & 3) + i] = reinterpret_cast<const uint8_t*>(g)[i];
        }
    }
    __syncthreads();

    // ---- 2. LDS -> upright rows
    const int Wd = T ? d.H : d.W;
    const int dh = T ? tw : th, dw = T ? th : tw;
    const int dy0 = T ? (FX ? d.W - sx0 - tw : sx0) : (FY ? d.H - sy0 - th : sy0);
    const int dx0 = T ? (FY ? d.H - sy0 - th : sy0) : (FX ? d.W - sx0 - tw : sx0);
    const size_t dpitch = (size_t)Wd * C;
    const uintptr_t d0 = (uintptr_t)dstbuf + (size_t)d.dst + (size_t)dy0 * dpitch + (size_t)dx0 * C;
    const int s0lo = (int)(s0 & 3), sp3 = (int)(spitch & 3);
    // LDS offset of stored pixel (rs, ps) of the tile
    auto at = [&](int rs, int ps) { return rs * PITCH + ((s0lo + rs * sp3) & 3) + ps * C; };
    // ... of upright pixel (rd, pd) of the tile
    auto from = [&](int rd, int pd) {
        const int rs = T ? (FY ? th - 1 - pd : pd) : (FY ? th - 1 - rd : rd);
        const int ps = T ? (FX ? tw - 1 - rd : rd) : (FX ? tw - 1 - pd : pd);
        return at(rs, ps);
    };
    const int nb = dw * C;
#pragma unroll
    for (int it = 0; it < VEC_ITER; ++it) {
        const int item = it * BLK + threadIdx.x, rd = item / NWIN, k = item - rd * NWIN;
        if (rd >= dh) continue;
        const uintptr_t g = d0 + (size_t)rd * dpitch;
        int lo, hi;
        window(g, nb, k, lo, hi);
        if (hi - lo != 16) continue;
        int pd = lo / C, ch = lo - pd * C;
        int a = from(rd, pd);
        uint32_t w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                v |= (uint32_t)lds[a + ch] << (8 * b);
                if (++ch == C) {
                    ch = 0;
                    a = from(rd, ++pd);                                // (one pixel past the run on the last byte: computed, never read)
                }
            }
            w[j] = v;
        }
        *reinterpret_cast<uint4*>(g + lo) = make_uint4(w[0], w[1], w[2], w[3]);
    }
#pragma unroll
    for (int it = 0; it < EDGE_ITER; ++it) {
        const int item = it * BLK + threadIdx.x, rd = item >> 5;
        if (rd >= dh) continue;
        const uintptr_t g = d0 + (size_t)rd * dpitch;
        int lo, hi;
        if (!edge(g, nb, (item >> 4) & 1, lo, hi) || lo + (item & 15) >= hi) continue;
        const int i = lo + (item & 15), pd = i / C;
        reinterpret_cast<uint8_t*>(g)[i] = lds[from(rd, pd) + (i - pd * C)];
    }
}

__global__ __launch_bounds__(BLK) void orient_kernel(const OrientImage* __restrict__ desc, uint8_t* __restrict__ dst) {
    __shared__ __align__(16) uint8_t lds[TILE * PITCH];
    const OrientImage d = desc[blockIdx.y];
    if (d.C == 3) turn_tile<3>(d, dst, lds);
    else if (d.C == 1) turn_tile<1>(d, dst, lds);
    else turn_tile<4>(d, dst, lds);
}

}  // namespace

hipError_t orient_u8(const void* batch, size_t batch_bytes, int N, uint8_t* dst, void* ws, hipStream_t s) {
    const OrientImage* d = static_cast<const OrientImage*>(batch);
    unsigned tiles = 1;
    for (int n = 0; n < N; ++n) tiles = std::max(tiles, orient_tiles(d[n].H, d[n].W));
    const hipError_t e = hipMemcpyAsync(ws, batch, batch_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return e;
    orient_kernel<<<dim3(tiles, N), BLK, 0, s>>>(static_cast<const OrientImage*>(ws), dst);
    return hipGetLastError();
}

}  // namespace chk
