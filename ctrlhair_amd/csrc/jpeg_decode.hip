// ch_jpeg_decode and ch_jpeg_decode_rst (include/ctrlhair_hip.h): N baseline-JPEG scans -> N images.
//
// Entropy stage, parallel WITHIN a scan (jpeg_entropy_core.h has every address decision and runs on the CPU under sanitizers):
//   jpeg_sync_kernel    `rounds` launches.  One wavefront per chunk of 64 subsequences of 128 bytes, the chunk's bytes and the image's six
//                       Huffman tables in LDS.  Inside a launch the lanes whose entry state changed decode and hand their exit to the
//                       next lane until nothing changes; between launches the last exit of a chunk becomes the first entry of the next,
//                       through two state buffers: a launch reads only what the launch before wrote.
//   jpeg_chain_kernel   one workgroup per image: is the chain of states whole (else the first break decides the status), exclusive
//                       prefix sum of the block counts, block total against the image's.
//   jpeg_write_kernel   the decode again from the now-true states, scattering the non-zero coefficients into the zeroed int16
//                       [blocks][64] buffer (natural order, the DC as a difference).
//   jpeg_dc_kernel      one workgroup per (image, component): prefix sum of the DC differences in scan order, 32-bit, stored as 16.
// Pixel stage, libjpeg's integer arithmetic:
//   jpeg_idct_kernel    dequantise and jidctint's slow-integer inverse DCT, one block per 8 lanes (a column each, then a row each), into
//                       component planes of whole blocks.
//   jpeg_colour_kernel  fancy upsampling of the chroma planes (h2v1 / h2v2, replication when the plane is at most 2 wide) fused with the
//                       16-bit fixed-point YCbCr -> RGB, 16 pixels per thread, 16-byte stores when the rows allow.
// Integer arithmetic only, no atomics: image n is a pure function of its bytes, the same in every batch and every call.
//
// Restart intervals (ch_jpeg_decode_rst: restart[n] MCUs per interval; a workgroup serves one stream, so the choice is uniform in it).  The
// sync and write kernels run the RST instantiation of the entropy core: lanes jump over RSTm markers into the one state every decoder has
// behind a marker.  jpeg_write_kernel, which decodes the true chain from true block ordinals, judges every jump (je::RstAudit) and turns
// the stream into RESTART; jpeg_dc_kernel restarts its prefix sums at every interval.  restart == nullptr or restart[n] == 0 (or an
// interval that holds the whole scan) takes the code without any of this.
#include <hip/hip_runtime.h>

#include "jpeg_entropy_core.h"
#include "kernels.h"
#include "launch.h"

namespace chk {
namespace {
namespace je = jpegent;

struct Shape {
    int H, W, C, sampling;
    int hs, vs;                            // luma sampling factors
    uint32_t mw, mh;                       // MCUs across and down
    je::Geometry g;
    uint32_t nsub_max;                     // subsequences of the longest stream accepted
    uint32_t bound;                        // its bytes
    uint32_t ypitch, yrows, cpitch, crows; // planes of whole blocks
    uint64_t plane_bytes;                  // per image
};

Shape make_shape(int H, int W, int C, int sampling) {
    Shape s;
    s.H = H, s.W = W, s.C = C, s.sampling = sampling;
    s.hs = (C == 3 && sampling) ? 2 : 1;
    s.vs = (C == 3 && sampling == 2) ? 2 : 1;
    s.mw = (uint32_t)(W + 8 * s.hs - 1) / (8 * s.hs);
    s.mh = (uint32_t)(H + 8 * s.vs - 1) / (8 * s.vs);
    s.g = je::geometry(H, W, C, sampling);
    const uint64_t b = 512ull * s.g.nblocks;
    s.bound = (uint32_t)(b < je::MAX_STREAM - 1 ? b : je::MAX_STREAM - 1);
    s.nsub_max = (s.bound + je::SUBSEQ - 1) / je::SUBSEQ;
    s.ypitch = s.mw * s.hs * 8, s.yrows = s.mh * s.vs * 8;
    s.cpitch = s.mw * 8, s.crows = s.mh * 8;
    s.plane_bytes = (uint64_t)s.ypitch * s.yrows + (C == 3 ? 2ull * s.cpitch * s.crows : 0);
    return s;
}

struct Layout {
    size_t coef, state[2], first, planes, flags, total;
};
size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }
Layout make_layout(const Shape& s, int N) {
    Layout l;
    size_t at = 0;
    l.coef = at, at = up16(at + (size_t)N * s.g.nblocks * 64 * sizeof(int16_t));
    for (int k = 0; k < 2; ++k) l.state[k] = at, at = up16(at + (size_t)N * s.nsub_max * sizeof(je::SubState));
    l.first = at, at = up16(at + (size_t)N * s.nsub_max * sizeof(uint32_t));
    l.planes = at, at = up16(at + (size_t)N * s.plane_bytes);
    l.flags = at, at = up16(at + (size_t)N * 2 * sizeof(int32_t));
    l.total = at;
    return l;
}

// ---- entropy stage -----------------------------------------------------------------------------------------------------------------------
struct ChunkShared {
    je::Huff huff[6];
    alignas(16) uint8_t win[je::CHUNK + je::MARGIN + 16];
};

// bytes [0, len) of stream n, clipped: a stream longer than the bound has no subsequences (jpeg_chain_kernel reports it)
__device__ inline uint32_t stream_of(const uint8_t* streams, const int64_t* offsets, int n, uint32_t bound, const uint8_t*& in) {
    const int64_t lo = offsets[n], hi = offsets[n + 1];
    in = streams + lo;
    return (hi > lo && (uint64_t)(hi - lo) <= bound) ? (uint32_t)(hi - lo) : 0u;
}

// The chunk's window and the image's tables into LDS (all 64 lanes; ends with a barrier).  Returns the window.
__device__ inline je::Window stage_chunk(ChunkShared& sh, const uint8_t* in, uint32_t len, uint32_t c, const uint8_t* tb, int lane) {
    const uint32_t base = c * (uint32_t)je::CHUNK;                             // < len: the caller's chunk has subsequences
    const uint32_t wl = len - base < (uint32_t)(je::CHUNK + je::MARGIN) ? len - base : (uint32_t)(je::CHUNK + je::MARGIN);
    const uint8_t* src = in + base;                                            // only [0, wl) of it is read
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15);    // byte k of the window lives at win[mis + k]
    const uint32_t head = (16 - mis) & 15;                                     // bytes before the first 16-byte line
    const uint32_t hb = head < wl ? head : wl;
    if ((uint32_t)lane < hb) sh.win[mis + lane] = src[lane];
    const uint32_t nvec = (wl - hb) / 16;
    for (uint32_t j = lane; j < nvec; j += 64)
        *reinterpret_cast<uint4*>(sh.win + mis + hb + 16 * j) = *reinterpret_cast<const uint4*>(src + hb + 16 * j);
    const uint32_t done = hb + 16 * nvec;
    if (done + lane < wl) sh.win[mis + done + lane] = src[done + lane];       // < 16 bytes left
    if (lane < 6) je::build_codes(sh.huff[lane], tb + je::TABLE_HUFF + lane * je::TABLE_HUFF_STRIDE);
    for (int k = lane; k < 6 * 256; k += 64) sh.huff[k >> 8].vals[k & 255] = tb[je::TABLE_HUFF + (k >> 8) * je::TABLE_HUFF_STRIDE + 16 + (k & 255)];
    __syncthreads();
    for (int k = lane; k < 6 << je::FAST_BITS; k += 64) {
        const int t = k >> je::FAST_BITS;
        sh.huff[t].fast[k & ((1 << je::FAST_BITS) - 1)] = je::fast_entry(sh.huff[t], (uint32_t)(k & ((1 << je::FAST_BITS) - 1)));
    }
    __syncthreads();
    return je::Window{sh.win + mis, base, wl};
}

__device__ inline je::State shfl_up_state(je::State s) {
    je::State r;
    r.pos = (uint32_t)__shfl_up((int)s.pos, 1);
    r.bz = (uint32_t)__shfl_up((int)s.bz, 1);
    return r;
}

__global__ __launch_bounds__(64) void jpeg_sync_kernel(const uint8_t* __restrict__ streams, const int64_t* __restrict__ offsets,
                                                       const uint8_t* __restrict__ tables, je::Geometry g, uint32_t bound, uint32_t nsub_max,
                                                       const je::SubState* __restrict__ prev, je::SubState* __restrict__ cur,
                                                       int32_t* __restrict__ flags, const uint32_t* __restrict__ restart) {
    __shared__ ChunkShared sh;
    const int n = blockIdx.y, lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    const bool rst = restart && je::effective_restart(g, restart[n]);
    const uint8_t* in;
    const uint32_t len = stream_of(streams, offsets, n, bound, in);
    const uint32_t nsub = (len + je::SUBSEQ - 1) / je::SUBSEQ;
    if (c * (uint32_t)je::LANES >= nsub) return;                               // the whole workgroup
    const uint32_t i = c * je::LANES + lane;
    const bool active = i < nsub;
    const uint64_t at = (uint64_t)n * nsub_max + i;
    je::SubState st{{je::INVALID, je::OK}, {je::INVALID, je::OK}, 0};
    je::State own{0, 0};
    bool changed = false;
    if (active) {
        if (i) own = rst ? je::guess_rst(i, in[i * je::SUBSEQ - 1], in[i * je::SUBSEQ]) : je::guess(i, in[i * je::SUBSEQ - 1], in[i * je::SUBSEQ]);
        if (!prev) {
            st.entry = own;
            changed = true;
        } else {
            st = prev[at];
            if (lane == 0 && i) {
                const je::State e = je::entry_from(prev[at - 1].exit, own);
                changed = !je::same(e, st.entry);
                st.entry = e;
            }
        }
    }
    if (!__syncthreads_or(changed)) {                                          // nothing to decode: the states carry over
        if (active) cur[at] = st;
        return;
    }
    const je::Window w = stage_chunk(sh, in, len, c, tables + (size_t)n * je::TABLE_BYTES, lane);
    // a marker inside the scan: 0xFF followed by a byte that is no stuffing (nor, in a stream with restart intervals, RST0..RST7)
    if (active) {
        const uint32_t b0 = i * je::SUBSEQ, b1 = b0 + je::SUBSEQ < len - 1 ? b0 + je::SUBSEQ : len - 1;
        bool marker = false;
        if (rst) {
            for (uint32_t b = b0; b < b1; ++b) marker |= je::byte_at(w, b) == 0xFF && je::byte_at(w, b + 1) != 0 && !je::is_rst(je::byte_at(w, b + 1));
        } else {
            for (uint32_t b = b0; b < b1; ++b) marker |= je::byte_at(w, b) == 0xFF && je::byte_at(w, b + 1) != 0;
        }
        if (marker) flags[2 * n] = 1;
    }
    const uint32_t end = (i + 1) * je::SUBSEQ < len ? (i + 1) * je::SUBSEQ : len;
    for (int round = 0; round <= je::LANES; ++round) {
        if (changed) {
            je::NoAudit none;
            if (rst) je::run_subseq<true>(sh.huff, g, w, len, end, st.entry, 0u, je::NoSink{}, none, st.exit, st.count);
            else je::run_subseq<false>(sh.huff, g, w, len, end, st.entry, 0u, je::NoSink{}, none, st.exit, st.count);
        }
        const je::State before = shfl_up_state(st.exit);
        changed = false;
        if (active && lane) {
            const je::State e = je::entry_from(before, own);
            changed = !je::same(e, st.entry);
            st.entry = e;
        }
        if (!__syncthreads_or(changed)) break;
    }
    if (active) cur[at] = st;
}

constexpr int SCAN_THREADS = 256;

// inclusive scan of v over the workgroup's SCAN_THREADS threads (buf: SCAN_THREADS values); every thread returns its inclusive sum
__device__ inline uint32_t block_scan(uint32_t v, uint32_t* buf) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
        const uint32_t add = t >= d ? buf[t - d] : 0u;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const uint32_t r = buf[t];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(SCAN_THREADS) void jpeg_chain_kernel(const int64_t* __restrict__ offsets, je::Geometry g, uint32_t bound,
                                                                  uint32_t nsub_max, const je::SubState* __restrict__ fin,
                                                                  uint32_t* __restrict__ first, const int32_t* __restrict__ flags,
                                                                  int32_t* __restrict__ status) {
    __shared__ uint32_t buf[SCAN_THREADS];
    __shared__ uint32_t brk_at, brk_why;
    const int n = blockIdx.x, t = threadIdx.x;
    const int64_t lo = offsets[n], hi = offsets[n + 1];
    if (hi <= lo || (uint64_t)(hi - lo) > bound) {
        if (t == 0) status[n] = hi <= lo ? je::INPUT_END : je::TOO_LONG;
        return;
    }
    const uint32_t len = (uint32_t)(hi - lo), nsub = (len + je::SUBSEQ - 1) / je::SUBSEQ;
    const je::SubState* f = fin + (uint64_t)n * nsub_max;
    uint32_t* fo = first + (uint64_t)n * nsub_max;
    if (t == 0) brk_at = 0xFFFFFFFFu, brk_why = 0;
    __syncthreads();
    uint64_t carry = 0;
    uint32_t my_brk = 0xFFFFFFFFu, my_why = 0;
    for (uint32_t i0 = 0; i0 < nsub; i0 += SCAN_THREADS) {
        const uint32_t i = i0 + t;
        uint32_t cnt = 0;
        if (i < nsub) {
            cnt = f[i].count;
            if (i && my_brk == 0xFFFFFFFFu) {
                const int why = je::chain_break(f[i - 1].exit, f[i].entry);
                if (why) my_brk = i, my_why = (uint32_t)why;
            }
        }
        const uint32_t inc = block_scan(cnt, buf);
        const uint64_t excl = carry + inc - cnt;
        if (i < nsub) fo[i] = excl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)excl;   // a block ordinal beyond the image's is never stored to
        buf[t] = inc;
        __syncthreads();
        carry += buf[SCAN_THREADS - 1];
        __syncthreads();
    }
    if (my_brk != 0xFFFFFFFFu) atomicMin(&brk_at, my_brk);                     // LDS
    __syncthreads();
    if (my_brk != 0xFFFFFFFFu && my_brk == brk_at) brk_why = my_why;
    __syncthreads();
    if (t == 0) {
        int st = brk_at != 0xFFFFFFFFu ? (int)brk_why : je::final_status(f[nsub - 1].exit, carry, g);
        if (st == je::OK && flags[2 * n]) st = je::MARKER;
        status[n] = st;
    }
}

__global__ __launch_bounds__(64) void jpeg_write_kernel(const uint8_t* __restrict__ streams, const int64_t* __restrict__ offsets,
                                                        const uint8_t* __restrict__ tables, je::Geometry g, uint32_t bound, uint32_t nsub_max,
                                                        const je::SubState* __restrict__ fin, const uint32_t* __restrict__ first,
                                                        int32_t* status, int16_t* __restrict__ coef, const uint32_t* __restrict__ restart) {
    __shared__ ChunkShared sh;
    const int n = blockIdx.y, lane = threadIdx.x;
    const uint32_t c = blockIdx.x;
    if (status[n] != je::OK) return;
    const uint8_t* in;
    const uint32_t len = stream_of(streams, offsets, n, bound, in);
    const uint32_t nsub = (len + je::SUBSEQ - 1) / je::SUBSEQ;
    if (c * (uint32_t)je::LANES >= nsub) return;
    const je::Window w = stage_chunk(sh, in, len, c, tables + (size_t)n * je::TABLE_BYTES, lane);
    const uint32_t i = c * je::LANES + lane;
    if (i >= nsub) return;
    const uint64_t at = (uint64_t)n * nsub_max + i;
    const uint32_t end = (i + 1) * je::SUBSEQ < len ? (i + 1) * je::SUBSEQ : len;
    je::State ex;
    uint32_t cnt;
    const je::CoefSink sink{coef + (uint64_t)n * g.nblocks * 64, g.nblocks};
    const uint32_t ri = restart ? je::effective_restart(g, restart[n]) : 0u;
    if (ri) {
        je::RstAudit audit{ri * (uint32_t)g.bpm, g.nblocks, false};
        je::run_subseq<true>(sh.huff, g, w, len, end, fin[at].entry, first[at], sink, audit, ex, cnt);
        // the same value from every lane that stores it; the workgroups that read OK above, before it, only write coefficients nobody reads
        if (audit.bad) status[n] = je::RESTART;
    } else {
        je::NoAudit none;
        je::run_subseq<false>(sh.huff, g, w, len, end, fin[at].entry, first[at], sink, none, ex, cnt);
    }
}

constexpr int DC_PER_THREAD = 8;

// DC differences -> DC values, per component in scan order.  With a restart interval the predictor is 0 at the start of every interval:
// the value is S(j) - S(head(j) - 1), S the sums over the whole scan as without one, and the head of item j's interval follows from its
// index alone.  Every S at the end of an interval goes through LDS (ends[k + 1]: of the k-th interval that touches this group of items;
// ends[0]: of the one before, carried from group to group).  All of it modulo 2^16, which is what the stored values are.
__global__ __launch_bounds__(SCAN_THREADS) void jpeg_dc_kernel(je::Geometry g, const int32_t* __restrict__ status, int16_t* __restrict__ coef,
                                                               const uint32_t* __restrict__ restart) {
    constexpr uint32_t GROUP = SCAN_THREADS * DC_PER_THREAD;
    __shared__ uint32_t buf[SCAN_THREADS];
    __shared__ uint32_t ends[GROUP + 1];
    const int n = blockIdx.y, comp = blockIdx.x, t = threadIdx.x;
    if (status[n] != je::OK) return;
    const uint32_t per = comp == 0 ? (uint32_t)g.luma : 1u, firstb = comp == 0 ? 0u : (uint32_t)g.luma + comp - 1;
    const uint32_t nmcu = g.nblocks / (uint32_t)g.bpm, items = nmcu * per;
    const uint32_t ri = restart ? je::effective_restart(g, restart[n]) : 0u, seg = ri * per;          // items per interval
    int16_t* cf = coef + (uint64_t)n * g.nblocks * 64;
    uint32_t carry = 0;
    if (ri && t == 0) ends[0] = 0;                                             // (block_scan's barriers stand before its first use)
    for (uint32_t j0 = 0; j0 < items; j0 += GROUP) {                           // a thread sums DC_PER_THREAD neighbours, the workgroup scans the sums
        const uint32_t base = j0 + t * DC_PER_THREAD;
        uint32_t v[DC_PER_THREAD], run = 0;
#pragma unroll
        for (int k = 0; k < DC_PER_THREAD; ++k) {
            const uint32_t j = base + k;
            const uint64_t blk = (uint64_t)(j / per) * g.bpm + firstb + j % per;   // < nblocks when j < items
            run += j < items ? (uint32_t)(int32_t)cf[blk * 64] : 0u;
            v[k] = run;
        }
        const uint32_t inc = block_scan(run, buf);
        const uint32_t before = carry + inc - run;
        if (!ri) {
#pragma unroll
            for (int k = 0; k < DC_PER_THREAD; ++k) {
                const uint32_t j = base + k;
                const uint64_t blk = (uint64_t)(j / per) * g.bpm + firstb + j % per;
                if (j < items) cf[blk * 64] = (int16_t)(uint16_t)(before + v[k]);
            }
        } else {
            const uint32_t s0 = j0 / seg, s1 = (j0 + GROUP) / seg;             // the first interval in this group of items and in the next
#pragma unroll
            for (int k = 0; k < DC_PER_THREAD; ++k) {
                const uint32_t j = base + k;
                if (j < items && (j + 1) % seg == 0) ends[j / seg - s0 + 1] = before + v[k];         // index <= GROUP
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < DC_PER_THREAD; ++k) {
                const uint32_t j = base + k;
                const uint64_t blk = (uint64_t)(j / per) * g.bpm + firstb + j % per;
                if (j < items) cf[blk * 64] = (int16_t)(uint16_t)(before + v[k] - ends[j / seg - s0]);
            }
            const uint32_t next = ends[s1 - s0];                               // S(s1 * seg - 1); s1 - s0 <= GROUP; read only if a group follows
            __syncthreads();
            if (t == 0) ends[0] = next;
        }
        buf[t] = inc;
        __syncthreads();
        carry += buf[SCAN_THREADS - 1];
        __syncthreads();
    }
}

// ---- pixel stage --------------------------------------------------------------------------------------------------------------------------
constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137, F1961 = 16069,
              F2053 = 16819, F2562 = 20995, F3072 = 25172;
// beyond these libjpeg's C code, its SIMD code and this 32-bit restatement part ways: CH_JPEG_DEC_RANGE
constexpr int RANGE_COEF = 8191, RANGE_PASS1 = 8191, RANGE_LO = -512, RANGE_HI = 511;

// jidctint.c's one-dimensional inverse, descaled by SHIFT bits.  |d[k]| <= 8191 keeps every sum below 2^31.
template <int SHIFT>
__device__ inline void idct8(const int (&d)[8], int (&o)[8]) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * F0541;
    int tmp2 = z1 - z3 * F1847, tmp3 = z1 + z2 * F0765;
    int tmp0 = (d[0] + d[4]) * 8192, tmp1 = (d[0] - d[4]) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7], tmp1 = d[5], tmp2 = d[3], tmp3 = d[1];
    z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * F1175;
    tmp0 *= F0298, tmp1 *= F2053, tmp2 *= F3072, tmp3 *= F1501;
    z1 *= -F0899, z2 *= -F2562, z3 = z3 * -F1961 + z5, z4 = z4 * -F0390 + z5;
    tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    o[0] = (tmp10 + tmp3 + R) >> SHIFT, o[7] = (tmp10 - tmp3 + R) >> SHIFT;
    o[1] = (tmp11 + tmp2 + R) >> SHIFT, o[6] = (tmp11 - tmp2 + R) >> SHIFT;
    o[2] = (tmp12 + tmp1 + R) >> SHIFT, o[5] = (tmp12 - tmp1 + R) >> SHIFT;
    o[3] = (tmp13 + tmp0 + R) >> SHIFT, o[4] = (tmp13 - tmp0 + R) >> SHIFT;
}

constexpr int IDCT_THREADS = 256, IDCT_BLOCKS = IDCT_THREADS / 8;

__global__ __launch_bounds__(IDCT_THREADS) void jpeg_idct_kernel(const int16_t* __restrict__ coef, const uint8_t* __restrict__ tables, Shape s,
                                                                 int N, const int32_t* __restrict__ status, uint8_t* __restrict__ planes,
                                                                 int32_t* __restrict__ flags) {
    __shared__ int tr[IDCT_BLOCKS][8][9];
    const int slot = threadIdx.x >> 3, j = threadIdx.x & 7;
    const uint64_t total = (uint64_t)N * s.g.nblocks;
    for (uint64_t b0 = (uint64_t)blockIdx.x * IDCT_BLOCKS; b0 < total; b0 += (uint64_t)gridDim.x * IDCT_BLOCKS) {
        const uint64_t gb = b0 + slot;
        const bool on = gb < total;
        const int n = on ? (int)(gb / s.g.nblocks) : 0;
        const uint32_t blk = on ? (uint32_t)(gb % s.g.nblocks) : 0;
        const bool live = on && status[n] == je::OK;
        const uint32_t mcu = blk / (uint32_t)s.g.bpm, bi = blk % (uint32_t)s.g.bpm;
        const int comp = je::comp_of(s.g, bi);
        bool range = false;
        if (live) {
            const int16_t* cf = coef + gb * 64;
            const uint8_t* q = tables + (size_t)n * je::TABLE_BYTES + je::TABLE_QUANT + comp * 64;
            int d[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                d[k] = (int)cf[k * 8 + j] * (int)q[k * 8 + j];
                range |= d[k] > RANGE_COEF || d[k] < -RANGE_COEF;
                d[k] = d[k] > RANGE_COEF ? RANGE_COEF : d[k] < -RANGE_COEF ? -RANGE_COEF : d[k];
            }
            idct8<11>(d, o);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                range |= o[k] > RANGE_PASS1 || o[k] < -RANGE_PASS1;
                tr[slot][k][j] = o[k] > RANGE_PASS1 ? RANGE_PASS1 : o[k] < -RANGE_PASS1 ? -RANGE_PASS1 : o[k];
            }
        }
        __syncthreads();
        if (live) {
            int d[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = tr[slot][j][k];
            idct8<18>(d, o);
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                range |= o[k] < RANGE_LO || o[k] > RANGE_HI;
                const int v = o[k] + 128;
                const uint32_t u = (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
                if (k < 4) lo |= u << (8 * k);
                else hi |= u << (8 * (k - 4));
            }
            const uint32_t mx = mcu % s.mw, my = mcu / s.mw;
            uint8_t* pl = planes + (uint64_t)n * s.plane_bytes;
            uint64_t at;
            if (comp == 0) {
                const uint32_t bx = mx * s.hs + bi % s.hs, by = my * s.vs + bi / s.hs;
                at = (uint64_t)(by * 8 + j) * s.ypitch + bx * 8;
            } else {
                at = (uint64_t)s.ypitch * s.yrows + (uint64_t)(comp - 1) * s.cpitch * s.crows + (uint64_t)(my * 8 + j) * s.cpitch + mx * 8;
            }
            *reinterpret_cast<uint2*>(pl + at) = make_uint2(lo, hi);           // 8-byte aligned: pitches and plane sizes are multiples of 8
            if (range) flags[2 * n + 1] = 1;
        }
        __syncthreads();
    }
}

__device__ inline int chroma_h2v1(const uint8_t* p, uint32_t pitch, int cw, int y, int x) {
    const uint8_t* r = p + (uint64_t)y * pitch;
    const int c = x >> 1;
    if (cw <= 2) return r[c];
    const int c2 = (x & 1) ? (c + 1 < cw ? c + 1 : cw - 1) : (c > 0 ? c - 1 : 0);
    return (3 * r[c] + r[c2] + ((x & 1) ? 2 : 1)) >> 2;
}

__device__ inline int chroma_h2v2(const uint8_t* p, uint32_t pitch, int ch, int cw, int y, int x) {
    const int r = y >> 1, c = x >> 1;
    if (cw <= 2) return p[(uint64_t)r * pitch + c];
    const int r2 = (y & 1) ? (r + 1 < ch ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
    const int c2 = (x & 1) ? (c + 1 < cw ? c + 1 : cw - 1) : (c > 0 ? c - 1 : 0);
    const uint8_t *a = p + (uint64_t)r * pitch, *b = p + (uint64_t)r2 * pitch;
    const int s0 = 3 * a[c] + b[c], s1 = 3 * a[c2] + b[c2];
    return (3 * s0 + s1 + ((x & 1) ? 7 : 8)) >> 4;
}

__device__ inline uint32_t clamp255(int v) { return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

constexpr int FIX_CR_R = 91881, FIX_CB_B = 116130, FIX_CB_G = 22554, FIX_CR_G = 46802;   // int(x * 65536 + 0.5) of 1.402, 1.772, 0.34414, 0.71414

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* __restrict__ planes, Shape s, uint8_t* __restrict__ img,
                                                          int32_t* __restrict__ status, const int32_t* __restrict__ flags, int vec) {
    const int n = blockIdx.y;
    if (status[n] != je::OK) return;
    if (flags[2 * n + 1]) {                                                    // the inverse DCT left its range: every workgroup sees it
        if (blockIdx.x == 0 && threadIdx.x == 0) status[n] = je::RANGE;        // (read by the others only as "not OK" or before this store:
        return;                                                                //  either way they return here)
    }
    const uint32_t gw = (uint32_t)(s.W + 15) / 16;
    const uint64_t gi = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (uint64_t)gw * s.H) return;
    const int y = (int)(gi / gw), x0 = (int)(gi % gw) * 16;
    const uint8_t* pl = planes + (uint64_t)n * s.plane_bytes;
    const uint8_t* yr = pl + (uint64_t)y * s.ypitch;
    const uint8_t *cbp = pl + (uint64_t)s.ypitch * s.yrows, *crp = cbp + (uint64_t)s.cpitch * s.crows;
    const int cw = (s.W + s.hs - 1) / s.hs, ch = (s.H + s.vs - 1) / s.vs;
    uint8_t* o = img + ((uint64_t)n * s.H * s.W + (uint64_t)y * s.W + x0) * s.C;
    uint32_t pack[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pack[k] = 0;
    const int cnt = s.W - x0 < 16 ? s.W - x0 : 16;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < cnt) {
            const int x = x0 + k, Y = yr[x];
            if (s.C == 1) {
                if (vec) pack[k >> 2] |= (uint32_t)Y << (8 * (k & 3));
                else o[k] = (uint8_t)Y;
            } else {
                int cb, cr;
                if (s.sampling == 0) {
                    cb = cbp[(uint64_t)y * s.cpitch + x], cr = crp[(uint64_t)y * s.cpitch + x];
                } else if (s.sampling == 1) {
                    cb = chroma_h2v1(cbp, s.cpitch, cw, y, x), cr = chroma_h2v1(crp, s.cpitch, cw, y, x);
                } else {
                    cb = chroma_h2v2(cbp, s.cpitch, ch, cw, y, x), cr = chroma_h2v2(crp, s.cpitch, ch, cw, y, x);
                }
                cb -= 128, cr -= 128;
                const uint32_t R = clamp255(Y + ((FIX_CR_R * cr + 32768) >> 16));
                const uint32_t G = clamp255(Y + ((-FIX_CB_G * cb - FIX_CR_G * cr + 32768) >> 16));
                const uint32_t B = clamp255(Y + ((FIX_CB_B * cb + 32768) >> 16));
                if (vec) {
                    const int b = 3 * k;
                    pack[b >> 2] |= R << (8 * (b & 3));
                    pack[(b + 1) >> 2] |= G << (8 * ((b + 1) & 3));
                    pack[(b + 2) >> 2] |= B << (8 * ((b + 2) & 3));
                } else {
                    o[3 * k] = (uint8_t)R, o[3 * k + 1] = (uint8_t)G, o[3 * k + 2] = (uint8_t)B;
                }
            }
        }
    }
    if (vec) {                                                                 // W is a multiple of 16 and img is 16-byte aligned: so is o
        uint4* ov = reinterpret_cast<uint4*>(o);
        ov[0] = make_uint4(pack[0], pack[1], pack[2], pack[3]);
        if (s.C == 3) {
            ov[1] = make_uint4(pack[4], pack[5], pack[6], pack[7]);
            ov[2] = make_uint4(pack[8], pack[9], pack[10], pack[11]);
        }
    }
}

}  // namespace

int jpeg_decode_default_rounds() { return je::DEFAULT_ROUNDS; }

size_t jpeg_decode_workspace_bytes(int N, int H, int W, int C, int sampling) { return make_layout(make_shape(H, W, C, sampling), N).total; }

hipError_t jpeg_decode(const uint8_t* streams, const int64_t* offsets, const uint8_t* tables, const uint32_t* restart, int N, int H, int W, int C,
                       int sampling, int rounds, uint8_t* img, int32_t* status, void* ws, hipStream_t st) {
    const Shape s = make_shape(H, W, C, sampling);
    const Layout l = make_layout(s, N);
    uint8_t* w = static_cast<uint8_t*>(ws);
    int16_t* coef = reinterpret_cast<int16_t*>(w + l.coef);
    je::SubState* state[2] = {reinterpret_cast<je::SubState*>(w + l.state[0]), reinterpret_cast<je::SubState*>(w + l.state[1])};
    uint32_t* first = reinterpret_cast<uint32_t*>(w + l.first);
    int32_t* flags = reinterpret_cast<int32_t*>(w + l.flags);
    if (rounds <= 0) rounds = je::DEFAULT_ROUNDS;
    if (rounds > je::MAX_ROUNDS) rounds = je::MAX_ROUNDS;
    hipError_t e = hipMemsetAsync(coef, 0, (size_t)N * s.g.nblocks * 64 * sizeof(int16_t), st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(flags, 0, (size_t)N * 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const dim3 chunks((s.nsub_max + je::LANES - 1) / je::LANES, N);
    for (int k = 0; k < rounds; ++k)
        hipLaunchKernelGGL(jpeg_sync_kernel, chunks, dim3(64), 0, st, streams, offsets, tables, s.g, s.bound, s.nsub_max,
                           k ? state[(k - 1) & 1] : (const je::SubState*)nullptr, state[k & 1], flags, restart);
    const je::SubState* fin = state[(rounds - 1) & 1];
    hipLaunchKernelGGL(jpeg_chain_kernel, dim3(N), dim3(SCAN_THREADS), 0, st, offsets, s.g, s.bound, s.nsub_max, fin, first, flags, status);
    hipLaunchKernelGGL(jpeg_write_kernel, chunks, dim3(64), 0, st, streams, offsets, tables, s.g, s.bound, s.nsub_max, fin, first, status, coef, restart);
    hipLaunchKernelGGL(jpeg_dc_kernel, dim3(C, N), dim3(SCAN_THREADS), 0, st, s.g, status, coef, restart);
    const uint64_t groups = ((uint64_t)N * s.g.nblocks + IDCT_BLOCKS - 1) / IDCT_BLOCKS;
    const int cap = 16 * device_cus();
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)(groups < (uint64_t)cap ? groups : (uint64_t)cap)), dim3(IDCT_THREADS), 0, st, coef, tables,
                       s, N, status, w + l.planes, flags);
    const uint64_t px = (uint64_t)((W + 15) / 16) * H;
    const int vec = (W % 16 == 0 && (reinterpret_cast<uintptr_t>(img) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((px + 255) / 256), N), dim3(256), 0, st, w + l.planes, s, img, status, flags, vec);
    return hipGetLastError();
}

}  // namespace chk
