// png_encode.hip -- the PNG encoder's device side: N uint8 images [N,H,W,C] -> N complete zlib streams (RFC 1950 / 1951), ready to be
// wrapped into IHDR / IDAT / IEND on the host (ctrlhair_amd/pngenc.py).  Three launches per call, integer arithmetic only:
//   png_filter_kernel    the PNG row filters (RFC 2083 section 6): type byte + filtered row, H * (1 + W * C) bytes per image
//   png_deflate_kernel   one workgroup per PNG_CHUNK bytes of that stream: distance-1 run matching, a dynamic Huffman code per chunk,
//                        or a stored block where that is not smaller; every chunk starts and ends on a byte
//   png_deflate_dist_kernel   the same with matches at up to three further distances the caller gives (ch_png_encode_dist): a position
//                        goes to the distance whose interval of x[i] == x[i - d] around it is longest -- the rule stands above the kernel
//   png_gather_kernel    scans the chunk sizes, packs the chunks behind the zlib header, sums the Adler-32 pairs, appends the trailer
// Determinism: the only atomics are integer add (histograms, counts, checksum sums) and integer or (bits into LDS words); both commute
// and associate exactly, every other value is a pure function of the chunk's bytes, and a chunk never looks outside itself.  The bytes
// of an image therefore depend neither on the call nor on the batch it is in.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>

#include "kernels.h"
#include "wave_ops.h"

namespace chk {

namespace {

constexpr int NT = 256;                                  // threads of every workgroup here
constexpr int SEG = PNG_CHUNK / NT;                      // bytes of a chunk per thread of the deflate kernel: 128
constexpr int SEGP = SEG + 4;                            // LDS pitch of a segment: 33 dwords, so the threads' byte walks meet no bank twice
constexpr int SLOT = PNG_CHUNK + 16;                     // bytes a chunk may take in the workspace (stored: 5 + len), 16-byte multiple
constexpr uint32_t ADLER_MOD = 65521;
constexpr int NLL = 286, NCL = 19;                       // literal/length and code-length alphabets
constexpr int LL_PAD = 288;
constexpr int CLSEQ_MAX = 2 * NT;                        // code-length symbols of one header (at most 286 + 30), two per thread
static_assert(SEG * NT == PNG_CHUNK && SEG % 16 == 0 && SEG < 258, "a thread's segment: 16-byte groups, shorter than one full match");
static_assert(NLL + 30 <= CLSEQ_MAX, "header sequence fits");

struct Layout {                                          // workspace sections, every one 256-byte aligned
    size_t fpad, nchunks, filt, slots, csize, cadler, total;
};

__host__ __device__ inline size_t up(size_t x, size_t a) { return (x + a - 1) / a * a; }

Layout layout(int N, int H, int W, int C) {
    Layout L;
    const size_t F = (size_t)H * (1 + (size_t)W * C);
    L.fpad = up(F, 16);
    L.nchunks = (F + PNG_CHUNK - 1) / PNG_CHUNK;
    L.filt = 0;
    L.slots = up(L.filt + L.fpad * N, 256);
    L.csize = up(L.slots + L.nchunks * N * SLOT, 256);
    L.cadler = up(L.csize + L.nchunks * N * sizeof(int), 256);
    L.total = up(L.cadler + L.nchunks * N * 2 * sizeof(uint32_t), 256);
    return L;
}

// ---- block-wide scans over one int per thread (NT threads, every thread calls) -----------------------------------------------
__device__ __forceinline__ int scan_add_excl(int v, int* sh, int* total) {          // sh: 4 ints
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = wave_scan_incl(v, lane);
    __syncthreads();                                                                // (sh may still be read from the scan before)
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    int base = 0, t = 0;
    for (int q = 0; q < 4; ++q) {
        if (q < wave) base += sh[q];
        t += sh[q];
    }
    *total = t;
    return base + x - v;
}

__device__ __forceinline__ int scan_max_incl(int v, int* sh) {                      // max over threads 0..tid
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x = y > x ? y : x;
    }
    __syncthreads();
    if (lane == 63) sh[wave] = x;
    __syncthreads();
    for (int q = 0; q < 4; ++q)
        if (q < wave) x = sh[q] > x ? sh[q] : x;
    return x;
}

__device__ __forceinline__ int scan_min_incl_rev(int v, int* sh) {                  // min over threads tid..NT-1
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_down(x, o, 64);
        if (lane + o < 64) x = y < x ? y : x;
    }
    __syncthreads();
    if (lane == 0) sh[wave] = x;
    __syncthreads();
    for (int q = 0; q < 4; ++q)
        if (q > wave) x = sh[q] < x ? sh[q] : x;
    return x;
}

// ---- bits into LDS words ---------------------------------------------------------------------------------------------------------
// A writer owns a bit range [start, end) of the block image; it gathers bits in a 64-bit register and ors whole words out.  The first
// and the last word of a range are shared with the neighbouring writers, hence the integer atomicOr (the words start as zero).
struct BitWriter {
    uint32_t* words;
    uint64_t acc;
    int nacc, w;
    __device__ __forceinline__ void begin(uint32_t* out, int bit) {
        words = out;
        w = bit >> 5;
        nacc = bit & 31;
        acc = 0;
    }
    __device__ __forceinline__ void put(uint32_t v, int nb) {                       // nb <= 32 - and nacc < 32 before: no overflow of 64
        acc |= (uint64_t)v << nacc;
        nacc += nb;
        if (nacc >= 32) {
            atomicOr(&words[w], (uint32_t)acc);
            ++w;
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ void end() {
        if (nacc > 0 && acc) atomicOr(&words[w], (uint32_t)acc);
    }
};

// length 3..258 -> (symbol 257..285, extra bits, extra value)   (RFC 1951 section 3.2.5)
__device__ __forceinline__ void length_code(int len, int& sym, int& nextra, int& extra) {
    const int l = len - 3;
    if (len == 258) {
        sym = 285, nextra = 0, extra = 0;
    } else if (l < 8) {
        sym = 257 + l, nextra = 0, extra = 0;
    } else {
        const int nb = 29 - __clz(l);                                               // floor(log2 l) - 2
        sym = 261 + 4 * nb + ((l >> nb) & 3);
        nextra = nb;
        extra = l & ((1 << nb) - 1);
    }
}

// ---- length-limited Huffman code of one alphabet (every thread of the block calls) ------------------------------------------------
// Sort the used symbols by (frequency, symbol) -- a total order, so the result is unique --, build the Huffman tree with the two-queue
// merge (one thread: 2 m - 1 dependent steps), read the depths, limit them to maxbits by the Kraft-sum repair of miniz
// (tdefl_huffman_enforce_max_code_size), hand the lengths out longest-to-rarest, number the codes canonically (RFC 1951 3.2.2).
struct HuffScratch {
    uint32_t nfreq[2 * LL_PAD];
    uint16_t parent[2 * LL_PAD];
    uint16_t sorted[LL_PAD];
    int blcount[16];
    int next[16];
    int m;
};

__device__ void huff_build(const uint32_t* freq, int n, int maxbits, uint8_t* lens, uint16_t* codes, HuffScratch& S) {
    const int tid = threadIdx.x;
    __syncthreads();                                                                // freq complete, S free
    if (tid == 0) S.m = 0;
    if (tid < 16) S.blcount[tid] = 0;
    for (int i = tid; i < n; i += NT) lens[i] = 0, codes[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
        const uint32_t f = freq[i];
        if (f) {
            int r = 0;
            for (int j = 0; j < n; ++j) {
                const uint32_t g = freq[j];
                r += (g != 0) & ((g < f) | ((g == f) & (j < i)));
            }
            S.sorted[r] = (uint16_t)i;
            S.nfreq[r] = f;
            atomicAdd(&S.m, 1);
        }
    }
    __syncthreads();
    const int m = S.m;
    if (m == 0) return;                                                             // (uniform)
    if (m == 1) {                                                                   // one symbol: a 1-bit code (an incomplete set of one
        if (tid == 0) lens[S.sorted[0]] = 1;                                        //  code of length 1 is what inflate accepts), code 0
        __syncthreads();
        return;
    }
    if (tid == 0) {
        int leaf = 0, node = m;
        uint32_t lf = S.nfreq[0], nf = UINT_MAX;
        for (int next = m; next < 2 * m - 1; ++next) {
            uint32_t sum = 0;
            for (int k = 0; k < 2; ++k) {
                int idx;
                if (lf <= nf) {
                    idx = leaf++;
                    sum += lf;
                    lf = leaf < m ? S.nfreq[leaf] : UINT_MAX;
                } else {
                    idx = node++;
                    sum += nf;
                    nf = node < next ? S.nfreq[node] : UINT_MAX;
                }
                S.parent[idx] = (uint16_t)next;
            }
            S.nfreq[next] = sum;
            if (node == next) nf = sum;                                             // the internal queue was empty: this node heads it
        }
    }
    __syncthreads();
    const int root = 2 * m - 2;
    for (int k = tid; k < m; k += NT) {
        int d = 0;
        for (int x = k; x != root; x = S.parent[x]) ++d;
        atomicAdd(&S.blcount[d < maxbits ? d : maxbits], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int total = 0;
        for (int i = 1; i <= maxbits; ++i) total += S.blcount[i] << (maxbits - i);
        while (total > (1 << maxbits)) {
            S.blcount[maxbits]--;
            for (int i = maxbits - 1; i > 0; --i)
                if (S.blcount[i]) {
                    S.blcount[i]--;
                    S.blcount[i + 1] += 2;
                    break;
                }
            --total;
        }
        int code = 0;
        S.next[0] = 0;
        for (int i = 1; i <= maxbits; ++i) {
            code = (code + (i > 1 ? S.blcount[i - 1] : 0)) << 1;
            S.next[i] = code;
        }
    }
    __syncthreads();
    for (int k = tid; k < m; k += NT) {                                             // sorted[0] is the rarest: it takes the longest code
        int c = 0;
        for (int l = maxbits; l >= 1; --l) {
            c += S.blcount[l];
            if (k < c) {
                lens[S.sorted[k]] = (uint8_t)l;
                break;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < n; i += NT) {
        const int l = lens[i];
        if (l) {
            int before = 0;
            for (int j = 0; j < i; ++j) before += lens[j] == l;
            const uint32_t code = (uint32_t)(S.next[l] + before);
            codes[i] = (uint16_t)(__brev(code) >> (32 - l));                        // Huffman codes go out most significant bit first
        }
    }
    __syncthreads();
}

__device__ __forceinline__ int cl_extra_bits(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }

// The header's code-length sequence (RFC 1951 3.2.7), run-length coded with the symbols 16 / 17 / 18 as zlib does: `total` lengths
// len_at(0..total-1), the literal/length lengths followed by the distance lengths.  One thread calls; returns the number of symbols.
template <class F>
__device__ __forceinline__ int cl_sequence(int total, F len_at, uint8_t* seq_sym, uint8_t* seq_ext) {
    int ns = 0, i = 0;
    while (i < total) {
        const int v = len_at(i);
        int r = 1;
        while (i + r < total && len_at(i + r) == v) ++r;
        i += r;
        if (v == 0) {
            while (r >= 11) {
                const int t = r < 138 ? r : 138;
                seq_sym[ns] = 18, seq_ext[ns++] = (uint8_t)(t - 11);
                r -= t;
            }
            if (r >= 3) {
                seq_sym[ns] = 17, seq_ext[ns++] = (uint8_t)(r - 3);
                r = 0;
            }
            while (r-- > 0) seq_sym[ns] = 0, seq_ext[ns++] = 0;
        } else {
            seq_sym[ns] = (uint8_t)v, seq_ext[ns++] = 0;
            --r;
            while (r >= 3) {
                const int t = r < 6 ? r : 6;
                seq_sym[ns] = 16, seq_ext[ns++] = (uint8_t)(t - 3);
                r -= t;
            }
            while (r-- > 0) seq_sym[ns] = (uint8_t)v, seq_ext[ns++] = 0;
        }
    }
    return ns;
}

}  // namespace

// ---- row filters -----------------------------------------------------------------------------------------------------------------------
// Grid (H, N): one workgroup per row.  x = the byte, a = the byte one pixel to the left, b = the byte above, c = the byte above a; bytes
// outside the image are 0.  Adaptive choice: the type with the smallest sum of |int8(filtered byte)|, the lowest type on a tie (libpng's
// minimum-sum-of-absolute-differences heuristic).  Threads take four bytes each, grouped so that the four land on an aligned word of
// the output row (whose start, y * (1 + W * C) + 1, has any alignment).
namespace {

__device__ __forceinline__ int paeth(int a, int b, int c) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

__device__ __forceinline__ uint8_t filter_byte(int type, int x, int a, int b, int c) {
    switch (type) {
        case 0: return (uint8_t)x;
        case 1: return (uint8_t)(x - a);
        case 2: return (uint8_t)(x - b);
        case 3: return (uint8_t)(x - ((a + b) >> 1));
        default: return (uint8_t)(x - paeth(a, b, c));
    }
}

__device__ __forceinline__ int abs8(uint8_t v) { return v < 128 ? v : 256 - v; }

}  // namespace

__global__ __launch_bounds__(NT) void png_filter_kernel(const uint8_t* __restrict__ img, int H, int W, int C, int filter,
                                                        uint8_t* __restrict__ filt, size_t fpad) {
    __shared__ int part[4][5];
    __shared__ int chosen;
    const int y = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
    const int rb = W * C;                                                           // row bytes, <= 131072
    const uint8_t* row = img + ((size_t)n * H + y) * rb;
    const uint8_t* prev = row - rb;                                                 // read for y > 0 only
    const bool top = y == 0;
    const size_t ob = (size_t)y * (1 + (size_t)rb);
    uint8_t* out = filt + (size_t)n * fpad + ob;                                    // out[0] the type byte, out[1 + j] byte j
    const int j0 = (int)((4 - ((ob + 1) & 3)) & 3);                                 // first j whose output address is word aligned
    const int groups = 1 + (rb - j0 + 3) / 4;                                       // group 0: j in [0, j0); group g: [j0 + 4 (g - 1), + 4)
    int type = filter;
    if (filter < 0) {
        int sum[5] = {0, 0, 0, 0, 0};
        for (int g = tid; g < groups; g += NT) {
            const int jb = g == 0 ? 0 : j0 + 4 * (g - 1), je = (g == 0 ? j0 : jb + 4) < rb ? (g == 0 ? j0 : jb + 4) : rb;
            for (int j = jb; j < je; ++j) {
                const int x = row[j], a = j >= C ? row[j - C] : 0, b = top ? 0 : prev[j], c = (top || j < C) ? 0 : prev[j - C];
#pragma unroll
                for (int t = 0; t < 5; ++t) sum[t] += abs8(filter_byte(t, x, a, b, c));
            }
        }
        const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            int v = sum[t];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if (lane == 0) part[wave][t] = v;
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0, bsum = INT_MAX;
            for (int t = 0; t < 5; ++t) {
                const int v = part[0][t] + part[1][t] + part[2][t] + part[3][t];
                if (v < bsum) bsum = v, best = t;
            }
            chosen = best;
        }
        __syncthreads();
        type = chosen;
    }
    if (tid == 0) out[0] = (uint8_t)type;
    for (int g = tid; g < groups; g += NT) {
        const int jb = g == 0 ? 0 : j0 + 4 * (g - 1), je = (g == 0 ? j0 : jb + 4) < rb ? (g == 0 ? j0 : jb + 4) : rb;
        uint32_t word = 0;
        for (int j = jb; j < je; ++j) {
            const int x = row[j], a = j >= C ? row[j - C] : 0, b = top ? 0 : prev[j], c = (top || j < C) ? 0 : prev[j - C];
            word |= (uint32_t)filter_byte(type, x, a, b, c) << (8 * (j - jb));
        }
        if (je - jb == 4 && g > 0) {
            *reinterpret_cast<uint32_t*>(out + 1 + jb) = word;                      // aligned: filt, fpad and ob + 1 + jb are multiples of 4
        } else {
            for (int j = jb; j < je; ++j) out[1 + j] = (uint8_t)(word >> (8 * (j - jb)));
        }
    }
}

// ---- chunk deflate ---------------------------------------------------------------------------------------------------------------------
// Grid (chunks, N).  Thread t owns bytes [t * SEG, (t + 1) * SEG) of the chunk.  A run of L equal bytes starting at s is coded as the
// literal at s, then floor((L - 1) / 258) matches (258, distance 1) at s + 1 + 258 k, then the remainder r = (L - 1) mod 258 as one match
// if r >= 3 and as r literals otherwise: where a token starts and what it is follows from (s, L) alone, and a thread codes the tokens
// that start in its segment.  s and the run's end come from the segment itself or, for a run that crosses segments, from a max-scan of
// the last run start and a reverse min-scan of the first run end per segment.
namespace {

struct DeflateShared {
    uint32_t data[NT * SEGP / 4];                                                   // the chunk, SEG bytes per thread at pitch SEGP
    uint32_t out[SLOT / 4];                                                         // the block being assembled
    uint32_t hist[LL_PAD];
    uint8_t ll_len[LL_PAD];
    uint16_t ll_code[LL_PAD];
    uint32_t cl_hist[32];
    uint8_t cl_len[32];
    uint16_t cl_code[32];
    uint8_t seq_sym[CLSEQ_MAX], seq_ext[CLSEQ_MAX];
    HuffScratch hs;
    int smax_all[NT], emin_all[NT];
    int scan[4];
    int nseq, nlit, hdr_fixed;
    uint32_t s1, s2;
};

__device__ __forceinline__ int ld(const uint8_t* d, int i) { return d[(i >> 7) * SEGP + (i & (SEG - 1))]; }
static_assert(SEG == 128, "ld() splits an index at bit 7");

// the tokens that start in [a, b): PASS 0 counts symbols, PASS 1 returns their bits, PASS 2 writes them
template <int PASS>
__device__ __forceinline__ int walk(DeflateShared& sh, int a, int b, int len, int carry_start, int carry_end, BitWriter* bw) {
    const uint8_t* d = reinterpret_cast<const uint8_t*>(sh.data);
    int bits = 0;
    int i = a;
    while (i < b) {
        const int v = ld(d, i);
        const int s = (i == 0 || ld(d, i - 1) != v) ? i : carry_start;             // only the segment's first run can start before it
        int j = i;
        while (j + 1 < b && ld(d, j + 1) == v) ++j;
        const int e = (j + 1 == b && b < len && ld(d, b) == v) ? carry_end : j;
        const int R = e - s, full = R / 258, rem = R - full * 258;
        const int hi = e < b - 1 ? e : b - 1;
        int nlit = i == s ? 1 : 0, n258 = 0, mrem = 0;
        const int lo = i > s + 1 ? i : s + 1;
        if (lo <= hi) {
            // full matches start at s + 1 + 258 k, k < full; a segment is shorter than 258: at most one of them starts in [lo, hi]
            const int k = (lo - (s + 1) + 257) / 258;
            const int p = s + 1 + 258 * k;
            if (k < full && p <= hi) n258 = 1;
            const int pr = s + 1 + 258 * full;
            if (rem >= 3) {
                if (pr >= lo && pr <= hi) mrem = rem;
            } else if (rem > 0) {
                const int q0 = pr > lo ? pr : lo;
                if (q0 <= hi) nlit += hi - q0 + 1;
            }
        }
        // order in the stream: the literal at s, the full match, the remainder (match or literals) -- positions ascend in that order
        int msym = 0, mnx = 0, mx = 0;
        if (mrem) length_code(mrem, msym, mnx, mx);
        if (PASS == 0) {
            if (nlit) atomicAdd(&sh.hist[v], (uint32_t)nlit);
            if (n258) atomicAdd(&sh.hist[285], 1u);
            if (mrem) atomicAdd(&sh.hist[msym], 1u);
        } else if (PASS == 1) {
            bits += nlit * sh.ll_len[v] + n258 * (sh.ll_len[285] + 1);
            if (mrem) bits += sh.ll_len[msym] + mnx + 1;
        } else {
            const uint32_t lc = sh.ll_code[v];
            const int ln = sh.ll_len[v];
            const int first = i == s ? 1 : 0;
            if (first) bw->put(lc, ln);
            if (n258) bw->put(sh.ll_code[285], sh.ll_len[285] + 1);                 // + the distance symbol 0: one zero bit
            if (mrem) {
                bw->put(sh.ll_code[msym], sh.ll_len[msym]);
                bw->put((uint32_t)mx, mnx + 1);                                     // extra bits, then the zero distance bit
            }
            for (int q = first; q < nlit; ++q) bw->put(lc, ln);
        }
        i = hi + 1;
    }
    return bits;
}

template <int P>
struct Pass {
    static constexpr int value = P;
};

// What follows the literal/length code of a chunk, for both deflate kernels (every thread calls): the header with its code-length
// code, the body or the stored form, the copy to the chunk's slot.  ndc distance lengths dlen_at(0..ndc-1) follow the literal/length
// lengths in the header; walk(Pass<1>, -) returns the bits of the thread's tokens, walk(Pass<2>, writer) writes them.
template <class DLen, class Walk>
__device__ __forceinline__ void finish_chunk(DeflateShared& sh, int len, int ndc, DLen dlen_at, Walk walk, uint8_t* __restrict__ slot,
                                             int* __restrict__ csize, uint32_t* __restrict__ cadler) {
    const int tid = threadIdx.x;
    // the header's code-length sequence (RFC 1951 3.2.7): nlit literal/length lengths and the ndc distance lengths, run-length coded
    if (tid == 0) {
        int nlit = NLL;
        while (nlit > 257 && sh.ll_len[nlit - 1] == 0) --nlit;
        sh.nlit = nlit;
        const uint8_t* ll = sh.ll_len;
        const int ns = cl_sequence(nlit + ndc, [ll, nlit, dlen_at](int i) -> int { return i < nlit ? ll[i] : dlen_at(i - nlit); },
                                   sh.seq_sym, sh.seq_ext);
        sh.nseq = ns;
        for (int k = 0; k < ns; ++k) sh.cl_hist[sh.seq_sym[k]] += 1;
    }
    huff_build(sh.cl_hist, NCL, 7, sh.cl_len, sh.cl_code, sh.hs);

    if (tid == 0) {                                                                 // the fixed part of the header
        const uint8_t order[NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
        int ncl = NCL;
        while (ncl > 4 && sh.cl_len[order[ncl - 1]] == 0) --ncl;
        BitWriter bw;
        bw.begin(sh.out, 0);
        bw.put(0u | (2u << 1), 3);                                                  // BFINAL 0, BTYPE 10
        bw.put((uint32_t)(sh.nlit - 257), 5);
        bw.put((uint32_t)(ndc - 1), 5);                                             // HDIST
        bw.put((uint32_t)(ncl - 4), 4);
        for (int k = 0; k < ncl; ++k) bw.put(sh.cl_len[order[k]], 3);
        bw.end();
        sh.hdr_fixed = 17 + 3 * ncl;
    }
    __syncthreads();
    int total = 0;
    {
        const int nseq = sh.nseq;
        int bits = 0;
        for (int k = 2 * tid; k < 2 * tid + 2 && k < nseq; ++k) bits += sh.cl_len[sh.seq_sym[k]] + cl_extra_bits(sh.seq_sym[k]);
        const int off = scan_add_excl(bits, sh.scan, &total);
        BitWriter bw;
        bw.begin(sh.out, sh.hdr_fixed + off);
        for (int k = 2 * tid; k < 2 * tid + 2 && k < nseq; ++k) {
            const int sym = sh.seq_sym[k];
            bw.put(sh.cl_code[sym], sh.cl_len[sym]);
            if (sym >= 16) bw.put(sh.seq_ext[k], cl_extra_bits(sym));
        }
        bw.end();
    }
    const int hdr_bits = sh.hdr_fixed + total;

    const int mybits = walk(Pass<1>{}, nullptr);
    int body = 0;
    const int off = scan_add_excl(mybits, sh.scan, &body);
    const int block_bits = hdr_bits + body + sh.ll_len[256];
    const int coded_bytes = (block_bits + 3 + 7) / 8 + 4;                           // + the empty stored block that realigns: 000, pad, 00 00 FF FF
    int nbytes;
    if (coded_bytes < 5 + len) {                                                    // (uniform)
        nbytes = coded_bytes;
        BitWriter bw;
        bw.begin(sh.out, hdr_bits + off);
        walk(Pass<2>{}, &bw);
        bw.end();
        if (tid == 0) {
            BitWriter e;
            e.begin(sh.out, hdr_bits + body);
            e.put(sh.ll_code[256], sh.ll_len[256]);
            e.end();
            const int p = coded_bytes - 2;                                          // the bytes FF FF
            atomicOr(&sh.out[p >> 2], 0xFFu << (8 * (p & 3)));
            atomicOr(&sh.out[(p + 1) >> 2], 0xFFu << (8 * ((p + 1) & 3)));
        }
    } else {
        nbytes = 5 + len;
        __syncthreads();                                                            // the header bits in out are dead: overwrite them
        const uint8_t* d = reinterpret_cast<const uint8_t*>(sh.data);
        uint8_t* o = reinterpret_cast<uint8_t*>(sh.out);
        if (tid == 0) {
            o[0] = 0;                                                               // BFINAL 0, BTYPE 00
            o[1] = (uint8_t)(len & 255), o[2] = (uint8_t)(len >> 8);                // (len = 32768 fits 16 bits)
            o[3] = (uint8_t)(~len & 255), o[4] = (uint8_t)((~len >> 8) & 255);
        }
        for (int i = tid; i < len; i += NT) o[5 + i] = (uint8_t)ld(d, i);
    }
    __syncthreads();
    uint4* dst = reinterpret_cast<uint4*>(slot);
    const uint4* o4 = reinterpret_cast<const uint4*>(sh.out);
    for (int i = tid; i < (nbytes + 15) / 16; i += NT) dst[i] = o4[i];              // nbytes <= 5 + PNG_CHUNK <= SLOT
    if (tid == 0) {
        *csize = nbytes;
        cadler[0] = sh.s1 % ADLER_MOD;
        cadler[1] = sh.s2 % ADLER_MOD;
    }
}

// ---- the same with caller-given match distances ------------------------------------------------------------------------------------------
// Distances d[0] = 1, d[1..NK-1] the caller's, in priority order.  eq_d[i] = (i >= d and x[i] == x[i - d]); the maximal true intervals of
// eq_d are the match intervals of d.  Position i belongs to the distance whose interval containing i is longest (a tie goes to the
// earlier distance); if that interval is shorter than 3, i is a literal.  A class run is a maximal run of positions of one distance; it
// lies inside one interval of that distance, so every byte of it repeats the byte d before it.  A class run of R positions from p is
// coded as floor(R / 258) matches (258, d) at p + 258 k and then the remainder, one match if it is >= 3, else literals.  All of it is a
// pure function of the chunk's bytes and the list.  Per distance a thread holds eq_d of its segment as a 128-bit mask; the interval that
// enters and the one that leaves the segment come from the two scans of the distance-1 kernel, distance after distance through the same LDS
// arrays, the results kept in registers; a second pair of scans does the same for class runs.  The class of a position is recomputed
// from the masks in every walk, piece by piece (a piece: positions between two interval boundaries of any distance -- one class).
typedef unsigned __int128 u128;
constexpr int LIT = -1;
constexpr int NDSYM = 30;                                                           // distance alphabet

struct PngDistances {
    int d[4];                                                                       // d[0] = 1
};

struct DeflateDistShared : DeflateShared {
    uint32_t d_hist[32];
    uint8_t d_len[32];
    uint16_t d_code[32];
    int8_t cfirst[NT], clast[NT];                                                   // class of a segment's first and last position
};

__device__ __forceinline__ int ctz128(u128 m) {
    const uint64_t lo = (uint64_t)m, hi = (uint64_t)(m >> 64);
    return lo ? __builtin_ctzll(lo) : hi ? 64 + __builtin_ctzll(hi) : 128;
}
__device__ __forceinline__ int clz128(u128 m) {
    const uint64_t lo = (uint64_t)m, hi = (uint64_t)(m >> 64);
    return hi ? __builtin_clzll(hi) : lo ? 64 + __builtin_clzll(lo) : 128;
}

// distance 1..32768 -> (symbol 0..29, extra bits, extra value)   (RFC 1951 section 3.2.5)
__device__ __forceinline__ void distance_code(int dist, int& sym, int& nextra, int& extra) {
    const int t = dist - 1;
    if (t < 4) {
        sym = t, nextra = 0, extra = 0;
    } else {
        const int nb = 30 - __clz(t);                                               // floor(log2 t) - 1
        sym = 2 * nb + 2 + ((t >> nb) & 1);
        nextra = nb;
        extra = t & ((1 << nb) - 1);
    }
}

template <int NK>
struct Segment {                                                                    // what a thread knows of its bytes [a, b)
    u128 eq[NK];                                                                    // bit j: eq_d[a + j]   (0 from b on)
    int enter[NK], leave[NK];                                                       // start of the interval that enters at a, end of the one that leaves at b - 1; -1: none
    int dsym[NK], dnx[NK], dx[NK];                                                  // the distances' codes
    int a, b;
    int cprev, cnext;                                                               // class of a - 1 and of b (LIT outside the chunk)
    int cstart, cend;                                                               // the class run entering at a starts here, the one leaving at b - 1 ends here
};

// the piece that holds position i (a <= i < b): its class; nx = the first position behind it (i < nx <= b)
template <int NK>
__device__ __forceinline__ int piece(const Segment<NK>& g, int i, int& nx) {
    const int j = i - g.a;                                                          // 0..127
    int best = LIT, blen = 2, next = g.b;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const u128 m = g.eq[k] >> j;
        if ((uint64_t)m & 1) {
            const int up = ctz128(~m);                                              // true bits from j upwards: 1..128 - j
            const int down = clz128(~(g.eq[k] << (127 - j)));                       // and from j downwards: 1..j + 1
            const int hi = i + up - 1, lo = i - down + 1;
            const int e = (hi == g.b - 1 && g.leave[k] >= 0) ? g.leave[k] : hi;
            const int s = (lo == g.a && g.enter[k] >= 0) ? g.enter[k] : lo;
            if (e - s + 1 > blen) blen = e - s + 1, best = k;                       // (strictly longer: a tie stays with the earlier distance)
            next = hi + 1 < next ? hi + 1 : next;
        } else {
            const int z = i + ctz128(m);                                            // the next true bit, or >= b
            next = z < next ? z : next;
        }
    }
    nx = next > i ? next : i + 1;
    return best;
}

// the tokens that start in [a, b): PASS 0 counts symbols, PASS 1 returns their bits, PASS 2 writes them
template <int PASS, int NK>
__device__ __forceinline__ int walk_dist(DeflateDistShared& sh, const Segment<NK>& g, BitWriter* bw) {
    const uint8_t* d = reinterpret_cast<const uint8_t*>(sh.data);
    int bits = 0;
    auto literal = [&](int q) {
        const int v = ld(d, q);
        if (PASS == 0) atomicAdd(&sh.hist[v], 1u);
        else if (PASS == 1) bits += sh.ll_len[v];
        else bw->put(sh.ll_code[v], sh.ll_len[v]);
    };
    auto match = [&](int n, int c) {
        int lsym, lnx, lx, dsym = 0, dnx = 0, dx = 0;
        length_code(n, lsym, lnx, lx);
#pragma unroll
        for (int k = 0; k < NK; ++k)
            if (c == k) dsym = g.dsym[k], dnx = g.dnx[k], dx = g.dx[k];
        if (PASS == 0) {
            atomicAdd(&sh.hist[lsym], 1u);
            atomicAdd(&sh.d_hist[dsym], 1u);
        } else if (PASS == 1) {
            bits += sh.ll_len[lsym] + lnx + sh.d_len[dsym] + dnx;
        } else {
            bw->put(sh.ll_code[lsym], sh.ll_len[lsym]);
            if (lnx) bw->put((uint32_t)lx, lnx);
            bw->put(sh.d_code[dsym], sh.d_len[dsym]);
            if (dnx) bw->put((uint32_t)dx, dnx);
        }
    };
    int i = g.a, nx = g.a, c = LIT;
    if (i < g.b) c = piece(g, i, nx);
    while (i < g.b) {
        if (c == LIT) {
            for (int q = i; q < nx; ++q) literal(q);
            i = nx;
            if (i < g.b) c = piece(g, i, nx);
            continue;
        }
        const int lo = i, c0 = c;                                                   // the part [lo, hi] of a class run of c0
        do {
            i = nx;
            if (i < g.b) c = piece(g, i, nx);
        } while (i < g.b && c == c0);
        const int hi = i - 1;
        const int p = (lo == g.a && g.cprev == c0) ? g.cstart : lo;
        const int e = (i == g.b && g.cnext == c0) ? g.cend : hi;
        const int R = e - p + 1, full = R / 258, rem = R - full * 258, pr = p + 258 * full;
        // full matches start at p + 258 k, k < full; a segment is shorter than 258: at most one of them starts in [lo, hi]
        const int k = (lo - p + 257) / 258;
        if (k < full && p + 258 * k <= hi) match(258, c0);
        if (rem >= 3) {
            if (pr >= lo && pr <= hi) match(rem, c0);
        } else {
            for (int q = pr > lo ? pr : lo; q <= hi; ++q) literal(q);               // (at most two; pr + rem - 1 = e >= hi)
        }
    }
    return bits;
}

}  // namespace

template <int NK>
__global__ __launch_bounds__(NT) void png_deflate_dist_kernel(const uint8_t* __restrict__ filt, size_t fpad, size_t F, size_t nchunks,
                                                              PngDistances D, uint8_t* __restrict__ slots, int* __restrict__ csize,
                                                              uint32_t* __restrict__ cadler) {
    __shared__ DeflateDistShared sh;
    const int tid = threadIdx.x;
    const size_t chunk = blockIdx.x, n = blockIdx.y;
    const size_t begin = chunk * PNG_CHUNK;
    const int len = (int)(F - begin < (size_t)PNG_CHUNK ? F - begin : (size_t)PNG_CHUNK);      // 1..PNG_CHUNK
    const uint8_t* src = filt + n * fpad + begin;                                   // 16-byte aligned; fpad rounds the image up to 16
    uint8_t* d = reinterpret_cast<uint8_t*>(sh.data);

    for (int i = tid * 16; i < len; i += NT * 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + i);
        uint32_t* p = sh.data + ((i >> 7) * SEGP + (i & (SEG - 1))) / 4;
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
    }
    for (int i = tid; i < SLOT / 4; i += NT) sh.out[i] = 0;
    for (int i = tid; i < LL_PAD; i += NT) sh.hist[i] = 0;
    if (tid < 32) sh.cl_hist[tid] = 0, sh.d_hist[tid] = 0;
    if (tid == 0) sh.s1 = 0, sh.s2 = 0;
    __syncthreads();

    Segment<NK> g;
    const int a = tid * SEG, b = a + SEG < len ? a + SEG : len;                     // a >= len: an idle thread (a short last chunk)
    g.a = a, g.b = b;
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        g.eq[k] = 0;
        distance_code(D.d[k], g.dsym[k], g.dnx[k], g.dx[k]);
    }
    // the eq masks and the Adler-32 sums of the segment
    {
        uint32_t s1 = 0, s2 = 0;                                                    // s2 = sum (b - i) d[i] <= 255 * 128 * 129 / 2
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            uint64_t part[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) part[k] = 0;
            for (int j = 0; j < 64; ++j) {
                const int i = a + 64 * w + j;
                if (i < b) {
                    const int v = ld(d, i);
                    s1 += (uint32_t)v;
                    s2 += (uint32_t)(b - i) * (uint32_t)v;
#pragma unroll
                    for (int k = 0; k < NK; ++k)
                        if (i >= D.d[k] && ld(d, i - D.d[k]) == v) part[k] |= 1ull << j;
                }
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) g.eq[k] |= (u128)part[k] << (64 * w);
        }
        if (a < b) {
            // Adler-32 of the image: A = 1 + sum d, B = F + sum (F - pos) d; (F - pos) = (b - i) + (F - begin - b)
            const uint32_t after = (uint32_t)((F - begin - (size_t)b) % ADLER_MOD);
            const uint32_t t2 = (uint32_t)(((uint64_t)after * s1 + s2) % ADLER_MOD);
            atomicAdd(&sh.s1, s1);                                                  // <= 255 * 32768: no overflow
            atomicAdd(&sh.s2, t2);                                                  // <= 256 * 65520
        }
    }
    // per distance: the interval that enters the segment and the one that leaves it
#pragma unroll
    for (int k = 0; k < NK; ++k) {
        const int dk = D.d[k];
        const bool busy = a < b;
        const bool prevbit = busy && a > 0 && a - 1 >= dk && ld(d, a - 1) == ld(d, a - 1 - dk);
        const bool nextbit = busy && b < len && b >= dk && ld(d, b) == ld(d, b - dk);
        const u128 m = g.eq[k];
        const u128 starts = m & ~((m << 1) | (u128)(prevbit ? 1 : 0));
        const u128 ends = m & ~((m >> 1) | (nextbit ? (u128)1 << (b - 1 - a) : (u128)0));
        const int last_start = starts ? a + 127 - clz128(starts) : -1;
        const int first_end = ends ? a + ctz128(ends) : INT_MAX;
        const int smax = scan_max_incl(last_start, sh.scan);
        const int emin = scan_min_incl_rev(first_end, sh.scan);
        // a thread needs its predecessor's inclusive maximum and its successor's inclusive minimum: pass them through LDS
        sh.smax_all[tid] = smax;
        sh.emin_all[tid] = emin;
        __syncthreads();
        g.enter[k] = (busy && ((uint64_t)m & 1) && prevbit) ? sh.smax_all[tid - 1] : -1;            // (prevbit: tid > 0)
        g.leave[k] = (busy && nextbit && ((uint64_t)(m >> (b - 1 - a)) & 1)) ? sh.emin_all[tid + 1] : -1;   // (nextbit: b < len, tid < NT - 1)
    }
    // class runs: the neighbours' classes, then the same two scans
    {
        int nx;
        sh.cfirst[tid] = (int8_t)(a < b ? piece(g, a, nx) : LIT);
        sh.clast[tid] = (int8_t)(a < b ? piece(g, b - 1, nx) : LIT);
        __syncthreads();
        g.cprev = tid > 0 ? sh.clast[tid - 1] : LIT;
        g.cnext = tid < NT - 1 ? sh.cfirst[tid + 1] : LIT;
        int last_start = -1, first_end = INT_MAX, pc = g.cprev;
        for (int i = a; i < b; i = nx) {
            const int c = piece(g, i, nx);
            if (c != pc) {
                if (c != LIT) last_start = i;
                if (pc != LIT && i > a && first_end == INT_MAX) first_end = i - 1;
            }
            pc = c;
        }
        if (a < b && pc != LIT && pc != g.cnext && first_end == INT_MAX) first_end = b - 1;
        const int smax = scan_max_incl(last_start, sh.scan);
        const int emin = scan_min_incl_rev(first_end, sh.scan);
        sh.smax_all[tid] = smax;
        sh.emin_all[tid] = emin;
        __syncthreads();
        g.cstart = tid > 0 ? sh.smax_all[tid - 1] : 0;
        g.cend = tid < NT - 1 ? sh.emin_all[tid + 1] : len - 1;
    }

    if (tid == 0) atomicAdd(&sh.hist[256], 1u);                                     // end of block
    walk_dist<0>(sh, g, nullptr);
    huff_build(sh.hist, NLL, 15, sh.ll_len, sh.ll_code, sh.hs);
    // the distance code: a real length-limited code over the used symbols (at most NK); one used symbol, or none, gets one bit
    huff_build(sh.d_hist, NDSYM, 15, sh.d_len, sh.d_code, sh.hs);
    int ndc = NDSYM;
    while (ndc > 1 && sh.d_len[ndc - 1] == 0) --ndc;
    const bool none = ndc == 1 && sh.d_len[0] == 0;                                 // no match at all: symbol 0 with one bit, as in png_deflate_kernel
    __syncthreads();
    if (none && tid == 0) sh.d_len[0] = 1;
    const uint8_t* dl = sh.d_len;
    finish_chunk(
        sh, len, ndc, [dl](int i) -> int { return dl[i]; },
        [&](auto pass, BitWriter* bw) -> int { return walk_dist<decltype(pass)::value>(sh, g, bw); },
        slots + (n * nchunks + chunk) * SLOT, csize + n * nchunks + chunk, cadler + 2 * (n * nchunks + chunk));
}

__global__ __launch_bounds__(NT) void png_deflate_kernel(const uint8_t* __restrict__ filt, size_t fpad, size_t F, size_t nchunks,
                                                         uint8_t* __restrict__ slots, int* __restrict__ csize,
                                                         uint32_t* __restrict__ cadler) {
    __shared__ DeflateShared sh;
    const int tid = threadIdx.x;
    const size_t chunk = blockIdx.x, n = blockIdx.y;
    const size_t begin = chunk * PNG_CHUNK;
    const int len = (int)(F - begin < (size_t)PNG_CHUNK ? F - begin : (size_t)PNG_CHUNK);      // 1..PNG_CHUNK
    const uint8_t* src = filt + n * fpad + begin;                                   // 16-byte aligned; fpad rounds the image up to 16
    uint8_t* d = reinterpret_cast<uint8_t*>(sh.data);

    for (int i = tid * 16; i < len; i += NT * 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + i);
        uint32_t* p = sh.data + ((i >> 7) * SEGP + (i & (SEG - 1))) / 4;
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
    }
    for (int i = tid; i < SLOT / 4; i += NT) sh.out[i] = 0;
    for (int i = tid; i < LL_PAD; i += NT) sh.hist[i] = 0;
    if (tid < 32) sh.cl_hist[tid] = 0;
    if (tid == 0) sh.s1 = 0, sh.s2 = 0;
    __syncthreads();

    // run boundaries and the Adler-32 sums of the segment
    const int a = tid * SEG, b = a + SEG < len ? a + SEG : len;                     // a >= len: an idle thread (a short last chunk)
    int last_start = -1, first_end = INT_MAX;
    {
        uint32_t s1 = 0, s2 = 0;                                                    // s2 = sum (b - i) d[i] <= 255 * 128 * 129 / 2
        int prevv = a > 0 && a < len ? ld(d, a - 1) : -1;
        for (int i = a; i < b; ++i) {
            const int v = ld(d, i);
            if (v != prevv) {
                last_start = i;
                if (i > a && first_end == INT_MAX) first_end = i - 1;
            }
            prevv = v;
            s1 += (uint32_t)v;
            s2 += (uint32_t)(b - i) * (uint32_t)v;
        }
        if (a < b) {
            if (first_end == INT_MAX && (b == len || ld(d, b) != prevv)) first_end = b - 1;
            // Adler-32 of the image: A = 1 + sum d, B = F + sum (F - pos) d; (F - pos) = (b - i) + (F - begin - b)
            const uint32_t after = (uint32_t)((F - begin - (size_t)b) % ADLER_MOD);
            const uint32_t t2 = (uint32_t)(((uint64_t)after * s1 + s2) % ADLER_MOD);
            atomicAdd(&sh.s1, s1);                                                  // <= 255 * 32768: no overflow
            atomicAdd(&sh.s2, t2);                                                  // <= 256 * 65520
        }
    }
    const int smax = scan_max_incl(last_start, sh.scan);
    const int emin = scan_min_incl_rev(first_end, sh.scan);
    // a thread needs its predecessor's inclusive maximum and its successor's inclusive minimum: pass them through LDS
    sh.smax_all[tid] = smax;
    sh.emin_all[tid] = emin;
    __syncthreads();
    const int cstart = tid > 0 ? sh.smax_all[tid - 1] : 0;
    const int cend = tid < NT - 1 ? sh.emin_all[tid + 1] : len - 1;

    if (tid == 0) atomicAdd(&sh.hist[256], 1u);                                     // end of block
    walk<0>(sh, a, b, len, cstart, cend, nullptr);
    huff_build(sh.hist, NLL, 15, sh.ll_len, sh.ll_code, sh.hs);
    // only distance symbol 0 exists: one distance length, 1
    finish_chunk(
        sh, len, 1, [](int) -> int { return 1; },
        [&](auto pass, BitWriter* bw) -> int { return walk<decltype(pass)::value>(sh, a, b, len, cstart, cend, bw); },
        slots + (n * nchunks + chunk) * SLOT, csize + n * nchunks + chunk, cadler + 2 * (n * nchunks + chunk));
}

// ---- gather -----------------------------------------------------------------------------------------------------------------------------
// Grid (blocks, N).  Every block of an image scans that image's chunk sizes tile by tile (256 at a time) and copies the chunks of the tile
// that are its own (chunk k of a tile goes to block k mod gridDim.x); block 0 also writes the zlib header, the final empty block (a
// fixed-Huffman block holding only its end code: 03 00), the Adler-32 and sizes[n].
__global__ __launch_bounds__(NT) void png_gather_kernel(const uint8_t* __restrict__ slots, const int* __restrict__ csize,
                                                        const uint32_t* __restrict__ cadler, size_t nchunks, size_t F, size_t bound,
                                                        uint8_t* __restrict__ out, long long* __restrict__ sizes) {
    __shared__ int scan[4];
    __shared__ long long offs[NT];
    __shared__ int sz[NT];
    __shared__ uint32_t sum1, sum2;
    const int tid = threadIdx.x;
    const size_t n = blockIdx.y;
    uint8_t* image = out + n * bound;
    const int* cs = csize + n * nchunks;
    long long base = 2;
    for (size_t tile = 0; tile < nchunks; tile += NT) {
        const size_t c = tile + tid;
        const int v = c < nchunks ? cs[c] : 0;
        int total = 0;
        const int ex = scan_add_excl(v, scan, &total);                              // <= 256 * (PNG_CHUNK + 5): fits
        offs[tid] = base + ex;
        sz[tid] = v;
        __syncthreads();
        for (int k = blockIdx.x; k < NT && tile + k < nchunks; k += gridDim.x) {
            const uint8_t* s = slots + (n * nchunks + tile + k) * SLOT;             // 16-byte aligned
            uint8_t* dptr = image + offs[k];
            const int nb = sz[k];
            int head = (int)((4 - (reinterpret_cast<uintptr_t>(dptr) & 3)) & 3);
            head = head < nb ? head : nb;
            const int words = (nb - head) / 4;
            if (tid < head) dptr[tid] = s[tid];
            const uint32_t* sw = reinterpret_cast<const uint32_t*>(s);
            uint32_t* dw = reinterpret_cast<uint32_t*>(dptr + head);
            const int shb = 8 * (head & 3);                                         // source bytes head + 4 w: the same misalignment for all w
            for (int w = tid; w < words; w += NT) {
                const int q = (head + 4 * w) >> 2;
                const uint32_t lo = sw[q];
                dw[w] = shb ? (lo >> shb) | (sw[q + 1] << (32 - shb)) : lo;         // q + 1: at most byte nb + 3 < SLOT of the slot
            }
            const int done = head + 4 * words;
            if (tid < nb - done) dptr[done + tid] = s[done + tid];
        }
        base += total;
        __syncthreads();
    }
    if (blockIdx.x == 0) {
        if (tid == 0) sum1 = 0, sum2 = 0;
        __syncthreads();
        uint32_t s1 = 0, s2 = 0;
        for (size_t c = tid; c < nchunks; c += NT) {
            s1 = (s1 + cadler[2 * (n * nchunks + c)]) % ADLER_MOD;
            s2 = (s2 + cadler[2 * (n * nchunks + c) + 1]) % ADLER_MOD;
        }
        atomicAdd(&sum1, s1);
        atomicAdd(&sum2, s2);
        __syncthreads();
        if (tid == 0) {
            const uint32_t A = (1 + sum1) % ADLER_MOD, B = (uint32_t)((F % ADLER_MOD + sum2) % ADLER_MOD);
            image[0] = 0x78, image[1] = 0x01;                                       // deflate, 32 KiB window; check bits, fastest level
            uint8_t* t = image + base;
            t[0] = 0x03, t[1] = 0x00;
            t[2] = (uint8_t)(B >> 8), t[3] = (uint8_t)B, t[4] = (uint8_t)(A >> 8), t[5] = (uint8_t)A;
            sizes[n] = base + 6;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
size_t png_zlib_bound(int H, int W, int C) {
    const size_t F = (size_t)H * (1 + (size_t)W * C);
    return 2 + F + 10 * ((F + PNG_CHUNK - 1) / PNG_CHUNK) + 2 + 4;
}

size_t png_encode_workspace_bytes(int N, int H, int W, int C) { return layout(N, H, W, C).total; }

// dist: ndist (0..3) host values, checked by the caller; ndist = 0 launches the distance-1 kernel, whose bytes are those of every release
hipError_t png_encode_dist(const uint8_t* img, int N, int H, int W, int C, int filter, const int* dist, int ndist, uint8_t* out,
                           int64_t* sizes, void* ws, hipStream_t s) {
    const Layout L = layout(N, H, W, C);
    const size_t F = (size_t)H * (1 + (size_t)W * C);
    uint8_t* base = static_cast<uint8_t*>(ws);
    uint8_t* filt = base + L.filt;
    uint8_t* slots = base + L.slots;
    int* csize = reinterpret_cast<int*>(base + L.csize);
    uint32_t* cadler = reinterpret_cast<uint32_t*>(base + L.cadler);
    hipLaunchKernelGGL(png_filter_kernel, dim3(H, N), dim3(NT), 0, s, img, H, W, C, filter, filt, L.fpad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)L.nchunks, N);
    PngDistances D = {{1, 0, 0, 0}};
    for (int k = 0; k < ndist; ++k) D.d[1 + k] = dist[k];
    switch (ndist) {
        case 0: hipLaunchKernelGGL(png_deflate_kernel, grid, dim3(NT), 0, s, filt, L.fpad, F, L.nchunks, slots, csize, cadler); break;
        case 1: hipLaunchKernelGGL(png_deflate_dist_kernel<2>, grid, dim3(NT), 0, s, filt, L.fpad, F, L.nchunks, D, slots, csize, cadler); break;
        case 2: hipLaunchKernelGGL(png_deflate_dist_kernel<3>, grid, dim3(NT), 0, s, filt, L.fpad, F, L.nchunks, D, slots, csize, cadler); break;
        case 3: hipLaunchKernelGGL(png_deflate_dist_kernel<4>, grid, dim3(NT), 0, s, filt, L.fpad, F, L.nchunks, D, slots, csize, cadler); break;
        default: return hipErrorInvalidValue;
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned gb = (unsigned)(L.nchunks < 64 ? L.nchunks : 64);
    hipLaunchKernelGGL(png_gather_kernel, dim3(gb, N), dim3(NT), 0, s, slots, csize, cadler, L.nchunks, F, png_zlib_bound(H, W, C), out,
                       reinterpret_cast<long long*>(sizes));
    return hipGetLastError();
}

hipError_t png_encode(const uint8_t* img, int N, int H, int W, int C, int filter, uint8_t* out, int64_t* sizes, void* ws, hipStream_t s) {
    return png_encode_dist(img, N, H, W, C, filter, nullptr, 0, out, sizes, ws, s);
}

}  // namespace chk
