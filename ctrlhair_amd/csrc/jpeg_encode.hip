// Baseline JPEG encoding on the device: N uint8 images [N,H,W,C] (C = 1 grey, 3 RGB) -> N entropy-coded scans, byte-stuffed and padded,
// the bytes between the SOS header and EOI.  The arithmetic is libjpeg's, integer throughout, so that the file
// around the scan (ctrlhair_amd/jpegenc.py) is the one Pillow writes for the same pixels, quality and subsampling.
//
//   jpeg_transform_kernel   a tile of MCUs per workgroup: rows in 16-byte segments -> LDS, colour conversion (and 2x2 chroma
//                           downsampling), forward DCT with one block per 8 lanes (rows in registers, transpose through LDS, columns),
//                           quantiser, int16 zigzag coefficients -> workspace; dummy luma blocks get their DC here
//   jpeg_count_kernel       32 blocks per workgroup: the bits of every block from its coefficients and its predecessor's DC, summed per group
//   jpeg_scan_bits_kernel   one workgroup per image: exclusive scan of the group sums -> each group's bit offset; zeroes the words two
//                           groups share
//   jpeg_emit_kernel        the same 32 blocks: every lane's bits at its offset into an LDS image of the group's span, whole words to
//                           the raw stream, integer OR only on the words shared with a neighbouring group
//   jpeg_ffcount_kernel, jpeg_scan_ff_kernel, jpeg_stuff_kernel   0xFF bytes per 256-byte segment, their exclusive scan, the scatter
//                           that puts 0x00 behind each
// No workgroup waits on another; the only atomics are integer OR / add, so the bytes are a function of the pixels alone.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"
#include "wave_ops.h"

namespace chk {

namespace {

constexpr int NT = 256;                     // threads of every workgroup here
constexpr int GB = NT / 8;                  // blocks of a count / emit group: one block per 8 lanes
constexpr int MAX_BLOCK_BITS = 20 + 63 * 26;  // DC: 9-bit code + 11 bits; every AC: 16-bit code + 10 bits (no EOB then) = 1658
constexpr int EMIT_WORDS = (GB * MAX_BLOCK_BITS + 7 + 31) / 32 + 2;   // LDS image of a group's span: its bits, the pad, a partial word at each end
constexpr int SEG = 256;                    // bytes of the raw stream per wave of the stuffing kernels
constexpr int RAWP = 304;                   // LDS pitch of a tile's pixel row: 15 bytes of misalignment + 256 bytes, in whole 16-byte segments

enum Mode { GREY = 0, S444 = 1, S420 = 2 };

struct Geom {
    int H, W, C, mode;
    int bw, bh;              // blocks that hold pixels: ceil(W / 8), ceil(H / 8)
    int mcuW, mcuH, bpm;     // MCUs per row / column, blocks per MCU (1, 3, 6)
    int TW, TH, mpt;         // tile of the transform kernel in pixels, MCUs per tile
    int tilesX;
    int nblocks, G;          // blocks per image in coding order, groups of GB blocks
    size_t rawBytes;         // bytes of the un-stuffed stream per image in the workspace (16-byte multiple)
    size_t nsegB;            // stuffing segments per image that the workspace holds
};

Geom geometry(int H, int W, int C, int subsampling) {
    Geom g{};
    g.H = H, g.W = W, g.C = C;
    g.mode = C == 1 ? GREY : (subsampling == 2 ? S420 : S444);
    g.bw = (W + 7) / 8, g.bh = (H + 7) / 8;
    if (g.mode == S420) g.mcuW = (W + 15) / 16, g.mcuH = (H + 15) / 16, g.bpm = 6, g.TW = 64, g.TH = 16, g.mpt = 4;
    else if (g.mode == S444) g.mcuW = g.bw, g.mcuH = g.bh, g.bpm = 3, g.TW = 64, g.TH = 8, g.mpt = 8;
    else g.mcuW = g.bw, g.mcuH = g.bh, g.bpm = 1, g.TW = 256, g.TH = 8, g.mpt = 32;
    g.tilesX = (g.mcuW + g.mpt - 1) / g.mpt;
    g.nblocks = g.mcuW * g.mcuH * g.bpm;             // at most 3 * 2^30 / 64 + edges
    g.G = (g.nblocks + GB - 1) / GB;
    const size_t raw = ((size_t)g.nblocks * MAX_BLOCK_BITS + 7) / 8;
    g.rawBytes = ((raw + 15) & ~(size_t)15) + 16;
    g.nsegB = ((g.rawBytes + SEG - 1) / SEG + 3) & ~(size_t)3;
    return g;
}

struct Layout {
    size_t coef, gsum, goff, nbytes, raw, ffcnt, ffoff, total;
};

Layout layout(int N, const Geom& g) {
    Layout L{};
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t a = at; at += (bytes + 15) & ~(size_t)15; return a; };
    L.coef = take((size_t)N * g.nblocks * 64 * sizeof(int16_t));
    L.gsum = take((size_t)N * g.G * sizeof(uint32_t));
    L.goff = take((size_t)N * g.G * sizeof(uint64_t));
    L.nbytes = take((size_t)N * sizeof(uint64_t));
    L.raw = take((size_t)N * g.rawBytes);
    L.ffcnt = take((size_t)N * g.nsegB * sizeof(uint32_t));
    L.ffoff = take((size_t)N * g.nsegB * sizeof(uint64_t));
    L.total = at;
    return L;
}

// ---- tables --------------------------------------------------------------------------------------------------------------------------------
// ITU-T T.81 Annex K.1: quantisation tables, natural order
__constant__ uint8_t BASE_Q[2][64] = {
    {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
     18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// zigzag position of natural index r * 8 + c
__constant__ uint8_t ZZPOS[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                  10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// Annex K.3: codes per length 1..16 and the symbols in code order; the code of a symbol follows as in Annex C
struct HuffSpec {
    uint8_t bits[16];
    uint8_t vals[162];
    int n;
};
constexpr HuffSpec DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr HuffSpec AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};
constexpr HuffSpec AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa},
    162};

// symbol -> (length << 16) | code: [0,16) DC luma, [16,32) DC chroma, [32,288) AC luma, [288,544) AC chroma
constexpr int HT_DC = 0, HT_AC = 32, HT_WORDS = 544;
struct HuffCodes {
    uint32_t e[HT_WORDS];
};
constexpr HuffCodes make_codes() {
    HuffCodes t{};
    const HuffSpec* spec[4] = {&DC_LUMA, &DC_CHROMA, &AC_LUMA, &AC_CHROMA};
    const int base[4] = {0, 16, 32, 288};
    for (int s = 0; s < 4; ++s) {
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int j = 0; j < spec[s]->bits[len - 1]; ++j) t.e[base[s] + spec[s]->vals[k++]] = ((uint32_t)len << 16) | code++;
            code <<= 1;
        }
    }
    return t;
}
__constant__ HuffCodes HUFF = make_codes();
static_assert(make_codes().e[0] == ((2u << 16) | 0) && make_codes().e[32 + 0xF0] == ((11u << 16) | 0x7F9) && make_codes().e[288] == ((2u << 16) | 0) &&
                  make_codes().e[288 + 0xFA] == ((16u << 16) | 0xFFFE) && make_codes().e[16 + 11] == ((11u << 16) | 0x7FE),
              "Annex K.3: DC luma 0 = 00, AC luma ZRL = 11111111001, AC chroma EOB = 00, the last AC chroma code, DC chroma 11");

// ---- forward DCT: jfdctint.c (slow-integer), CONST_BITS 13, PASS1_BITS 2 --------------------------------------------------------------------
template <bool FIRST>
__device__ inline void fdct8(int (&d)[8]) {
    constexpr int CB = 13, P1 = 2;
    constexpr int F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137, F1961 = 16069,
                  F2053 = 16819, F2562 = 20995, F3072 = 25172;
    constexpr int SH = FIRST ? CB - P1 : CB + P1;
    auto desc = [](int x, int n) { return (x + (1 << (n - 1))) >> n; };
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) d[0] = (t10 + t11) << P1, d[4] = (t10 - t11) << P1;
    else d[0] = desc(t10 + t11, P1), d[4] = desc(t10 - t11, P1);
    const int za = (t12 + t13) * F0541;
    d[2] = desc(za + t13 * F0765, SH);
    d[6] = desc(za - t12 * F1847, SH);
    int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F1175;
    const int u4 = t4 * F0298, u5 = t5 * F2053, u6 = t6 * F3072, u7 = t7 * F1501;
    z1 *= -F0899, z2 *= -F2562, z3 = z3 * -F1961 + z5, z4 = z4 * -F0390 + z5;
    d[7] = desc(u4 + z1 + z3, SH);
    d[5] = desc(u5 + z2 + z4, SH);
    d[3] = desc(u6 + z2 + z3, SH);
    d[1] = desc(u7 + z1 + z4, SH);
}

// jccolor.c: 16-bit fixed point, FIX(x) = int(x * 65536 + 0.5)
__device__ inline int ycc_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ inline int ycc_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ inline int ycc_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// ---- (a) pixels -> quantised zigzag coefficients ------------------------------------------------------------------------------------------------
// grid (tilesX * mcuH, N).  img_end: one past the last byte of the whole batch; a 16-byte segment is loaded whole only inside [img, img_end).
__global__ __launch_bounds__(NT) void jpeg_transform_kernel(const uint8_t* __restrict__ img, const uint8_t* img_end, Geom g, int quality,
                                                            int16_t* __restrict__ coef) {
    __shared__ __align__(16) uint8_t raw[16 * RAWP];
    __shared__ uint8_t yp[2048], cbp[512], crp[512];          // Y: 16 x 64 (4:2:0), 8 x 64 (4:4:4), 8 x 256 (grey); chroma: 8 x 32 or 8 x 64
    __shared__ int tr[GB][8][9];
    __shared__ __align__(16) int16_t zz[GB][64];
    __shared__ uint16_t q8[2][64];
    const int tid = threadIdx.x, n = blockIdx.y;
    const int ty = blockIdx.x / g.tilesX, tx = blockIdx.x % g.tilesX;
    const int x0 = tx * g.TW, y0 = ty * g.TH;
    const int wt = min(g.TW, g.W - x0), ht = min(g.TH, g.H - y0);      // pixels of the tile that exist; both >= 1
    const uint8_t* ib = img + (size_t)n * g.H * g.W * g.C;

    if (tid < 128) {                                                    // jpeg_quality_scaling, jpeg_add_quant_table (baseline); times 8: the DCT's scale
        const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
        const int v = (BASE_Q[tid >> 6][tid & 63] * s + 50) / 100;
        q8[tid >> 6][tid & 63] = (uint16_t)(min(max(v, 1), 255) << 3);
    }
    {   // rows in 16-byte segments at their own alignment: byte i of tile row r lands at raw[r * RAWP + (address of the row & 15) + i]
        const int per = g.C == 1 ? 32 : 16;                              // segments per row: 15 + 256 bytes are 17, 15 + 192 are 13
        const int r = tid / per, j = tid % per;
        if (r < ht) {
            const uint8_t* a = ib + ((size_t)(y0 + r) * g.W + x0) * g.C;
            const int len = wt * g.C, mis = (int)(reinterpret_cast<uintptr_t>(a) & 15);
            if (16 * j < mis + len) {
                const uint8_t* p = a - mis + 16 * j;
                uint8_t* dst = raw + r * RAWP + 16 * j;
                if (p >= img && p + 16 <= img_end) {
                    *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(p);
                } else {
                    for (int k = 0; k < 16; ++k)
                        if (p + k >= a && p + k < a + len) dst[k] = p[k];
                }
            }
        }
    }
    __syncthreads();
    if (g.C == 1) {
        for (int p = tid; p < 8 * 256; p += NT) {
            const int r = min(p >> 8, ht - 1), c = min(p & 255, wt - 1);
            const int mis = (int)(reinterpret_cast<uintptr_t>(ib + ((size_t)(y0 + r) * g.W + x0)) & 15);
            yp[p] = raw[r * RAWP + mis + c];
        }
    } else {
        const bool sub = g.mode == S420;
        for (int p = tid; p < g.TH * 64; p += NT) {
            const int r = min(p >> 6, ht - 1), c = min(p & 63, wt - 1);
            const int mis = (int)(reinterpret_cast<uintptr_t>(ib + ((size_t)(y0 + r) * g.W + x0) * 3) & 15);
            const uint8_t* px = raw + r * RAWP + mis + 3 * c;
            yp[p] = (uint8_t)ycc_y(px[0], px[1], px[2]);
            if (!sub) cbp[p] = (uint8_t)ycc_cb(px[0], px[1], px[2]), crp[p] = (uint8_t)ycc_cr(px[0], px[1], px[2]);
        }
        if (sub) {
            // h2v2_downsample: the input's last row repeated to an even height and its last column outwards, then the last DOWNSAMPLED
            // row repeated: chroma row cy comes from min(cy, ceil(H / 2) - 1), whose two source rows are clamped to H - 1
            const int j = tid >> 5, i = tid & 31;
            const int cy = min((y0 >> 1) + j, ((g.H + 1) >> 1) - 1);
            const int ra = 2 * cy - y0, rb = min(ra + 1, ht - 1);
            const int ca = min(2 * i, wt - 1), cb = min(2 * i + 1, wt - 1);
            int sb = 1 + (i & 1), sr = 1 + (i & 1);                     // bias 1, 2, 1, 2 along the output columns (x0 / 2 is even)
            for (int k = 0; k < 4; ++k) {
                const int r = (k & 2) ? rb : ra, c = (k & 1) ? cb : ca;
                const int mis = (int)(reinterpret_cast<uintptr_t>(ib + ((size_t)(y0 + r) * g.W + x0) * 3) & 15);
                const uint8_t* px = raw + r * RAWP + mis + 3 * c;
                sb += ycc_cb(px[0], px[1], px[2]), sr += ycc_cr(px[0], px[1], px[2]);
            }
            cbp[tid] = (uint8_t)(sb >> 2), crp[tid] = (uint8_t)(sr >> 2);
        }
    }
    __syncthreads();

    // one block per 8 lanes: lane r transforms row r, the block is transposed through LDS, lane c transforms column c
    const int q = tid >> 3, lane = tid & 7;
    const int nq = g.mpt * g.bpm;                                        // 24, 24 or 32 blocks of the tile
    const int mj = q / g.bpm, k = q - mj * g.bpm;                        // MCU of the tile, block of the MCU
    const bool chroma = g.mode == S420 ? k >= 4 : k >= 1;
    if (q < nq) {
        const uint8_t* plane;
        int pitch, oy = 0, ox;
        if (g.mode == S420) {
            if (k < 4) plane = yp, pitch = 64, oy = (k >> 1) * 8, ox = mj * 16 + (k & 1) * 8;
            else plane = k == 4 ? cbp : crp, pitch = 32, ox = mj * 8;
        } else if (g.mode == S444) {
            plane = k == 0 ? yp : (k == 1 ? cbp : crp), pitch = 64, ox = mj * 8;
        } else {
            plane = yp, pitch = 256, ox = q * 8;
        }
        int d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = (int)plane[(oy + lane) * pitch + ox + i] - 128;
        fdct8<true>(d);
#pragma unroll
        for (int i = 0; i < 8; ++i) tr[q][lane][i] = d[i];
    }
    __syncthreads();
    if (q < nq) {
        int d[8];
#pragma unroll
        for (int v = 0; v < 8; ++v) d[v] = tr[q][v][lane];
        fdct8<false>(d);
#pragma unroll
        for (int v = 0; v < 8; ++v) {
            const unsigned qv = q8[chroma][v * 8 + lane];
            const unsigned a = ((unsigned)abs(d[v]) + (qv >> 1)) / qv;     // exact: plain integer division
            zz[q][ZZPOS[v * 8 + lane]] = (int16_t)(d[v] < 0 ? -(int)a : (int)a);
        }
    }
    __syncthreads();
    const int mx = tx * g.mpt + mj;
    if (q < nq && mx < g.mcuW) {
        int4 v = *reinterpret_cast<const int4*>(&zz[q][lane * 8]);
        if (g.mode == S420 && k >= 1 && k < 4) {
            // a luma block beyond the blocks that hold pixels: AC zero, DC that of the block before it in MCU order (itself maybe a dummy)
            const bool right = 2 * mx + 1 >= g.bw, below = 2 * ty + 1 >= g.bh;
            auto dummy = [&](int kk) { return ((kk & 1) && right) || ((kk & 2) && below); };
            if (dummy(k)) {
                int src = k - 1;
                while (dummy(src)) --src;                                 // block 0 always holds pixels
                v = make_int4(lane == 0 ? (int)(uint16_t)zz[q - k + src][0] : 0, 0, 0, 0);
            }
        }
        const size_t b = ((size_t)ty * g.mcuW + mx) * g.bpm + k;
        *reinterpret_cast<int4*>(coef + ((size_t)n * g.nblocks + b) * 64 + lane * 8) = v;
    }
}

// ---- (b), (c) entropy coding ---------------------------------------------------------------------------------------------------------------
// The pieces (value, bits) of one lane's 8 coefficients of block b, in order: lane 0 starts with the DC difference, lane 7 ends with EOB
// unless coefficient 63 is set.  mask: bit k = coefficient k is non-zero.
template <class Put>
__device__ inline void lane_pieces(const int16_t (&c)[8], int lane, uint64_t mask, int pred, const uint32_t* dc, const uint32_t* ac, Put put) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = lane * 8 + i, v = c[i];
        if (k == 0) {
            const int diff = v - pred, cat = 32 - __clz(abs(diff));          // __clz(0) = 32
            const uint32_t e = dc[cat];
            put(((e & 0xFFFF) << cat) | ((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << cat) - 1)), (int)(e >> 16) + cat);
        } else if (v != 0) {
            const uint64_t below = (mask & ((1ull << k) - 1)) | 1;           // the DC's position counts as the non-zero before the first AC
            const int run = k - (63 - __clzll(below)) - 1;
            const uint32_t zrl = ac[0xF0];
            for (int z = run >> 4; z > 0; --z) put(zrl & 0xFFFF, (int)(zrl >> 16));
            const int size = 32 - __clz(abs(v));
            const uint32_t e = ac[((run & 15) << 4) | size];
            put(((e & 0xFFFF) << size) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1)), (int)(e >> 16) + size);
        }
    }
    if (lane == 7 && !(mask >> 63)) put(ac[0] & 0xFFFF, (int)(ac[0] >> 16));
}

// What a lane of a count / emit group works on: block b = group * GB + tid / 8 of image n
struct LaneBlock {
    bool valid;
    int16_t c[8];
    uint64_t mask;
    int pred;
    const uint32_t *dc, *ac;
};

__device__ inline LaneBlock load_lane_block(const int16_t* __restrict__ coef, const Geom& g, int n, int b, int lane, const uint32_t* huff) {
    LaneBlock L;
    L.valid = b < g.nblocks;
    const int16_t* base = coef + (size_t)n * g.nblocks * 64;
    int4 v = make_int4(0, 0, 0, 0);
    if (L.valid) v = *reinterpret_cast<const int4*>(base + (size_t)b * 64 + lane * 8);
    const int w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        L.c[i] = (int16_t)(w[i >> 1] >> ((i & 1) * 16));
        m |= (L.c[i] != 0 ? 1u : 0u) << i;
    }
    uint64_t mask = (uint64_t)m << (8 * lane);
#pragma unroll
    for (int d = 1; d < 8; d <<= 1) mask |= __shfl_xor(mask, d, 8);          // all 8 lanes of the block are in one wave and all take part
    L.mask = mask;
    // the block of the same component before b in coding order
    const int k = b % g.bpm;
    int pb;
    bool chroma;
    if (g.mode == S420) chroma = k >= 4, pb = k == 0 ? b - 3 : (k < 4 ? b - 1 : b - 6);
    else chroma = k >= 1, pb = b - g.bpm;
    L.pred = (L.valid && lane == 0 && pb >= 0) ? base[(size_t)pb * 64] : 0;
    L.dc = huff + HT_DC + (chroma ? 16 : 0);
    L.ac = huff + HT_AC + (chroma ? 256 : 0);
    return L;
}

// exclusive scan over the workgroup's NT values in thread order; wsum: 4 words of LDS; total: the sum
__device__ inline uint32_t block_excl_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t x = wave_scan_incl(v, lane);
    __syncthreads();                                                          // the previous round's readers are done with wsum
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    uint32_t pre = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) {
        if (i < w) pre += wsum[i];
        total += wsum[i];
    }
    return pre + x - v;
}

// grid (G, N): gsum[n * G + group] = bits of the group's blocks
__global__ __launch_bounds__(NT) void jpeg_count_kernel(const int16_t* __restrict__ coef, Geom g, uint32_t* __restrict__ gsum) {
    __shared__ uint32_t huff[HT_WORDS];
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, n = blockIdx.y;
    for (int i = tid; i < HT_WORDS; i += NT) huff[i] = HUFF.e[i];
    __syncthreads();
    const LaneBlock L = load_lane_block(coef, g, n, blockIdx.x * GB + (tid >> 3), tid & 7, huff);
    uint32_t bits = 0;
    if (L.valid) lane_pieces(L.c, tid & 7, L.mask, L.pred, L.dc, L.ac, [&](uint32_t, int nb) { bits += nb; });
    uint32_t total;
    block_excl_scan(bits, wsum, total);
    if (tid == 0) gsum[(size_t)n * g.G + blockIdx.x] = total;
}

// grid (N): goff[n * G + group] = bits before the group; nbytes[n] = bytes of the padded stream.  Zeroes every word of the raw stream
// that two groups share (a group's first bit inside a word) and the stream's last partial word: the emit kernel ORs into exactly those.
__global__ __launch_bounds__(NT) void jpeg_scan_bits_kernel(const uint32_t* __restrict__ gsum, Geom g, uint64_t* __restrict__ goff,
                                                            uint64_t* __restrict__ nbytes, uint8_t* __restrict__ rawbuf) {
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, n = blockIdx.x;
    uint32_t* raww = reinterpret_cast<uint32_t*>(rawbuf + (size_t)n * g.rawBytes);
    uint64_t carry = 0;
    for (int base = 0; base < g.G; base += NT) {
        const int i = base + tid;
        uint32_t total;
        const uint32_t ex = block_excl_scan(i < g.G ? gsum[(size_t)n * g.G + i] : 0u, wsum, total);
        if (i < g.G) {
            const uint64_t off = carry + ex;
            goff[(size_t)n * g.G + i] = off;
            if (off & 31) raww[off >> 5] = 0;
        }
        carry += total;
    }
    if (tid == 0) {
        const uint64_t end = (carry + 7) & ~(uint64_t)7;
        nbytes[n] = end >> 3;
        if (end & 31) raww[end >> 5] = 0;
    }
}

// grid (G, N): the group's bits into an LDS image of its span, then whole words to the raw stream (big-endian bit order: byte-swapped)
__global__ __launch_bounds__(NT) void jpeg_emit_kernel(const int16_t* __restrict__ coef, Geom g, const uint64_t* __restrict__ goff,
                                                       uint8_t* __restrict__ rawbuf) {
    __shared__ uint32_t huff[HT_WORDS];
    __shared__ uint32_t wsum[4];
    __shared__ uint32_t span[EMIT_WORDS];
    const int tid = threadIdx.x, n = blockIdx.y, lane = tid & 7;
    for (int i = tid; i < HT_WORDS; i += NT) huff[i] = HUFF.e[i];
    for (int i = tid; i < EMIT_WORDS; i += NT) span[i] = 0;
    __syncthreads();
    const int b = blockIdx.x * GB + (tid >> 3);
    const LaneBlock L = load_lane_block(coef, g, n, b, lane, huff);
    uint32_t bits = 0;
    if (L.valid) lane_pieces(L.c, lane, L.mask, L.pred, L.dc, L.ac, [&](uint32_t, int nb) { bits += nb; });
    uint32_t total;
    const uint32_t ex = block_excl_scan(bits, wsum, total);
    const uint64_t S = goff[(size_t)n * g.G + blockIdx.x];
    uint64_t E = S + total;
    const bool last_group = blockIdx.x == g.G - 1;
    const int pad = last_group ? (int)((8 - (E & 7)) & 7) : 0;                // the stream's last byte is filled with 1-bits
    E += pad;
    const uint64_t w0 = S >> 5;                                               // first word of the span
    if (L.valid) {
        const uint64_t at = S + ex;
        uint32_t w = (uint32_t)((at >> 5) - w0);
        int fill = (int)(at & 31);
        uint64_t acc = 0;
        bool first = true;                                                    // the lane's first word may hold a neighbour's bits; the ones after it are its own
        auto put = [&](uint32_t val, int nb) {
            acc |= (uint64_t)val << (64 - fill - nb);                         // fill < 32, nb <= 27
            fill += nb;
            if (fill >= 32) {
                if (first) atomicOr(&span[w], (uint32_t)(acc >> 32)), first = false;
                else span[w] = (uint32_t)(acc >> 32);
                ++w, acc <<= 32, fill -= 32;
            }
        };
        lane_pieces(L.c, lane, L.mask, L.pred, L.dc, L.ac, put);
        if (b == g.nblocks - 1 && lane == 7 && pad) put((1u << pad) - 1, pad);
        if (fill) atomicOr(&span[w], (uint32_t)(acc >> 32));
    }
    __syncthreads();
    uint32_t* raww = reinterpret_cast<uint32_t*>(rawbuf + (size_t)n * g.rawBytes);
    const int nw = (int)(((E + 31) >> 5) - w0);
    for (int i = tid; i < nw; i += NT) {
        const uint64_t gw = w0 + i;
        const uint32_t v = __builtin_bswap32(span[i]);
        if (gw * 32 >= S && (gw + 1) * 32 <= E) raww[gw] = v;                 // every bit of the word is this group's
        else atomicOr(&raww[gw], v);                                          // shared with a neighbour: zeroed by jpeg_scan_bits_kernel
    }
}

// ---- (d) byte stuffing ---------------------------------------------------------------------------------------------------------------------------
// A thread owns 4 bytes of the raw stream, a wave one segment of SEG = 256.  grid (ceil(rawBytes / 1024), N): the workgroups behind
// nbytes[n] leave at once.
__device__ inline int ff_bytes(uint32_t w, uint64_t at, uint64_t nb) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) c += (at + k < nb && ((w >> (8 * k)) & 0xFF) == 0xFF) ? 1 : 0;
    return c;
}

__global__ __launch_bounds__(NT) void jpeg_ffcount_kernel(const uint8_t* __restrict__ rawbuf, Geom g, const uint64_t* __restrict__ nbytes,
                                                          uint32_t* __restrict__ ffcnt) {
    const int tid = threadIdx.x, n = blockIdx.y;
    const uint64_t nb = nbytes[n], at = ((uint64_t)blockIdx.x * NT + tid) * 4;
    if ((uint64_t)blockIdx.x * NT * 4 >= nb) return;
    const uint32_t* raww = reinterpret_cast<const uint32_t*>(rawbuf + (size_t)n * g.rawBytes);
    int c = at < nb ? ff_bytes(raww[at >> 2], at, nb) : 0;
    c = wave_sum(c);
    if ((tid & 63) == 0) ffcnt[(size_t)n * g.nsegB + (size_t)blockIdx.x * (NT / 64) + (tid >> 6)] = (uint32_t)c;
}

// grid (N): ffoff[n * nsegB + s] = 0xFF bytes before segment s; sizes[n] = bytes of the stuffed scan
__global__ __launch_bounds__(NT) void jpeg_scan_ff_kernel(const uint32_t* __restrict__ ffcnt, Geom g, const uint64_t* __restrict__ nbytes,
                                                          uint64_t* __restrict__ ffoff, long long* __restrict__ sizes) {
    __shared__ uint32_t wsum[4];
    const int tid = threadIdx.x, n = blockIdx.x;
    const uint64_t nb = nbytes[n], nseg = (nb + SEG - 1) / SEG;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < nseg; base += NT) {
        const uint64_t i = base + tid;
        uint32_t total;
        const uint32_t ex = block_excl_scan(i < nseg ? ffcnt[(size_t)n * g.nsegB + i] : 0u, wsum, total);
        if (i < nseg) ffoff[(size_t)n * g.nsegB + i] = carry + ex;
        carry += total;
    }
    if (tid == 0) sizes[n] = (long long)(nb + carry);
}

__global__ __launch_bounds__(NT) void jpeg_stuff_kernel(const uint8_t* __restrict__ rawbuf, Geom g, const uint64_t* __restrict__ nbytes,
                                                        const uint64_t* __restrict__ ffoff, uint8_t* __restrict__ out, size_t bound) {
    const int tid = threadIdx.x, n = blockIdx.y, lane = tid & 63;
    const uint64_t nb = nbytes[n], at = ((uint64_t)blockIdx.x * NT + tid) * 4;
    if ((uint64_t)blockIdx.x * NT * 4 >= nb) return;
    const uint32_t* raww = reinterpret_cast<const uint32_t*>(rawbuf + (size_t)n * g.rawBytes);
    const uint32_t w = at < nb ? raww[at >> 2] : 0;
    const int c = ff_bytes(w, at, nb);
    int x = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (at >= nb) return;
    const uint64_t seg = (uint64_t)blockIdx.x * (NT / 64) + (tid >> 6);
    uint8_t* o = out + (size_t)n * bound + at + ffoff[(size_t)n * g.nsegB + seg] + (uint64_t)(x - c);   // at most 2 * nb <= bound bytes in all
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (at + k < nb) {
            const uint8_t v = (uint8_t)(w >> (8 * k));
            *o++ = v;
            if (v == 0xFF) *o++ = 0;
        }
    }
}

}  // namespace

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// A block is at most MAX_BLOCK_BITS = 1658 bits (a DC of category 11 behind a 9-bit code, 63 AC terms of size 10 behind 16-bit codes, and
// then no EOB); the pad fills the last byte; stuffing at most doubles the bytes, the padded one included.
size_t jpeg_scan_bound(int H, int W, int C, int subsampling) {
    const Geom g = geometry(H, W, C, subsampling);
    return 2 * (((size_t)g.nblocks * MAX_BLOCK_BITS + 7) / 8) + 2;
}

size_t jpeg_encode_workspace_bytes(int N, int H, int W, int C, int subsampling) { return layout(N, geometry(H, W, C, subsampling)).total; }

hipError_t jpeg_encode(const uint8_t* img, int N, int H, int W, int C, int quality, int subsampling, uint8_t* out, int64_t* sizes, void* ws,
                       hipStream_t s) {
    const Geom g = geometry(H, W, C, subsampling);
    const Layout L = layout(N, g);
    uint8_t* base = static_cast<uint8_t*>(ws);
    int16_t* coef = reinterpret_cast<int16_t*>(base + L.coef);
    uint32_t* gsum = reinterpret_cast<uint32_t*>(base + L.gsum);
    uint64_t* goff = reinterpret_cast<uint64_t*>(base + L.goff);
    uint64_t* nbytes = reinterpret_cast<uint64_t*>(base + L.nbytes);
    uint8_t* raw = base + L.raw;
    uint32_t* ffcnt = reinterpret_cast<uint32_t*>(base + L.ffcnt);
    uint64_t* ffoff = reinterpret_cast<uint64_t*>(base + L.ffoff);
    hipError_t e;
    hipLaunchKernelGGL(jpeg_transform_kernel, dim3((unsigned)(g.tilesX * g.mcuH), N), dim3(NT), 0, s, img, img + (size_t)N * H * W * C, g, quality,
                       coef);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_count_kernel, dim3(g.G, N), dim3(NT), 0, s, coef, g, gsum);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_scan_bits_kernel, dim3(N), dim3(NT), 0, s, gsum, g, goff, nbytes, raw);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_emit_kernel, dim3(g.G, N), dim3(NT), 0, s, coef, g, goff, raw);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 sgrid((unsigned)((g.rawBytes + NT * 4 - 1) / (NT * 4)), N);
    hipLaunchKernelGGL(jpeg_ffcount_kernel, sgrid, dim3(NT), 0, s, raw, g, nbytes, ffcnt);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_scan_ff_kernel, dim3(N), dim3(NT), 0, s, ffcnt, g, nbytes, ffoff, reinterpret_cast<long long*>(sizes));
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(jpeg_stuff_kernel, sgrid, dim3(NT), 0, s, raw, g, nbytes, ffoff, out, jpeg_scan_bound(H, W, C, subsampling));
    return hipGetLastError();
}

}  // namespace chk
