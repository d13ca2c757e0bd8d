// conv_pw.h -- 1x1 ("pointwise") convolution on the exact-f32 matrix cores (v_mfma_f32_32x32x2_f32) for the learned ResBlock
// shortcut conv_s (architecture.py:75-79: x_s = conv_s(ace_s(x)), no bias) of the exact-f32 Winograd path, whose output the
// Winograd conv_1 launch adds as its residual (conv_wino.h).
//
// A 1x1 conv is a plain GEMM  out[row][pixel] = sum_ci W[row][ci] in[ci][pixel]  with 9x less reuse of every staged input byte
// than a 3x3 conv, so the block shares its input tile among RT row tiles: 8 waves = RT row tiles of 32 rows x (8 / RT) groups of
// 64 pixels; one ring stage = 16 input channels = 8 k-steps = 16 MFMAs (1024 matrix-pipe cycles) per wave against 16 KB
// (RT = 4: 128 pixels, 8 KB of input + 8 KB of A) or 20 KB (RT = 2: 256 pixels) of LDS-DMA.  Same machinery as conv_wino.h:
// persistent 512-thread blocks, every operand by LDS-DMA (buffer_load ... lds, 16 B per lane -- the pixel rows of a 1x1 conv are
// aligned, there is no halo), a 6-stage ring running as one flat sequence across the block's tasks, one barrier per stage.
// No input transform and no per-tap addressing: the non-MFMA instruction stream is ~40 instructions per 16 MFMAs.
#pragma once
#include "conv_wino.h"

namespace chk {

// GROUPED launch (conv_pw_grouped): several GEMMs with the same Cin and Cout but their own operands and pixel counts run as ONE
// persistent launch -- the exact-f32 style-LUT builds of all styled ACEs of the generator (sean_model.cpp: operands swapped, the
// "pixels" are the 18 C rows of conv_gamma / conv_beta, the GEMM rows the (sample, label) columns).  Group g owns the tasks
// [start, next group's start) x row groups: local task -> (row group fastest, pixel tile).
struct PwGroup {
    const float* in;        // [Cin][HW]
    const float* wpk;       // pack_pw_A image of the group's Cout rows
    float* out;             // [Cout][HW]
    int HW, start;          // HW % 128 == 0; pixel tiles (of 128) before this group: its first task is start * (row groups of the launch)
};
struct PwParams {
    const float* in;        // [B][Cin][HW]
    const float* wpk;       // pack_pw_A image
    float* out;             // [B][Cout][HW]
    int B, Cin, Cout, HW;   // Cin % 16 == 0, HW % (512 / RT) == 0
    const PwGroup* groups;  // device array of ngroups entries, or null (plain launch)
    int ngroups;
    long long in_bs;        // plain launch: floats between the samples of `in`; 0 = Cin * HW (a launch over the first Cin planes of wider samples: sean_model.cpp, Zencoder ConvTranspose)
    int wide;               // option "sean.pw_wide": 0 = pw_conv_kernel; 1 = 64-row wave tiles (pw_conv_wide_kernel) where the launcher's rule takes them
                            // (pw_wide_rule).  Grouped launch: the caller vouches for every group's HW % 256 == 0
    const int* skip;        // optional (code memo, the grouped style-LUT launch): device word; the whole launch returns at once where it reads 1
    // set by the launcher
    int nrg, npt, ntasks, nst;
};

// image of (row tile rt, stage st): [lane][8 k-steps] floats: W[row = 32 rt + (lane & 31)][ci = 16 st + 2 s + (lane >> 5)]
template <class F>
std::vector<float> pack_pw_A(int rows, int Cin, F get) {
    const int nrt = (rows + 31) / 32, nst = Cin / 16;
    std::vector<float> dst((size_t)nrt * nst * 512, 0.f);
    for (int rt = 0; rt < nrt; ++rt)
        for (int st = 0; st < nst; ++st)
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < 8; ++s) {
                    const int row = rt * 32 + (lane & 31), ci = 16 * st + 2 * s + (lane >> 5);
                    if (row < rows) dst[((size_t)rt * nst + st) * 512 + lane * 8 + s] = get(row, ci);
                }
    return dst;
}

template <int RT>
struct PwCfg {
    static constexpr int PG = 8 / RT, PXB = 64 * PG;             // pixel groups of 64 per block, pixels per block
    static constexpr int PDW = 16 * PXB, ADW = RT * 512;          // patch / A dwords per stage
    static constexpr int SDW = PDW + ADW, NST = 6;
    static constexpr int NPD = PDW / (4 * 512);                   // patch DMAs (16 B) per thread per stage: 1 (RT = 4) / 2 (RT = 2)
    static constexpr int NLD = NPD + 1;
    static constexpr int LDS_BYTES = NST * SDW * 4 + 512 * 16;    // + a scratch line per thread for the A DMA of idle threads
};

template <int RT>
__global__ __launch_bounds__(512, 1) void pw_conv_kernel(const PwParams p) {
    using Cfg = PwCfg<RT>;
    constexpr int PG = Cfg::PG, PXB = Cfg::PXB, PDW = Cfg::PDW, SDW = Cfg::SDW, NST = Cfg::NST, NPD = Cfg::NPD, NLD = Cfg::NLD;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;
    const int lb = xcd_remap(blockIdx.x, G);
    if (lb >= p.ntasks) return;
    if (p.skip && *p.skip) return;          // (code memo: every group's output still holds the LUT of these codes)
    const int mytasks = (p.ntasks - lb + G - 1) / G;
    const int nst = p.nst;
    constexpr unsigned SB = SDW * 4, RING = NST * SB;
    // grouped launch: task -> group (wave-uniform scan of at most a few dozen entries through scalar loads)
    auto group_of = [&](int L) {
        int g = 0;
        while (g + 1 < p.ngroups && L >= p.groups[g + 1].start * p.nrg) ++g;
        return g;
    };
    const unsigned lds0 = (unsigned)(size_t)(wino_lds_void*)smem;

    // ---- issue side: task L -> (row group rg fastest, pixel tile, sample) ----------------------------------------------------------
    unsigned vp[NPD];                       // patch units of this thread: channel u / (PXB / 4), pixels 4 (u % (PXB / 4)) ...
    const bool a_wave = wave < RT * 2;      // waves whose threads copy A units (the others park their DMA in the scratch line)
    int it = lb, is = 0;
    wino_u32x4 d_in, d_a;
    unsigned so_in = 0, so_a = 0;
    int HW = p.HW;                          // pixels per channel plane of the task the issue side serves
    auto issue_task = [&]() {
        int rg, pt, ib;
        const float *tin, *twpk;
        if (p.groups) {
            const int g = group_of(it), local = it - p.groups[g].start * p.nrg;
            rg = local % p.nrg;
            pt = local / p.nrg;
            ib = 0;
            HW = p.groups[g].HW;
            tin = p.groups[g].in;
            twpk = p.groups[g].wpk;
        } else {
            rg = it % p.nrg;
            pt = (it / p.nrg) % p.npt;
            ib = it / (p.nrg * p.npt);
            tin = p.in;
            twpk = p.wpk;
        }
#pragma unroll
        for (int i = 0; i < NPD; ++i) {
            const int u = i * 512 + tid, ch = u / (PXB / 4), q = u - ch * (PXB / 4);
            vp[i] = (unsigned)(ch * HW + pt * PXB + 4 * q) * 4u;
        }
        d_in = wino_rsrc(tin + (long long)ib * (p.in_bs ? p.in_bs : (long long)p.Cin * HW), (unsigned)p.Cin * HW * 4u);
        // the RT row tiles of a group are consecutive images of nst * 2 KB each: thread tid copies unit (tid & 127) of row tile tid >> 7
        const int nrt = (p.Cout + 31) / 32, have = nrt - rg * RT < RT ? nrt - rg * RT : RT;       // (last group may be partial)
        d_a = wino_rsrc(twpk + (long long)rg * RT * nst * 512, (unsigned)have * nst * 2048u);
        so_in = 0;
        so_a = 0;
    };
    issue_task();
    const unsigned va_rt = a_wave ? (unsigned)((tid >> 7) * nst * 2048 + (tid & 127) * 16) : 0x80000000u;
    unsigned islot = lds0;
    auto issue = [&]() {
        const unsigned wb = islot + (unsigned)wave * 1024u;
#pragma unroll
        for (int i = 0; i < NPD; ++i) wino_dma16(vp[i], d_in, so_in, wb + (unsigned)i * 8192u);
        // A: threads 0 .. RT*128-1 fill the stage's A area in order; the others park their 16 bytes in the scratch line
        const unsigned wa = a_wave ? islot + PDW * 4u + (unsigned)wave * 1024u : lds0 + RING + (unsigned)wave * 1024u;
        wino_dma16(va_rt, d_a, so_a, wa);
        islot = islot + SB == lds0 + RING ? lds0 : islot + SB;
        so_in += 64u * (unsigned)HW;
        so_a += 2048u;
        if (++is == nst) {
            if (it + G < p.ntasks) {
                it += G;
                is = 0;
                issue_task();
            } else {
                is = nst - 1;
                so_in -= 64u * (unsigned)HW;
                so_a -= 2048u;
            }
        }
    };

    // ---- consumer side: wave = row tile (wave / PG) x pixel group (wave % PG) ---------------------------------------------------
    f32x16 acc[2];
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
    const int rtl = wave / PG, pg = wave % PG;
    const int boff = (lane >> 5) * PXB + pg * 64 + (lane & 31);            // B fragment origin: channel parity plane, pixel
    const int aoff = PDW + rtl * 512 + lane * 8;

#pragma unroll
    for (int j = 0; j < NST - 1; ++j) issue();
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD * (NST - 3)) : "memory");
    __syncthreads();
    unsigned rslot = lds0;
    bool after_epi = false;
    auto frag = [&](unsigned slot) { return reinterpret_cast<const float*>(smem) + (slot - lds0) / 4; };
    float4 a_lo = *reinterpret_cast<const float4*>(frag(lds0) + aoff), a_hi = *reinterpret_cast<const float4*>(frag(lds0) + aoff + 4);
    float b0 = frag(lds0)[boff], b1 = frag(lds0)[boff + 32];
    const int nrt_all = (p.Cout + 31) / 32;
    // row group of task L (grouped launch: local task -> row group fastest)
    auto row_group = [&](int L) { return (p.groups ? L - p.groups[group_of(L)].start * p.nrg : L) % p.nrg; };
    for (int k = 0, ct = lb; k < mytasks; ++k, ct += G) {
        // a wave whose row tile lies beyond Cout (last row group) multiplies nothing: it keeps issuing its DMAs and meets every barrier
        const bool live = row_group(ct) * RT + rtl < nrt_all;
        const bool live_next = k + 1 < mytasks && row_group(ct + G) * RT + rtl < nrt_all;
        for (int cs = 0; cs < nst; ++cs) {
            if (after_epi) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD * (NST - 3)) : "memory");
            __syncthreads();
            after_epi = false;
            issue();
            const unsigned nslot = rslot + SB == lds0 + RING ? lds0 : rslot + SB;
            const float* sp = frag(rslot);
            const float* spn = frag(nslot);
            if (!live) {                                                    // (wave-uniform)
                if (cs == nst - 1 && live_next) {                           // first fragments of the next task
                    b0 = spn[boff];
                    b1 = spn[boff + 32];
                    a_lo = *reinterpret_cast<const float4*>(spn + aoff);
                    a_hi = *reinterpret_cast<const float4*>(spn + aoff + 4);
                }
                rslot = nslot;
                continue;
            }
            const float av[8] = {a_lo.x, a_lo.y, a_lo.z, a_lo.w, a_hi.x, a_hi.y, a_hi.z, a_hi.w};
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const float c0 = b0, c1 = b1;
                if (s < 7) {
                    b0 = sp[boff + (2 * s + 2) * PXB];
                    b1 = sp[boff + (2 * s + 2) * PXB + 32];
                } else {                                                    // the next stage was verified by the barrier above
                    b0 = spn[boff];
                    b1 = spn[boff + 32];
                    a_lo = *reinterpret_cast<const float4*>(spn + aoff);
                    a_hi = *reinterpret_cast<const float4*>(spn + aoff + 4);
                }
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], c0, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], c1, acc[1], 0, 0, 0);
            }
            rslot = nslot;
        }
        // ---- epilogue: 32 rows x 64 pixels per wave, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5), pixel lane & 31 -------------------
        if (live) {
            int rg, pt, b, eHW;
            float* tout;
            if (p.groups) {
                const int g = group_of(ct), local = ct - p.groups[g].start * p.nrg;
                rg = local % p.nrg;
                pt = local / p.nrg;
                b = 0;
                eHW = p.groups[g].HW;
                tout = p.groups[g].out;
            } else {
                rg = ct % p.nrg;
                pt = (ct / p.nrg) % p.npt;
                b = ct / (p.nrg * p.npt);
                eHW = p.HW;
                tout = p.out;
            }
            const int row0 = (rg * RT + rtl) * 32 + 4 * (lane >> 5);
            float* ob = tout + (long long)b * p.Cout * eHW + pt * PXB + pg * 64 + (lane & 31);
#pragma unroll
            for (int n = 0; n < 2; ++n)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = row0 + (r & 3) + 8 * (r >> 2);
                    if (row < p.Cout) ob[(long long)row * eHW + n * 32] = acc[n][r];
                    acc[n][r] = 0.f;
                }
            after_epi = true;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // no LDS-DMA may outlive the block
}

// WIDE wave tiles (PwParams::wide): a wave owns a row PAIR = 64 rows x 64 pixels (four 32x32 accumulators), so every B register feeds
// two MFMAs and a barrier interval holds 32 MFMAs per wave.  8 waves = RP row pairs x (8 / RP) pixel groups:
//   RP = 2: 128 rows x 256 pixels, stage = 16 KB of input + 8 KB of A (the four row-tile images of pack_pw_A, unchanged), ring of six;
//   RP = 1:  64 rows x 512 pixels, stage = 32 KB + 4 KB, ring of four (Cout = 64).
// The row pair sits in the upper wave bits (rp = wave / PG, PG = 4 at RP = 2): the two waves of a SIMD (w, w + 4) belong to different
// row pairs.  Every output element is the same accumulator chain over the same k-steps as in pw_conv_kernel: identical bits.
// Grouped launch: every group's HW % PXB == 0; PwGroup::start stays in tiles of 128 pixels (start / (PXB / 128) tiles of this kernel).
template <int RP>
struct PwWideCfg {
    static constexpr int PG = 8 / RP, PXB = 64 * PG;             // pixel groups of 64 per block, pixels per block
    static constexpr int RTB = 2 * RP;                            // row tiles per block
    static constexpr int PDW = 16 * PXB, ADW = RTB * 512;         // patch / A dwords per stage
    static constexpr int SDW = PDW + ADW, NST = RP == 2 ? 6 : 4;
    static constexpr int NPD = PDW / (4 * 512);                   // patch DMAs (16 B) per thread per stage: 2 (RP = 2) / 4 (RP = 1)
    static constexpr int NLD = NPD + 1;
    static constexpr int LDS_BYTES = NST * SDW * 4 + 512 * 16;    // + a scratch line per thread for the A DMA of idle threads
};

template <int RP>
__global__ __launch_bounds__(512, 1) void pw_conv_wide_kernel(const PwParams p) {
    using Cfg = PwWideCfg<RP>;
    constexpr int PG = Cfg::PG, PXB = Cfg::PXB, RTB = Cfg::RTB, PDW = Cfg::PDW, SDW = Cfg::SDW, NST = Cfg::NST, NPD = Cfg::NPD, NLD = Cfg::NLD;
    constexpr int PXS = PXB / 128;          // PwGroup::start counts tiles of 128 pixels
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int G = gridDim.x;
    const int lb = xcd_remap(blockIdx.x, G);
    if (lb >= p.ntasks) return;
    if (p.skip && *p.skip) return;          // (code memo: every group's output still holds the LUT of these codes)
    const int mytasks = (p.ntasks - lb + G - 1) / G;
    const int nst = p.nst;
    constexpr unsigned SB = SDW * 4, RING = NST * SB;
    auto group_of = [&](int L) {
        int g = 0;
        while (g + 1 < p.ngroups && L >= p.groups[g + 1].start / PXS * p.nrg) ++g;
        return g;
    };
    const unsigned lds0 = (unsigned)(size_t)(wino_lds_void*)smem;

    // ---- issue side: task L -> (row group rg fastest, pixel tile, sample) ----------------------------------------------------------
    unsigned vp[NPD];                       // patch units of this thread: channel u / (PXB / 4), pixels 4 (u % (PXB / 4)) ...
    const bool a_wave = wave < RTB * 2;     // waves whose threads copy A units (the others park their DMA in the scratch line)
    int it = lb, is = 0;
    wino_u32x4 d_in, d_a;
    unsigned so_in = 0, so_a = 0;
    int HW = p.HW;
    const int nrt_all = (p.Cout + 31) / 32;
    auto issue_task = [&]() {
        int rg, pt, ib;
        const float *tin, *twpk;
        if (p.groups) {
            const int g = group_of(it), local = it - p.groups[g].start / PXS * p.nrg;
            rg = local % p.nrg;
            pt = local / p.nrg;
            ib = 0;
            HW = p.groups[g].HW;
            tin = p.groups[g].in;
            twpk = p.groups[g].wpk;
        } else {
            rg = it % p.nrg;
            pt = (it / p.nrg) % p.npt;
            ib = it / (p.nrg * p.npt);
            tin = p.in;
            twpk = p.wpk;
        }
#pragma unroll
        for (int i = 0; i < NPD; ++i) {
            const int u = i * 512 + tid, ch = u / (PXB / 4), q = u - ch * (PXB / 4);
            vp[i] = (unsigned)(ch * HW + pt * PXB + 4 * q) * 4u;
        }
        d_in = wino_rsrc(tin + (long long)ib * (p.in_bs ? p.in_bs : (long long)p.Cin * HW), (unsigned)p.Cin * HW * 4u);
        // the RTB row tiles of a group are consecutive images of nst * 2 KB each; images beyond the last row tile read as zeros
        const int have = nrt_all - rg * RTB < RTB ? nrt_all - rg * RTB : RTB;
        d_a = wino_rsrc(twpk + (long long)rg * RTB * nst * 512, (unsigned)have * nst * 2048u);
        so_in = 0;
        so_a = 0;
    };
    issue_task();
    const unsigned va_rt = a_wave ? (unsigned)((tid >> 7) * nst * 2048 + (tid & 127) * 16) : 0x80000000u;
    unsigned islot = lds0;
    auto issue = [&]() {
        const unsigned wb = islot + (unsigned)wave * 1024u;
#pragma unroll
        for (int i = 0; i < NPD; ++i) wino_dma16(vp[i], d_in, so_in, wb + (unsigned)i * 8192u);
        const unsigned wa = a_wave ? islot + PDW * 4u + (unsigned)wave * 1024u : lds0 + RING + (unsigned)wave * 1024u;
        wino_dma16(va_rt, d_a, so_a, wa);
        islot = islot + SB == lds0 + RING ? lds0 : islot + SB;
        so_in += 64u * (unsigned)HW;
        so_a += 2048u;
        if (++is == nst) {
            if (it + G < p.ntasks) {
                it += G;
                is = 0;
                issue_task();
            } else {
                is = nst - 1;
                so_in -= 64u * (unsigned)HW;
                so_a -= 2048u;
            }
        }
    };

    // ---- consumer side: wave = row pair (wave / PG) x pixel group (wave % PG); acc[row tile of the pair][pixel half] ------------------
    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][n][r] = 0.f;
    const int rp = wave / PG, pg = wave % PG;
    const int boff = (lane >> 5) * PXB + pg * 64 + (lane & 31);            // B fragment origin: channel parity plane, pixel
    const int aoff = PDW + 2 * rp * 512 + lane * 8;                         // row tile 2 rp; 2 rp + 1: + 512

#pragma unroll
    for (int j = 0; j < NST - 1; ++j) issue();
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD * (NST - 3)) : "memory");
    __syncthreads();
    unsigned rslot = lds0;
    bool after_epi = false;
    auto frag = [&](unsigned slot) { return reinterpret_cast<const float*>(smem) + (slot - lds0) / 4; };
    float4 a0_lo, a0_hi, a1_lo, a1_hi;
    float b0, b1;
    auto first_frags = [&](const float* f) {
        b0 = f[boff];
        b1 = f[boff + 32];
        a0_lo = *reinterpret_cast<const float4*>(f + aoff);
        a0_hi = *reinterpret_cast<const float4*>(f + aoff + 4);
        a1_lo = *reinterpret_cast<const float4*>(f + aoff + 512);
        a1_hi = *reinterpret_cast<const float4*>(f + aoff + 516);
    };
    first_frags(frag(lds0));
    auto row_group = [&](int L) { return (p.groups ? L - p.groups[group_of(L)].start / PXS * p.nrg : L) % p.nrg; };
    for (int k = 0, ct = lb; k < mytasks; ++k, ct += G) {
        // a wave whose row tiles both lie beyond Cout (last row group) multiplies nothing: it keeps issuing its DMAs and meets every barrier
        const bool live = row_group(ct) * RTB + 2 * rp < nrt_all;
        const bool live_next = k + 1 < mytasks && row_group(ct + G) * RTB + 2 * rp < nrt_all;
        for (int cs = 0; cs < nst; ++cs) {
            if (after_epi) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD * (NST - 3)) : "memory");
            __syncthreads();
            after_epi = false;
            issue();
            const unsigned nslot = rslot + SB == lds0 + RING ? lds0 : rslot + SB;
            const float* sp = frag(rslot);
            const float* spn = frag(nslot);
            rslot = nslot;
            if (!live) {                                                    // (wave-uniform)
                if (cs == nst - 1 && live_next) first_frags(spn);
                continue;
            }
            const float av0[8] = {a0_lo.x, a0_lo.y, a0_lo.z, a0_lo.w, a0_hi.x, a0_hi.y, a0_hi.z, a0_hi.w};
            const float av1[8] = {a1_lo.x, a1_lo.y, a1_lo.z, a1_lo.w, a1_hi.x, a1_hi.y, a1_hi.z, a1_hi.w};
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const float c0 = b0, c1 = b1;
                if (s < 7) {
                    b0 = sp[boff + (2 * s + 2) * PXB];
                    b1 = sp[boff + (2 * s + 2) * PXB + 32];
                } else first_frags(spn);                                    // the next stage was verified by the barrier above
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], c0, acc[0][0], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], c0, acc[1][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[s], c1, acc[0][1], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[s], c1, acc[1][1], 0, 0, 0);
            }
        }
        // ---- epilogue: 64 rows x 64 pixels per wave, rows 32 t + (r & 3) + 8 (r >> 2) + 4 (lane >> 5), pixel lane & 31 -----------------
        if (live) {
            int rg, pt, b, eHW;
            float* tout;
            if (p.groups) {
                const int g = group_of(ct), local = ct - p.groups[g].start / PXS * p.nrg;
                rg = local % p.nrg;
                pt = local / p.nrg;
                b = 0;
                eHW = p.groups[g].HW;
                tout = p.groups[g].out;
            } else {
                rg = ct % p.nrg;
                pt = (ct / p.nrg) % p.npt;
                b = ct / (p.nrg * p.npt);
                eHW = p.HW;
                tout = p.out;
            }
            const int row0 = (rg * RTB + 2 * rp) * 32 + 4 * (lane >> 5);
            float* ob = tout + (long long)b * p.Cout * eHW + pt * PXB + pg * 64 + (lane & 31);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int n = 0; n < 2; ++n)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = row0 + 32 * t + (r & 3) + 8 * (r >> 2);
                        if (row < p.Cout) ob[(long long)row * eHW + n * 32] = acc[t][n][r];
                        acc[t][n][r] = 0.f;
                    }
            after_epi = true;
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // no LDS-DMA may outlive the block
}

inline bool pw_supported(int Cin, int Cout, int HW) { return Cin % 16 == 0 && HW % 256 == 0 && Cout >= 32; }
// the kernel of a plain launch: 0 = pw_conv_kernel, else RP of pw_conv_wide_kernel.  128 x 256 tiles from three row tiles on; the two
// row tiles of Cout = 64 as one row pair x 512 pixels (128 -> 64 at 512^2, HBM-bound: 0.76 against 0.92 ms, profiles/r12_pw_wide.md)
inline int pw_wide_rule(int wide, int Cout, int HW) {
    if (!wide || HW % 256 || Cout < 64) return 0;
    if (Cout > 64) return 2;
    return HW % 512 == 0 ? 1 : 0;
}
hipError_t conv_pw(PwParams p, hipStream_t s);              // conv_inst_wino.hip
// grouped launch: p.groups / p.ngroups (device array), p.Cin, p.Cout; ntasks = (sum of the groups' pixel tiles) x row groups
inline int pw_group_tasks(int Cout, int HW) { return ((((Cout + 31) / 32) + 3) / 4) * (HW / 128); }
hipError_t conv_pw_grouped(PwParams p, int ntasks, hipStream_t s);

}  // namespace chk
