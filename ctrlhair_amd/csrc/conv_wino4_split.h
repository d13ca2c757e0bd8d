// conv_wino4_split.h -- wino4_plain_kernel (conv_wino4.h) with the 36 Winograd positions, not the 32 GEMM rows, split between the two
// waves that share a group of 16 tiles.  Wave (jh, tg) accumulates the 18 positions xi = 6 i + j with j in {3 jh, 3 jh + 1, 3 jh + 2}
// for BOTH 16-row halves: again 36 accumulators of 16x16 and 36 MFMAs per k-step, every B register feeding two of them.  What it saves
// is the input transform: a wave needs only its three outputs of each patch row (wino4_in1d_half: 5 / 6 operations instead of 12, from
// five of the six patch columns -- one halo read per row instead of two) and three column transforms instead of six: about 70 vector
// operations and 12 LDS reads per k-step where wino4_plain_kernel has 144 and 18, and nothing is exchanged inside the k-loop.
//
// The price is paid once per task.  The output transform's second pass (wino4_out1d over j) needs all six j of a (row, tile); it is two
// independent halves that meet in the last operation of each output, so the jh = 0 wave forms (m0 + s1, s1, d1), the jh = 1 wave
// (s2, d2, m5), each wave sends the triples of the row half it does NOT finalise to its partner (12 floats per (row, tile): 48 per lane)
// and combines the other half with exactly wino4_out1d's last four operations: every output bit equals wino4_plain_kernel's.
//
// LDS for the exchange: after a task's last k-step q, and one block barrier, stage q mod 4 of the ring is dead (its A image was consumed
// in k-step q, its patch in q - 1; the next DMA into it is issued behind the top barrier of k-step q + 1) and so is the patch half of
// stage (q + 1) mod 4 (transformed into registers during k-step q; rewritten in k-step q + 2).  Four rounds, one per accumulator row of
// the lane: write 3 units of 16 bytes ([unit][lane]: conflict-free), barrier, read the partner's.  Rounds alternate between two regions
// of 8 x 3 KB, so the barrier of round e also orders the reads of round e - 1 before the writes of round e + 1: five barriers per task.
//
// A operand: the same U values in another fragment order (pack_wino4_A(..., split = true): wino4_split_frag), the nine units of a wave
// contiguous; image size, DMA issue side, ring, counted waits and task order are those of wino4_plain_kernel.
#pragma once
#include "conv_wino4.h"

namespace chk {

// the wave's three outputs of wino4_in1d: r0, r1, r2 (JH = 0, from d0 .. d4) or r3, r4, r5 (JH = 1, from d1 .. d5), the same expressions
template <int JH>
__device__ __forceinline__ void wino4_in1d_half(const float (&d)[6], float& o0, float& o1, float& o2) {
    if constexpr (JH == 0) {
        const float a = __builtin_fmaf(-4.f, d[2], d[4]), b = __builtin_fmaf(-4.f, d[1], d[3]);
        o0 = __builtin_fmaf(4.f, d[0], __builtin_fmaf(-5.f, d[2], d[4]));
        o1 = a + b;
        o2 = a - b;
    } else {
        const float c = d[4] - d[2], t = d[3] - d[1];
        o0 = __builtin_fmaf(2.f, t, c);
        o1 = __builtin_fmaf(-2.f, t, c);
        o2 = __builtin_fmaf(4.f, d[1], __builtin_fmaf(-5.f, d[3], d[5]));
    }
}
// wino4_out1d up to its last operation per output: (m0, m1, m2) -> (m0 + s1, s1, d1) or (m3, m4, m5) -> (s2, d2, m5) ...
template <int JH>
__device__ __forceinline__ void wino4_out1d_part(float a, float b, float c, float& p0, float& p1, float& p2) {
    if constexpr (JH == 0) {
        const float s1 = b + c, d1 = b - c;
        p0 = a + s1; p1 = s1; p2 = d1;
    } else {
        p0 = a + b; p1 = a - b; p2 = c;
    }
}
// ... and those last operations
__device__ __forceinline__ void wino4_out1d_join(float m0s1, float s1, float d1, float s2, float d2, float m5, float& y0, float& y1, float& y2, float& y3) {
    y0 = m0s1 + s2;
    y1 = __builtin_fmaf(2.f, d2, d1);
    y2 = __builtin_fmaf(4.f, s2, s1);
    y3 = __builtin_fmaf(8.f, d2, d1) + m5;
}

// One wave's program: JH is the wave's half of the positions.  Both programs execute the same sequence of barriers and DMAs.
template <int MODE, int JH>
__device__ __forceinline__ void wino4_split_body(const Wino4Params& p, float* smem, const int wave) {
    using namespace wino4;
    constexpr bool REFL = (MODE & 1) != 0;
    const int tid = threadIdx.x, lane = tid & 63;
    const int n = lane & 15, kk = lane >> 4;
    const int tg = wave & 3;
    const int G = gridDim.x;
    const int lb = xcd_remap(blockIdx.x, G);
    if (lb >= p.ntasks) return;
    const int mytasks = (p.ntasks - lb + G - 1) / G;
    const int nk = p.nks;
    const int HW = p.H * p.W;
    constexpr unsigned SB = SUNITS * 16u, RING = NST * SB;
    const unsigned lds0 = (unsigned)(size_t)(wino_lds_void*)smem;

    auto task_of = [&](int L, int& rt, int& tile) {      // as wino4_plain_kernel
        const int per = p.tbk * p.nrt;
        const int tgr = L / per;
        int r = L - tgr * per;
        const int tgsz = min(p.tbk, p.ntiles - tgr * p.tbk);
        const int rg = r / (tgsz * p.rb);
        r -= rg * tgsz * p.rb;
        const int rgsz = min(p.rb, p.nrt - rg * p.rb);
        const int tl = r / rgsz;
        rt = rg * p.rb + (r - tl * rgsz);
        tile = tgr * p.tbk + tl;
    };

    // ---- issue side: wino4_plain_kernel's, on the split image ----------------------------------------------------------------------
    unsigned voff[3];
    const unsigned va = (unsigned)tid * 16u;
    int it = lb, is = 0;
    wino_u32x4 d_in, d_a;
    unsigned so_in = 0, so_a = 0;
    auto issue_task = [&]() {
        int irt, tile;
        task_of(it, irt, tile);
        const int tx = tile % p.ntx, ty = (tile / p.ntx) % p.nty, ib = tile / (p.ntx * p.nty);
        const int y0 = ty * TS - 1, x0 = tx * TS - 4;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int u = i * 512 + tid;
            const int k4 = u / PPL, rem = u - k4 * PPL;
            const int py = rem / PUN, ux = rem - py * PUN;
            int y = y0 + py;
            const int x = x0 + 4 * ux;
            if constexpr (REFL) y = y < 0 ? -y : (y >= p.H ? 2 * p.H - 2 - y : y);
            const bool ok = u < PUNITS && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
            voff[i] = ok ? (unsigned)(k4 * HW + y * p.W + x) * 4u : 0x80000000u;
        }
        d_in = wino_rsrc(p.in + (long long)ib * p.Cin * HW, (unsigned)p.Cin * HW * 4u);
        d_a = wino_rsrc(p.wpk_split + (long long)irt * p.nks * ADW, (unsigned)p.nks * ADW * 4u);
        so_in = 0;
        so_a = 0;
    };
    issue_task();
    unsigned islot = lds0;
    auto issue_piece = [&](auto pt) {
        constexpr int pc = decltype(pt)::value;
        const unsigned wb = islot + (unsigned)wave * 1024u;
        if constexpr (pc < 2) wino_dma16(voff[pc], d_in, so_in, wb + (unsigned)pc * 8192u);
        else wino_dma16(va, d_a, so_a + (unsigned)(pc - 2) * 8192u, wb + PSLOTS * 16u + (unsigned)(pc - 2) * 8192u);
    };
    auto issue_tail = [&]() {
        const unsigned wb = islot + (unsigned)wave * 1024u;
        if (wave < 6) wino_dma16(voff[2], d_in, so_in, wb + 2u * 8192u);
        if (wave < 2) wino_dma16(va, d_a, so_a + 2u * 8192u, wb + PSLOTS * 16u + 2u * 8192u);
        islot = islot + SB == lds0 + RING ? lds0 : islot + SB;
        so_in += 16u * (unsigned)HW;
        so_a += (unsigned)ADW * 4u;
        if (++is == nk) {
            if (it + G < p.ntasks) {
                it += G;
                is = 0;
                issue_task();
            } else {                   // past the end: keep re-issuing the last k-step (never read; keeps the vmcnt counting uniform)
                is = nk - 1;
                so_in -= 16u * (unsigned)HW;
                so_a -= (unsigned)ADW * 4u;
            }
        }
    };
    auto issue_kstep = [&]() {
        issue_piece(WInt<0>{}); issue_piece(WInt<1>{}); issue_piece(WInt<2>{}); issue_piece(WInt<3>{});
        issue_tail();
    };
    auto wait_ring = [&]() {
        if (wave < 2) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
        else if (wave < 6) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    };

    // ---- consumer side ---------------------------------------------------------------------------------------------------
    f32x4 acc[36];                                // acc[2 q + m]: position q = 3 i + jj (xi = 6 i + 3 JH + jj) of row half m
#pragma unroll
    for (int x = 0; x < 36; ++x) acc[x] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int tx = n & 7, tyl = 2 * tg + (n >> 3);
    const int boff = kk * (PPL * 4) + (4 * tyl) * (PUN * 4) + 4 * tx + 3;
    auto stage = [&](unsigned slot) { return reinterpret_cast<const float*>(smem) + (slot - lds0) / 4; };
    bool eL = false, eR = false;
    auto edge_of = [&](int L, bool& l, bool& r) {
        int rt_, tile_;
        task_of(L < p.ntasks ? L : p.ntasks - 1, rt_, tile_);
        const int ttx_ = tile_ % p.ntx;
        l = ttx_ == 0 && tx == 0;
        r = ttx_ == p.ntx - 1 && tx == 7;
    };
    auto load_row = [&](const float* sp, int r, float (&d)[6]) {      // patch row r: the four middle columns + this wave's halo column
        const float* q = sp + boff + r * (PUN * 4);
        const f32x4 mid = *reinterpret_cast<const f32x4*>(q + 1);
        d[1] = mid.x; d[2] = mid.y; d[3] = mid.z; d[4] = mid.w;
        if constexpr (JH == 0) {
            d[0] = q[0];
            if constexpr (REFL) d[0] = eL ? d[2] : d[0];
        } else {
            d[5] = q[5];
            if constexpr (REFL) d[5] = eR ? d[3] : d[5];
        }
    };
    auto col_transform = [&](float (&vv)[18], int jj) {
        wino4_in1d(vv[jj], vv[3 + jj], vv[6 + jj], vv[9 + jj], vv[12 + jj], vv[15 + jj], vv[jj], vv[3 + jj], vv[6 + jj], vv[9 + jj], vv[12 + jj], vv[15 + jj]);
    };
    auto a_ptr = [&](unsigned slot) { return reinterpret_cast<const f32x4*>(stage(slot) + PSLOTS * 4) + 9 * JH * 64 + lane; };

    issue_kstep();
    issue_kstep();
    issue_kstep();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    float v[18], w[18];                           // B fragments v[3 i + jj]
    if constexpr (REFL) edge_of(lb, eL, eR);
    {   // B fragments of the first k-step
        const float* sp = stage(lds0);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            float d[6];
            load_row(sp, r, d);
            wino4_in1d_half<JH>(d, v[3 * r], v[3 * r + 1], v[3 * r + 2]);
        }
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) col_transform(v, jj);
    }
    unsigned rslot = lds0;
    // one k-step: nine groups of four MFMAs (two positions x two row halves) on the B fragments `vc`; the next k-step's patch -> `vx`
    auto kstep = [&](float (&vc)[18], float (&vx)[18]) {
        wait_ring();
        __syncthreads();
        const unsigned nslot = rslot + SB == lds0 + RING ? lds0 : rslot + SB;
        const f32x4* ap = a_ptr(rslot);
        const float* spn = stage(nslot);
        f32x4 F[2];
        F[0] = ap[0];
        float d[6];
        auto group = [&](auto gt) {
            constexpr int g = decltype(gt)::value;      // positions q = 2 g, 2 g + 1
            if constexpr (g + 1 < 9) F[(g + 1) & 1] = ap[(g + 1) * 64];
            if constexpr (g < 6) load_row(spn, g, d);
            __builtin_amdgcn_sched_barrier(0);
            const f32x4 c = F[g & 1];
            __builtin_amdgcn_s_setprio(1);
            acc[4 * g] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.x, vc[2 * g], acc[4 * g], 0, 0, 0);
            acc[4 * g + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.y, vc[2 * g], acc[4 * g + 1], 0, 0, 0);
            acc[4 * g + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.z, vc[2 * g + 1], acc[4 * g + 2], 0, 0, 0);
            acc[4 * g + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(c.w, vc[2 * g + 1], acc[4 * g + 3], 0, 0, 0);
            __builtin_amdgcn_s_setprio(0);
            if constexpr (g < 6) wino4_in1d_half<JH>(d, vx[3 * g], vx[3 * g + 1], vx[3 * g + 2]);
            if constexpr (g >= 6) col_transform(vx, g - 6);
#ifdef CH_W4_PIN                                    // (the ablation of wino4_pin, conv_wino4.h)
            if constexpr (g < 6) {
                wino4_pin(vx[3 * g]); wino4_pin(vx[3 * g + 1]); wino4_pin(vx[3 * g + 2]);
            } else {
#pragma unroll
                for (int i = 0; i < 6; ++i) wino4_pin(vx[3 * i + g - 6]);
            }
#endif
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (g >= 2 && g < 6) issue_piece(WInt<g - 2>{});
            __builtin_amdgcn_sched_barrier(0);
        };
        group(WInt<0>{}); group(WInt<1>{}); group(WInt<2>{}); group(WInt<3>{}); group(WInt<4>{}); group(WInt<5>{});
        group(WInt<6>{}); group(WInt<7>{}); group(WInt<8>{});
        issue_tail();
        rslot = nslot;
    };

    for (int k = 0, ct = lb; k < mytasks; ++k, ct += G) {
        for (int cs = 0; cs < nk; cs += 2) {
            kstep(v, w);          // (nks is even: the launcher)
            if constexpr (REFL)
                if (cs + 2 >= nk) edge_of(ct + G, eL, eR);
            kstep(w, v);
        }
        // ---- epilogue of task ct: this wave finalises row half JH and sends its triples of the other half ---------------------------
        int crt, tile;
        task_of(ct, crt, tile);
        const int ttx = tile % p.ntx, tty = (tile / p.ntx) % p.nty, b = tile / (p.ntx * p.nty);
        const int y = tty * TS + 4 * tyl, x = ttx * TS + 4 * tx;
        const int rW = p.W >> p.res_up, rHW = rW * (p.H >> p.res_up);
        // exchange areas of 3 KB per wave: region 0 = the dead stage [0, 24 KB); region 1 = waves 0-4: the dead stage [24 KB, 39 KB),
        // waves 5-7: the patch half of the stage after it [0, 9 KB)
        const unsigned dslot = rslot == lds0 ? lds0 + RING - SB : rslot - SB;
        auto area = [&](int par, int wv) {
            const unsigned o = par == 0 ? dslot + (unsigned)wv * 3072u : (wv < 5 ? dslot + 24576u + (unsigned)wv * 3072u : rslot + (unsigned)(wv - 5) * 3072u);
            return reinterpret_cast<f32x4*>(smem) + ((o - lds0) >> 4) + lane;
        };
        f32x4* const xw[2] = {area(0, wave), area(1, wave)};
        const f32x4* const xr[2] = {area(0, wave ^ 4), area(1, wave ^ 4)};
        __syncthreads();                             // every wave is through the task's last k-step
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = crt * 32 + JH * 16 + 4 * kk + e, rc = row < p.Cout ? row : p.Cout - 1;
            const float bsv = p.bias ? p.bias[rc] : 0.f;
            f32x4 rr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) rr[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (p.res) {
                const float* rp = p.res + ((long long)b * p.Cout + rc) * rHW;
                if (p.res_up) {
#pragma unroll
                    for (int r2 = 0; r2 < 2; ++r2) {
                        const float2 q2 = *reinterpret_cast<const float2*>(rp + ((y >> 1) + r2) * rW + (x >> 1));
                        rr[2 * r2] = rr[2 * r2 + 1] = (f32x4){q2.x, q2.x, q2.y, q2.y};
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) rr[r] = *reinterpret_cast<const f32x4*>(rp + (y + r) * rW + x);
                }
            }
            float P[2][12];                          // P[m][3 r + .]: the wave's triple of output row r, row half m
#pragma unroll
            for (int m = 0; m < 2; ++m) {
                float t[4][3];                       // first pass (over i), wave-local
#pragma unroll
                for (int jj = 0; jj < 3; ++jj)
                    wino4_out1d(acc[2 * jj + m][e], acc[2 * (3 + jj) + m][e], acc[2 * (6 + jj) + m][e], acc[2 * (9 + jj) + m][e], acc[2 * (12 + jj) + m][e],
                                acc[2 * (15 + jj) + m][e], t[0][jj], t[1][jj], t[2][jj], t[3][jj]);
#pragma unroll
                for (int r = 0; r < 4; ++r) wino4_out1d_part<JH>(t[r][0], t[r][1], t[r][2], P[m][3 * r], P[m][3 * r + 1], P[m][3 * r + 2]);
            }
#pragma unroll
            for (int u = 0; u < 3; ++u) xw[e & 1][u * 64] = (f32x4){P[1 - JH][4 * u], P[1 - JH][4 * u + 1], P[1 - JH][4 * u + 2], P[1 - JH][4 * u + 3]};
            __syncthreads();
            float Q[12];                             // the partner's triples of row half JH
#pragma unroll
            for (int u = 0; u < 3; ++u) {
                const f32x4 q4 = xr[e & 1][u * 64];
                Q[4 * u] = q4.x; Q[4 * u + 1] = q4.y; Q[4 * u + 2] = q4.z; Q[4 * u + 3] = q4.w;
            }
            const float(&L)[12] = JH == 0 ? P[0] : Q;      // (m0 + s1, s1, d1)
            const float(&R)[12] = JH == 0 ? Q : P[1];      // (s2, d2, m5)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float o0, o1, o2, o3;
                wino4_out1d_join(L[3 * r], L[3 * r + 1], L[3 * r + 2], R[3 * r], R[3 * r + 1], R[3 * r + 2], o0, o1, o2, o3);
                f32x4 o = {o0 + bsv + rr[r].x, o1 + bsv + rr[r].y, o2 + bsv + rr[r].z, o3 + bsv + rr[r].w};
                if (p.act != ACT_NONE) {
                    o.x = apply_act(o.x, p.act); o.y = apply_act(o.y, p.act);
                    o.z = apply_act(o.z, p.act); o.w = apply_act(o.w, p.act);
                }
                if (row < p.Cout) *reinterpret_cast<f32x4*>(p.out + ((long long)b * p.Cout + row) * HW + (y + r) * p.W + x) = o;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int x2 = 0; x2 < 36; ++x2) acc[x2] = (f32x4){0.f, 0.f, 0.f, 0.f};
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// MODE bit 0: reflection padding, as wino4_plain_kernel (the left edge's replacement touches only the jh = 0 waves, the right edge's
// only jh = 1).  p.wpk_split = the pack_wino4_A(..., split = true) image.
template <int MODE>
__global__ __launch_bounds__(512, 1) void wino4_plain_split_kernel(const Wino4Params p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (wave < 4) wino4_split_body<MODE, 0>(p, smem, wave);
    else wino4_split_body<MODE, 1>(p, smem, wave);
}

}  // namespace chk
