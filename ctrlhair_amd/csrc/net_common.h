// net_common.h -- shared host-side helpers of the model files: host tensor store, weight upload, MFMA operand
// packing, and the plain convs of every net: ONE layer type (ConvLayer: each weight image a route may read), ONE route
// decision of the exact-f32 path (ConvRoute / conv_route: F(4x4,3x3) with or without the pre-transformed input, F(2x2,3x3),
// 1x1 GEMM, direct kernel), ONE launcher (run_conv) and its profile figures (conv_figures), and ONE filler of the f16x3
// ConvParams (sh16_conv_params).  The SEAN generator, the Zencoder, the shape nets and BiSeNet all launch through these.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "conv_mfma.h"
#include "conv_pw.h"
#include "conv_sh16.h"
#include "conv_wino.h"
#include "conv_wino4v.h"

namespace chk {

struct HostTensor {
    std::vector<char> data;
    std::vector<int64_t> shape;
    int dtype = 0;  // 0 f32, 1 i64
    const float* f32() const { return reinterpret_cast<const float*>(data.data()); }
    size_t numel() const {
        size_t n = 1;
        for (auto d : shape) n *= (size_t)d;
        return n;
    }
};
typedef std::map<std::string, HostTensor> TensorStore;

struct Builder {
    const TensorStore& ts;
    std::vector<void*>& allocs;
    std::string err;
    std::string prefix;   // prepended to every tensor name looked up
    Builder(const TensorStore& t, std::vector<void*>& a) : ts(t), allocs(a) {}

    bool has(const std::string& n) const { return ts.find(prefix + n) != ts.end(); }
    const HostTensor* get(const std::string& n0, size_t numel) {
        const std::string n = prefix + n0;
        auto it = ts.find(n);
        if (it == ts.end()) {
            if (err.empty()) err = "missing tensor '" + n + "'";
            return nullptr;
        }
        if (it->second.dtype != 0 || it->second.numel() != numel) {
            if (err.empty())
                err = "tensor '" + n + "' has wrong dtype/size (" + std::to_string(it->second.numel()) + " vs " +
                      std::to_string(numel) + ")";
            return nullptr;
        }
        return &it->second;
    }
    std::vector<float> vec(const std::string& n, size_t numel) {
        auto t = get(n, numel);
        return t ? std::vector<float>(t->f32(), t->f32() + numel) : std::vector<float>(numel, 0.f);
    }
    float* upload(const std::vector<float>& v) {
        void* d = nullptr;
        if (hipMalloc(&d, v.size() * sizeof(float) + 64) != hipSuccess) {
            if (err.empty()) err = "hipMalloc failed (weights)";
            return nullptr;
        }
        allocs.push_back(d);
        if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)
            if (err.empty()) err = "hipMemcpy failed (weights)";
        return static_cast<float*>(d);
    }
    void* dalloc(size_t bytes) {
        void* d = nullptr;
        if (hipMalloc(&d, bytes + 256) != hipSuccess) {
            if (err.empty()) err = "hipMalloc failed (workspace, " + std::to_string(bytes >> 20) + " MiB)";
            return nullptr;
        }
        allocs.push_back(d);
        return d;
    }
    float* falloc(size_t floats) { return static_cast<float*>(dalloc(floats * 4)); }
};

// Pack GEMM rows into the per-lane A-fragment order conv_mfma_kernel streams:
//   [wave tile (64 rows)][chunk][k-group (4 k-steps)][M-subtile (2)][lane (64)][4 floats]
//   lane l holds row (l&31) of its M-subtile, channel parity (l>>5); k-step s = tap*(CK/2) + channel pair.
template <class F>
std::vector<float> pack_A(int rows, int Cin, int KS, int CK, F get) {
    int mt64 = (rows + 63) / 64;
    mt64 = (mt64 + 1) & ~1;   // even number of wave tiles so WM=2 blocks never read past the end
    const int nch = (Cin + CK - 1) / CK;
    const int ksteps = KS * KS * CK / 2, ng = ksteps / 4, half = CK / 2;
    std::vector<float> dst((size_t)mt64 * nch * ng * 2 * 64 * 4, 0.f);
    size_t o = 0;
    for (int mt = 0; mt < mt64; ++mt)
        for (int ch = 0; ch < nch; ++ch)
            for (int g = 0; g < ng; ++g)
                for (int ms = 0; ms < 2; ++ms)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int q = 0; q < 4; ++q, ++o) {
                            const int s = g * 4 + q, t = s / half, cp = s % half;
                            const int row = mt * 64 + ms * 32 + (lane & 31);
                            const int ci = ch * CK + 2 * cp + (lane >> 5);
                            if (row < rows && ci < Cin) dst[o] = get(row, ci, t);
                        }
    return dst;
}

// f16x3 split-operand packing for conv_sh16_kernel:
//   [wave tile 64 rows][chunk 16 ch][tap][M-subtile][hi|lo][lane][8 halfs]; lane l: row (l&31), channels 8*(l>>5)+e
// Every row is scaled by its own power of two 2^k[row] before the hi/lo split so that max|row| * 2^k lies in [2^14, 2^15)
// (sh16.h: an element 2^18 times smaller than the row maximum still keeps 22 significand bits); `wscale[row]` receives the
// exact inverse 2^-k[row], which the consuming epilogue multiplies the accumulator by.  `kmax` (optional, per row) caps
// the exponent (two operands sharing an accumulator must share 2^k * s_in: see sh16_row_exponents).
inline int sh16_row_exponent(float rowmax) {
    if (!(rowmax > 0.f) || !std::isfinite(rowmax)) return 0;
    int e;
    (void)std::frexp(rowmax, &e);          // rowmax = m * 2^e, m in [0.5, 1)
    return 15 - e;                         // rowmax * 2^k in [2^14, 2^15)
}
template <class F>
std::vector<int> sh16_row_exponents(int rows, int Cin, int KS, F get) {
    std::vector<int> k(rows);
    for (int r = 0; r < rows; ++r) {
        float mx = 0.f;
        for (int ci = 0; ci < Cin; ++ci)
            for (int t = 0; t < KS * KS; ++t) mx = std::max(mx, std::fabs(get(r, ci, t)));
        k[r] = sh16_row_exponent(mx);
    }
    return k;
}
template <class F>
std::vector<float> pack_A_sh16(int rows, int Cin, int KS, F get, const std::vector<int>& kexp, bool bf16 = false) {
    const int mt64 = (rows + 63) / 64, nch = (Cin + 15) / 16, nt = KS * KS;
    std::vector<_Float16> dst((size_t)mt64 * nch * nt * 2 * 2 * 64 * 8, (_Float16)0.f);
    size_t o = 0;
    for (int mt = 0; mt < mt64; ++mt)
        for (int ch = 0; ch < nch; ++ch)
            for (int t = 0; t < nt; ++t)
                for (int ms = 0; ms < 2; ++ms) {
                    for (int hl = 0; hl < 2; ++hl)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 8; ++e, ++o) {
                                const int row = mt * 64 + ms * 32 + (lane & 31);
                                const int ci = ch * 16 + (lane >> 5) * 8 + e;
                                if (row < rows && ci < Cin) {
                                    const float w = std::ldexp(get(row, ci, t), kexp[row]);
                                    if (bf16) {            // bf16 single-term mode: hi = bf16 bits (round to nearest even), lo unused
                                        uint32_t u;
                                        std::memcpy(&u, &w, 4);
                                        const uint16_t b = (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
                                        _Float16 hb;
                                        std::memcpy(&hb, &b, 2);
                                        dst[o] = hl == 0 ? hb : (_Float16)0.f;
                                        continue;
                                    }
                                    const _Float16 h = (_Float16)w;
                                    dst[o] = hl == 0 ? h : (_Float16)(w - (float)h);
                                }
                            }
                }
    std::vector<float> out(dst.size() / 2);
    std::memcpy(out.data(), dst.data(), dst.size() * 2);
    return out;
}
// inverse row scales 2^-k, padded to whole 64-row tiles (epilogues read float4 runs)
inline std::vector<float> sh16_wscale(const std::vector<int>& kexp) {
    std::vector<float> v(((kexp.size() + 63) / 64) * 64, 1.f);
    for (size_t r = 0; r < kexp.size(); ++r) v[r] = std::ldexp(1.f, -kexp[r]);
    return v;
}

// ---- the plain conv layer: every weight image a route may read (a handle uploads only those its path and options can reach) ----
struct ConvLayer {
    float* wpk = nullptr;           // exact-f32 direct kernel (conv_mfma.h): pack_A image
    float* bias = nullptr;
    int Cout = 0, Cin = 0, KS = 0, stride = 1, pad = 0;
    float* sh_wpk = nullptr;        // f16x3 kernels (conv_sh16.h): split-operand A fragments (pack_A_sh16) ...
    float* sh_wscale = nullptr;     // ... and the per-row inverse scales 2^-k (sh16.h)
    int s2d_cr = 0, s2d_phase0 = 0; // make_conv_s2d: real (padded) input channels and first phase of the space-to-depth form
    float* wino = nullptr;          // 3x3 stride-1 pad-1, exact f32: Winograd F(2x2,3x3) image U = G g G^T (conv_wino.h) ...
    float* zero = nullptr;          // ... and a few zero words (source of out-of-image patch elements) where the caller has no zero page
    float* wino4 = nullptr;         // the same conv as F(4x4,3x3) (conv_wino4.h) ...
    float* wino4s = nullptr;        // ... and those values in the split kernel's fragment order (conv_wino4_split.h)
    float* pw = nullptr;            // 1x1, exact f32: pack_pw_A image of the GEMM kernel (conv_pw.h)
    int d2s = 0;                    // 1 = GEMM row 4 c + (2 py + px) holds phase (py, px) of channel c: depth-to-space store (a stride-2
                                    //   ConvTranspose2d as four phase convs of the input grid; F(2x2,3x3) only)
};

// w: [Cout][Cin][KS][KS] (already folded: BN / spectral norm / flips), bias may be empty
// want_wino: also pack the Winograd F(2x2,3x3) image (16 / 9 of the weights, packed through a transient host copy in double) -- only
// for layers that can reach a Winograd-sized output (>= 16 x 16) on a handle with aux.wino on (the 4 x 4 layer of the
// shape decoder, 2048 -> 2048, carried 268 MB that no launch ever read)
inline ConvLayer make_conv(Builder& B, const std::vector<float>& w, const std::vector<float>& bias, int cout, int cin,
                           int ks, int stride, int pad, bool want_wino = true) {
    ConvLayer L;
    L.Cout = cout;
    L.Cin = cin;
    L.KS = ks;
    L.stride = stride;
    L.pad = pad;
    const int ck = conv_ck(ks, stride);
    const float* wp = w.data();
    L.wpk = B.upload(pack_A(cout, cin, ks, ck, [&](int row, int ci, int t) {
        return wp[((size_t)row * cin + ci) * ks * ks + t];
    }));
    if (!bias.empty()) L.bias = B.upload(bias);
    if (want_wino && ks == 3 && stride == 1 && pad == 1 && cin % 8 == 0 && cout >= 16) {
        // the same conv as Winograd F(2x2,3x3) on the f32 matrix cores (run_conv takes it where the shape fits the kernel's tiles)
        L.wino = B.upload(pack_wino_A(cout, cin, [&](int row, int ci, int t) { return wp[((size_t)row * cin + ci) * 9 + t]; }));
        L.zero = B.upload(std::vector<float>(64, 0.f));
    }
    return L;
}

// stride-1 conv for the f16x3 kernels (conv_sh16.h): rows padded to a multiple of 4 with zero rows (C4 output runs)
inline ConvLayer make_conv_sh16(Builder& B, const std::vector<float>& w, const std::vector<float>& bias, int cout, int cin,
                                int ks, int pad) {
    ConvLayer L;
    L.Cout = (cout + 3) & ~3;
    L.Cin = cin;
    L.KS = ks;
    L.stride = 1;
    L.pad = pad;
    const float* wp = w.data();
    auto getw = [&](int row, int ci, int t) { return row < cout ? wp[((size_t)row * cin + ci) * ks * ks + t] : 0.f; };
    const auto kexp = sh16_row_exponents(L.Cout, cin, ks, getw);
    L.sh_wpk = B.upload(pack_A_sh16(L.Cout, cin, ks, getw, kexp));
    L.sh_wscale = B.upload(sh16_wscale(kexp));
    if (!bias.empty()) {
        std::vector<float> b(L.Cout, 0.f);
        std::copy(bias.begin(), bias.end(), b.begin());
        L.bias = B.upload(b);
    }
    return L;
}

// stride-2, pad-(ks > 1) conv in the space-to-depth form of conv_sh16_kernel<S2D> (conv_sh16.h): a 2x2-tap (ks 3 / 4) or
// 1x1 (ks 1) stride-1 conv at the output resolution over `phases` copies of the input channels.  Virtual channel
// vc = phase * cr + c; tap (dy, dx) of phase (py, px) carries the original weight at (ky, kx) = (2 dy + py, 2 dx + px)
// (zero where that index leaves the ks x ks kernel).  cr = cin rounded up to a multiple of 16 (padding channels: zeros).
// L.Cin = phases * cr, L.KS = 2 or 1, L.stride = 2 (marker), L.Cout padded to a multiple of 4.
inline ConvLayer make_conv_s2d(Builder& B, const std::vector<float>& w, const std::vector<float>& bias, int cout, int cin, int ks) {
    ConvLayer L;
    const int cr = (cin + 15) & ~15, phases = ks == 1 ? 1 : 4;
    L.Cout = (cout + 3) & ~3;
    L.Cin = phases * cr;
    L.KS = ks == 1 ? 1 : 2;
    L.stride = 2;
    L.pad = ks == 1 ? 0 : 1;
    L.s2d_cr = cr;
    L.s2d_phase0 = ks == 1 ? 3 : 0;
    const float* wp = w.data();
    auto getw = [&](int row, int vc, int t) {
        const int c = vc % cr;
        if (row >= cout || c >= cin) return 0.f;
        if (ks == 1) return wp[(size_t)row * cin + c];
        const int ph = vc / cr, ky = 2 * (t / 2) + (ph >> 1), kx = 2 * (t % 2) + (ph & 1);
        return (ky < ks && kx < ks) ? wp[(((size_t)row * cin + c) * ks + ky) * ks + kx] : 0.f;
    };
    const auto kexp = sh16_row_exponents(L.Cout, L.Cin, L.KS, getw);
    L.sh_wpk = B.upload(pack_A_sh16(L.Cout, L.Cin, L.KS, getw, kexp));
    L.sh_wscale = B.upload(sh16_wscale(kexp));
    if (!bias.empty()) {
        std::vector<float> b(L.Cout, 0.f);
        std::copy(bias.begin(), bias.end(), b.begin());
        L.bias = B.upload(b);
    }
    return L;
}

// ---- one call of a plain conv: its epilogue, its input view and the environment the routes read ---------------------------------
struct ConvOpts {
    int pad_mode = PAD_ZERO;
    int in_mode = IN_DIRECT;
    int act = ACT_NONE;
    const float* res = nullptr;
    int res_up = 0;
    int res_after_act = 0;
    float* partial = nullptr;      // split-K scratch (optional): enables split-K for few-tile / long-K layers
    long long partial_cap = 0;
    int no_wino = 0;               // 1 = keep the layer on the direct kernel (A/B tests)
    // the handle's side: options, device and shared buffers (defaults: what a net without them runs with)
    int wino = 1;                  // Winograd level: 0 = direct kernels only, 1 = F(2x2,3x3) and the 1x1 GEMM, 2 = also F(4x4,3x3)
    int wino4_force = 0;           // F(4x4,3x3) wherever the shape allows, whatever the task count
    int batch_inv = 0;             // every choice that follows the task count is made as for a large batch (no sample-pair tiles)
    int wino4_split = -1;          // Wino4Params::split
    int v_pays = -1;               // the V route of an F(4x4,3x3) call: -1 = where wino4v_pays says so, 1 = wherever V fits, 0 = never
    int pw_wide = 0;               // PwParams::wide
    int num_cus = 256;
    float* vbuf = nullptr;         // the pre-transformed input V (conv_wino4v.h) and its size; null: no V route
    size_t vbuf_bytes = 0;
    const float* zero = nullptr;   // zero page; null: the layer's own zero words
    unsigned* claim = nullptr;     // claim slot of an F(2x2,3x3) launch (dynamic task claiming), or null
};

inline int conv_out_size(const ConvLayer& L, int in, int in_mode) {
    const int l = in_mode == IN_DIRECT ? in : 2 * in;
    return (l + 2 * L.pad - L.KS) / L.stride + 1;
}

// few tiles of the direct kernels (64 rows x 512 pixels) for the device: such a layer prefers split-K and takes no fused 1x1 operand
inline bool conv_few_tiles(int Cout, long long npix) { return ((Cout + 63) / 64) * ((npix + 511) / 512) < 192; }

// The V route of one F(4x4,3x3) layer (conv_wino4v.h): taken when it `pays` and V fits the buffer; then vp is the transform pass over `in`
// (padded: hidden planes of an ACE level, conv_wino.h WINO_AXOFF; reflect: reflection padding)
inline bool wino4v_plan(bool pays, float* vbuf, size_t vbuf_bytes, const float* in, int Bn, int H, int W, int K, int nks, Wino4vPackParams& vp,
                        bool padded = false, bool reflect = false) {
    if (!(pays && vbuf && H % 32 == 0 && W % 32 == 0 && wino4v_bytes(Bn, H, W, nks) <= vbuf_bytes)) return false;
    vp = Wino4vPackParams{};
    vp.in = in;
    vp.v = vbuf;
    vp.B = Bn;
    vp.K = K;
    vp.H = H;
    vp.W = W;
    vp.nks = nks;
    vp.pitch = padded ? wino_apitch(W) : W;
    vp.xoff = padded ? WINO_AXOFF : 0;
    vp.padded = padded ? 1 : 0;
    vp.reflect = reflect ? 1 : 0;
    return true;
}

enum class ConvRoute {     // the route of one exact-f32 plain conv call (conv_route): decided once, read by the launcher and the profile figures
    F4V,         // F(4x4,3x3) over the input pre-transformed by one extra pass (conv_wino4v.h)
    F4,          // F(4x4,3x3) (conv_wino4.h; the launcher may take the split kernel, conv_wino4_split.h)
    F2,          // F(2x2,3x3) (conv_wino.h)
    Pw,          // 1x1 GEMM kernel (conv_pw.h): no bias, no residual
    Direct       // conv_mfma.h
};

// From the layer's images, the call's shape (H x W: OUTPUT size) and `o`.  Launches nothing.  A route needs its image: a layer without an
// F(4x4) image (every layer of the aux nets) never takes F(4x4), one without a direct image (the Zencoder's phase convs) must not fall to Direct.
inline ConvRoute conv_route(const ConvLayer& L, int B, int H, int W, const ConvOpts& o) {
    const bool up = o.in_mode == IN_UP2_NEAREST, refl = o.pad_mode == PAD_REFLECT;
    const bool k3 = L.KS == 3 && L.stride == 1 && L.pad == 1 && !o.res_after_act && o.wino && !o.no_wino;
    // F(2x2): tiles of 32 x 16 pixels over the direct or nearest-x2 view; 16 x 16 images as pairs of samples (direct input, zero padding, residual of
    // the same size -- so never with an up-sampled residual at 16 pixels --, and only where the batch may decide)
    const bool tiles = wino_supported(H, W, L.Cin) || (!up && !refl && !o.res_up && !o.batch_inv && !L.d2s && wino_supported_pair16(B, H, W, L.Cin));
    const bool f2 = k3 && L.wino && (o.zero || L.zero) && (o.in_mode == IN_DIRECT || up) && !(up && refl) && tiles;
    if (k3 && o.wino >= 2 && L.wino4 && o.in_mode == IN_DIRECT && !L.d2s && wino4_supported(H, W, L.Cin) &&
        (!f2 || o.wino4_force || o.batch_inv || wino4_pays((long long)B * (H / 32) * (W / 32) * ((L.Cout + 31) / 32), o.num_cus))) {
        // many GEMM rows on a small level: the input transform once, in its own pass, instead of in every row tile
        const bool pays = o.v_pays < 0 ? wino4v_pays(L.Cout, H) : o.v_pays != 0;
        Wino4vPackParams vp;
        return wino4v_plan(pays, o.vbuf, o.vbuf_bytes, nullptr, B, H, W, L.Cin, L.Cin / 4, vp) ? ConvRoute::F4V : ConvRoute::F4;
    }
    if (f2) return ConvRoute::F2;
    if (o.wino && !o.no_wino && L.pw && L.KS == 1 && L.stride == 1 && o.in_mode == IN_DIRECT && !o.res && !L.bias && o.act == ACT_NONE &&
        pw_supported(L.Cin, L.Cout, H * W))
        return ConvRoute::Pw;
    return ConvRoute::Direct;
}

// What a profile records for the call (SeanModel::prof, kind 0): FLOPs of the dense evaluation, FLOPs the matrix cores run on this route
// (< 0: the same) and algorithmic bytes.  Cin2: channels of a fused 1x1 second operand (Direct only)
struct ConvFigures { double flops, flops_exec, bytes; };
inline ConvFigures conv_figures(ConvRoute rt, const ConvLayer& w, double npix, bool res, int Cin2 = 0) {
    const double k2 = w.KS * w.KS, cin2 = Cin2;
    switch (rt) {
        case ConvRoute::F4V:
        case ConvRoute::F4:      // 36 MFMA products per 4 x 4 tile and channel instead of 144
            return {2.0 * w.Cout * w.Cin * 9.0 * npix, 2.0 * w.Cout * w.Cin * 36.0 * npix / 16.0,
                    4.0 * (npix * w.Cin + npix * w.Cout * (res ? 2.0 : 1.0) + (double)w.Cout * w.Cin * 36.0)};
        case ConvRoute::F2:      // 16 MFMA products per quad and channel instead of 36
            return {2.0 * w.Cout * w.Cin * 9.0 * npix, 2.0 * w.Cout * w.Cin * 16.0 * npix / 4.0,
                    4.0 * (npix * w.Cin + npix * w.Cout * (res ? 2.0 : 1.0) + (double)w.Cout * w.Cin * 16.0)};
        case ConvRoute::Pw:
            return {2.0 * w.Cout * w.Cin * npix, -1.0, 4.0 * (npix * w.Cin + npix * w.Cout + (double)w.Cout * w.Cin)};
        default:
            return {2.0 * w.Cout * (w.Cin * k2 + cin2) * npix, -1.0,
                    4.0 * (npix * (w.Cin + cin2) + npix * w.Cout * (res ? 2.0 : 1.0) + (double)w.Cout * (w.Cin * k2 + cin2))};
    }
}

// the direct kernel's operands (conv_mfma.h); in: [B][Cin][Hin][Win]
inline ConvParams conv_direct_params(const ConvLayer& L, const float* in, float* out, int B, int Hin, int Win, const ConvOpts& o) {
    ConvParams p{};
    p.in = in;
    p.wpk = L.wpk;
    p.out = out;
    p.B = B;
    p.Cin = L.Cin;
    p.Hin = Hin;
    p.Win = Win;
    p.H = conv_out_size(L, Hin, o.in_mode);
    p.W = conv_out_size(L, Win, o.in_mode);
    p.pad = L.pad;
    p.pad_mode = o.pad_mode;
    p.in_mode = o.in_mode;
    p.Mrows = L.Cout;
    p.bias = L.bias;
    p.res = o.res;
    p.res_up = o.res_up;
    p.res_after_act = o.res_after_act;
    p.act = o.act;
    p.partial = o.partial;
    p.partial_cap = o.partial_cap;
    return p;
}

// The launcher: in [B][Cin][Hin][Win] -> out [B][Cout][Ho][Wo] on route `rt` (= conv_route of the same call).  The three Winograd / GEMM parameter
// structs take their common operands from one list; the V route launches its transform pass first.
inline hipError_t run_conv(ConvRoute rt, const ConvLayer& L, const float* in, float* out, int B, int Hin, int Win, const ConvOpts& o, hipStream_t st) {
    const int H = conv_out_size(L, Hin, o.in_mode), W = conv_out_size(L, Win, o.in_mode);
    auto common = [&](auto& q, const float* image) {
        q.in = in;
        q.wpk = image;
        q.out = out;
        q.B = B;
        q.Cin = L.Cin;
        q.Cout = L.Cout;
    };
    auto epilogue = [&](auto& q) {
        q.H = H;
        q.W = W;
        q.bias = L.bias;
        q.res = o.res;
        q.res_up = o.res_up;
        q.act = o.act;
        q.reflect = o.pad_mode == PAD_REFLECT ? 1 : 0;
    };
    switch (rt) {
        case ConvRoute::F4V:
        case ConvRoute::F4: {
            Wino4Params q{};
            common(q, L.wino4);
            epilogue(q);
            q.wpk_split = L.wino4s;
            q.split = o.wino4_split;
            if (rt == ConvRoute::F4) return conv_wino4_plain(q, st);
            Wino4vPackParams vp;
            if (!wino4v_plan(true, o.vbuf, o.vbuf_bytes, in, B, H, W, L.Cin, L.Cin / 4, vp, false, q.reflect != 0)) return hipErrorInvalidValue;
            const hipError_t e = wino4v_pack(vp, st);
            if (e != hipSuccess) return e;
            q.v = o.vbuf;
            return conv_wino4v_plain(q, st);
        }
        case ConvRoute::F2: {
            WinoParams q{};
            common(q, L.wino);
            epilogue(q);
            q.in_up = o.in_mode == IN_UP2_NEAREST ? 1 : 0;
            q.d2s = L.d2s;
            q.zero = o.zero ? o.zero : L.zero;
            q.claim = o.claim;
            q.partial = o.partial;             // (few tasks, long k-loop: conv_wino_plain splits K)
            q.partial_cap = o.partial_cap;
            return conv_wino_plain(q, st);
        }
        case ConvRoute::Pw: {
            PwParams q{};
            common(q, L.pw);
            q.HW = H * W;
            q.wide = o.pw_wide;
            return conv_pw(q, st);
        }
        default: break;
    }
    if (!L.wpk) return hipErrorInvalidValue;
    const ConvParams p = conv_direct_params(L, in, out, B, Hin, Win, o);
    if (L.stride == 2) return conv_plain_s2(p, L.KS, st);
    if (L.KS == 3) return conv_plain3(p, st);
    if (L.KS == 1) return conv_plain1(p, st);
    return hipErrorInvalidValue;
}
inline hipError_t run_conv(const ConvLayer& L, const float* in, float* out, int B, int Hin, int Win, const ConvOpts& o, hipStream_t st) {
    return run_conv(conv_route(L, B, conv_out_size(L, Hin, o.in_mode), conv_out_size(L, Win, o.in_mode), o), L, in, out, B, Hin, Win, o, st);
}

// The f16x3 ConvParams (conv_sh16.h) of layer L: everything the layer determines, the operands and the OUTPUT size H x W; s_in = first-pass SH16
// scale of the input.  The caller adds what is its own: input mode, activation, residual, amax slots, C4 flag, split-K scratch.
inline ConvParams sh16_conv_params(const ConvLayer& L, const float* in, float* out, int B, int H, int W, float s_in) {
    ConvParams p{};
    p.in = in;
    p.wpk = L.sh_wpk;
    p.wscale = L.sh_wscale;
    p.in_scale_inv = 1.f / s_in;
    p.out = out;
    p.B = B;
    p.Cin = L.Cin;
    p.s2d_cr = L.s2d_cr;
    p.s2d_phase0 = L.s2d_phase0;
    p.H = H;
    p.W = W;
    p.Mrows = L.Cout;
    p.bias = L.bias;
    return p;
}

}  // namespace chk
