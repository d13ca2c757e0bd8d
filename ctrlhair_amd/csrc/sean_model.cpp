// sean_model.cpp -- weight folding/packing + forward schedule of the SEAN generator on MI355X.
//
// Reference behaviour restated (file:line refer to /root/reference):
//   generator.py:72-109            SPADEGenerator.forward (fc, 7 ResBlocks, nearest x2 ups, conv_img, tanh)
//   architecture.py:69-96          SPADEResnetBlock.forward / shortcut / actvn
//   normalization.py:108-189       ACE.forward (noise, eval-BN, style broadcast, style convs, SPADE, blend, modulate)
//   normalization.py:249-257       SPADE.forward
//   torch spectral_norm (eval)     W = W_orig / (u . W_mat v)
// Exact reformulations used: convs whose input is a one-hot label map or the piecewise-constant
// style map are evaluated as 9-tap label-table gathers; sigmoid(blending) is folded into weights/biases.
#include "sean_model.h"

#include <cmath>
#include <cstring>
#include <type_traits>

#include "ace_sparse.h"
#include "conv_ace_sparse.h"
#include "conv_mfma.h"
#include "conv_sh16.h"
#include "conv_pw.h"
#include "conv_wino.h"
#include "conv_wino4v.h"
#include "kernels.h"
#include "sh16.h"

namespace chk {

size_t SeanModel::noise_floats(int S) const {
    size_t n = 0;
    for (const auto& b : blocks) {
        const size_t r = (size_t)S / b.res_div;
        n += r * r * (b.learned ? 3 : 2);
    }
    return n;
}

namespace {

constexpr int LABEL_NC = 19, STYLE = 512, HID = 128;

// ---- build(): the stages, in call order ----------------------------------------------------------------------------------
// spectral norm folded at load (torch eval semantics W / (u . W_mat v)); f16x3 path: per-row power-of-two scaling
struct SN { const float* w = nullptr; double sigma = 1.0; int cout = 0, cin = 0, ks = 0; };
auto sn_get(const SN& r) {
    return [r](int row, int ci, int t) { return r.w[((size_t)row * r.cin + ci) * r.ks * r.ks + t] / (float)r.sigma; };
}

// host operands of one ACE, handed from part to part of SeanBuild::ace()
struct AceSrc {
    int C = 0;
    const float *bs = nullptr, *wgp = nullptr, *wbp = nullptr;   // mlp_shared bias, mlp_gamma / mlp_beta weights
    float ag = 0.f, ab = 0.f;                    // weight of the style branch
    float sg = 1.f, sb = 1.f;                    // ... and of the SPADE branch (1 - ag, 1 - ab)
    std::vector<float> va, vd, vn, vbg, vbb;     // eval BN + noise scaling as per-channel affine; blended biases
    std::vector<float> T;                        // mlp_shared as label table
    std::vector<double> edge_hv, edge_W6;        // straight-edge tables: host operands (contracted after the biases are final)
};

struct SeanBuild {
    SeanModel& m;
    const SeanOptions& opt;
    Builder B;
    const int mb, ms;
    int ace_index = 0;
    SeanBuild(SeanModel& mm, const TensorStore& ts, int mb_, int ms_) : m(mm), opt(mm.opt), B(ts, mm.allocs), mb(mb_), ms(ms_) {}

    std::string dims() {
        auto itfc = B.ts.find("fc.weight");
        if (itfc == B.ts.end() || itfc->second.shape.size() != 4) return "missing tensor 'fc.weight'";
        m.ngf = (int)itfc->second.shape[0] / 16;
        if (m.ngf < 4 || (m.ngf & 3)) return "unsupported ngf";
        if (ms % 32 != 0 || ms < 32 || mb < 1) return "max_size must be a multiple of 32 and max_batch >= 1";
        m.max_batch = mb;
        m.max_size = ms;
        return "";
    }

    std::string fc_and_img() {
        const int ngf = m.ngf;
        // ---- fc as label table: T[(j*9+t)*K + k] = W[k][j][t] --------------------------------------------------
        {
            const int K = 16 * ngf;
            auto w = B.get("fc.weight", (size_t)K * LABEL_NC * 9);
            auto b = B.get("fc.bias", K);
            if (!w || !b) return B.err;
            std::vector<float> T((size_t)LABEL_NC * 9 * K);
            for (int k = 0; k < K; ++k)
                for (int j = 0; j < LABEL_NC; ++j)
                    for (int t = 0; t < 9; ++t) T[((size_t)j * 9 + t) * K + k] = w->f32()[((size_t)k * LABEL_NC + j) * 9 + t];
            m.fc_table = B.upload(T);
            m.fc_bias = B.upload(std::vector<float>(b->f32(), b->f32() + K));
        }
        auto w = B.get("conv_img.weight", (size_t)3 * ngf * 9);
        auto b = B.get("conv_img.bias", 3);
        if (!w || !b) return B.err;
        m.img_w = B.upload(std::vector<float>(w->f32(), w->f32() + 3 * ngf * 9));
        std::vector<float> w4((size_t)(ngf / 4) * 27 * 4);
        for (int g = 0; g < ngf / 4; ++g)
            for (int t = 0; t < 9; ++t)
                for (int co = 0; co < 3; ++co)
                    for (int e = 0; e < 4; ++e)
                        w4[(((size_t)g * 9 + t) * 3 + co) * 4 + e] = w->f32()[((size_t)co * ngf + g * 4 + e) * 9 + t];
        m.img_w4 = B.upload(w4);
        m.img_b = B.upload(std::vector<float>(b->f32(), b->f32() + 3));
        return "";
    }

    // ---- the seven ResBlocks: convs, then the two or three ACEs ---------------------------------------------------
    std::string res_blocks() {
        struct BS { const char* name; int fin, fout, res_div; bool up, styled; };
        const BS specs[7] = {{"head_0", 16, 16, 32, false, true}, {"G_middle_0", 16, 16, 16, true, true},
                             {"G_middle_1", 16, 16, 16, false, true}, {"up_0", 16, 8, 8, true, true},
                             {"up_1", 8, 4, 4, true, true}, {"up_2", 4, 2, 2, true, true},
                             {"up_3", 2, 1, 1, true, false}};
        m.blocks.clear();
        for (const auto& s : specs) {
            BlockW bw;
            bw.name = s.name;
            bw.fin = s.fin * m.ngf;
            bw.fout = s.fout * m.ngf;
            bw.fmid = bw.fin < bw.fout ? bw.fin : bw.fout;
            bw.res_div = s.res_div;
            bw.up_before = s.up;
            bw.styled = s.styled;
            bw.learned = bw.fin != bw.fout;
            const int fuse_shift = block_convs(bw);
            if (!B.err.empty()) return B.err;
            if (bw.learned) ace(bw.name + ".ace_s", bw.fin, bw, bw.ace_s, std::ldexp(SH16_ACT_SCALE, fuse_shift));
            ace(bw.name + ".ace_0", bw.fin, bw, bw.ace_0);
            ace(bw.name + ".ace_1", bw.fmid, bw, bw.ace_1);
            if (!B.err.empty()) return B.err;
            m.blocks.push_back(bw);
        }
        m.n_aces = ace_index;
        return level_facts();
    }
    // what every ACE of a resolution level shares, read off the ACEs -- the block table cannot make them disagree, and here that is checked
    std::string level_facts() {
        for (int k = 0; k < 6; ++k) m.levels[k] = SeanModel::Level{ms >> k};
        std::string err;
        for_each_ace(m.blocks, [&](const AceW& a) {
            SeanModel::Level& L = m.levels[level_of(a.res_div)];
            const bool etab = a.edge_tab != nullptr;
            if (L.used && (L.styled != a.styled || L.edge_tab != etab)) err = "the ACEs of one resolution level disagree (styled / straight-edge table) at " + a.name;
            L.used = true;
            L.styled = a.styled;
            L.edge_tab = etab;
        });
        return err;
    }

    SN sn_read(const std::string& p, int cout, int cin, int ks) {
        SN r;
        const size_t kk = (size_t)cin * ks * ks;
        auto w = B.get(p + ".weight_orig", (size_t)cout * kk);
        auto u = B.get(p + ".weight_u", cout);
        auto v = B.get(p + ".weight_v", kk);
        if (!w || !u || !v) return r;
        double sigma = 0.0;   // u . (W_mat v)
        for (int o = 0; o < cout; ++o) {
            double acc = 0.0;
            const float* wr = w->f32() + (size_t)o * kk;
            for (size_t i = 0; i < kk; ++i) acc += (double)wr[i] * v->f32()[i];
            sigma += acc * u->f32()[o];
        }
        r.w = w->f32();
        r.sigma = sigma;
        r.cout = cout; r.cin = cin; r.ks = ks;
        return r;
    }
    void sn_pack(const SN& r, const std::string& p, bool bias, const std::vector<int>* kexp, ConvLayer& cw) {
        if (!r.w) return;
        auto getw = sn_get(r);
        if (opt.use_sh16) {
            cw.sh_wpk = B.upload(pack_A_sh16(r.cout, r.cin, r.ks, getw, *kexp, opt.terms == 2));
            cw.sh_wscale = B.upload(sh16_wscale(*kexp));
        } else {
            cw.wpk = B.upload(pack_A(r.cout, r.cin, r.ks, r.ks == 3 ? CK_KS3 : CK_KS1, getw));
            if (opt.wino && r.ks == 3 && r.cin % 8 == 0) cw.wino = B.upload(pack_wino_A(r.cout, r.cin, getw));
            if (opt.wino >= 2 && r.ks == 3 && r.cin % 8 == 0 && r.cin >= 16) {
                cw.wino4 = B.upload(pack_wino4_A(r.cout, r.cin, getw));
                if (opt.wino4_split > 0 || (opt.wino4_split < 0 && r.cout < 512)) cw.wino4s = B.upload(pack_wino4_A(r.cout, r.cin, getw, true));
            }
            if (opt.wino && r.ks == 1 && r.cin % 16 == 0) cw.pw = B.upload(pack_pw_A(r.cout, r.cin, [&](int row, int ci) { return getw(row, ci, 0); }));
        }
        cw.Cout = r.cout;
        cw.Cin = r.cin;
        cw.KS = r.ks;
        cw.pad = r.ks / 2;
        if (bias) {
            auto bb = B.get(p + ".bias", r.cout);
            if (bb) cw.bias = B.upload(std::vector<float>(bb->f32(), bb->f32() + r.cout));
        }
    }
    // conv_0 / conv_1 / conv_s of one block; returns the exponent D that aligns conv_s with conv_1 (f16x3 path, else 0). Errors: B.err
    int block_convs(BlockW& bw) {
        int fuse_shift = 0;
        const SN c0 = sn_read(bw.name + ".conv_0", bw.fmid, bw.fin, 3), c1 = sn_read(bw.name + ".conv_1", bw.fout, bw.fmid, 3);
        SN cs;
        if (bw.learned) cs = sn_read(bw.name + ".conv_s", bw.fout, bw.fin, 1);
        if (!B.err.empty()) return 0;
        std::vector<int> k0, k1, ks_;
        if (opt.use_sh16) {
            k0 = sh16_row_exponents(c0.cout, c0.cin, 3, sn_get(c0));
            k1 = sh16_row_exponents(c1.cout, c1.cin, 3, sn_get(c1));
            if (bw.learned) {
                // conv_s is folded into conv_1 as extra K chunks on the same accumulators: row by row the two operands
                // must share 2^k * s_in.  conv_1's rows keep their own exponents; conv_s's rows take k1[row] - D with
                // D = max over rows of (k1 - ks) (no row overflows, rows of similar relative size lose nothing), and the
                // 2^D is carried by the first-pass scale of the shortcut activations (ace_s writes hs * 8 * 2^D).
                ks_ = sh16_row_exponents(cs.cout, cs.cin, 1, sn_get(cs));
                int D = k1[0] - ks_[0];
                for (int r = 0; r < c1.cout; ++r) D = std::max(D, k1[r] - ks_[r]);
                D = std::max(-24, std::min(24, D));
                for (int r = 0; r < c1.cout; ++r) {       // exactly ks = k1 - D, neither above its own optimum
                    ks_[r] = std::min(ks_[r], k1[r] - D);
                    k1[r] = ks_[r] + D;
                }
                fuse_shift = D;
            }
        }
        sn_pack(c0, bw.name + ".conv_0", true, &k0, bw.conv_0);
        sn_pack(c1, bw.name + ".conv_1", true, &k1, bw.conv_1);
        if (bw.learned) sn_pack(cs, bw.name + ".conv_s", false, &ks_, bw.conv_s);
        return fuse_shift;
    }

    // ---- one ACE's weights, in four parts.  Errors: B.err ----------------------------------------------------------
    void ace(const std::string& p, int C, const BlockW& bw, AceW& a, float out_scale = SH16_ACT_SCALE) {
        a.out_scale = out_scale;
        a.name = p;
        a.C = C;
        a.res_div = bw.res_div;
        a.styled = bw.styled;
        a.index = ace_index++;
        AceSrc s;
        s.C = C;
        if (!ace_norm_and_table(p, a, s)) return;
        ace_region_tables(a, s);
        ace_spade_rows(a, s);
        if (a.styled && !ace_style(p, a, s)) return;
        if (!s.edge_hv.empty()) ace_edge_rows(p, a, s);
        // (last: the style branch adds its biases to vbg / vbb)
        a.bn_a = B.upload(s.va);
        a.bn_d = B.upload(s.vd);
        a.nv = B.upload(s.vn);
        a.bias_g = B.upload(s.vbg);
        a.bias_b = B.upload(s.vbb);
    }

    // part 1: norm / noise vectors, SPADE blend factors and weight pointers, mlp_shared as label table
    bool ace_norm_and_table(const std::string& p, AceW& a, AceSrc& s) {
        const int C = s.C;
        auto nvar = B.get(p + ".noise_var", C);
        auto rm = B.get(p + ".param_free_norm.running_mean", C);
        auto rv = B.get(p + ".param_free_norm.running_var", C);
        auto ws = B.get(p + ".Spade.mlp_shared.0.weight", (size_t)HID * LABEL_NC * 9);
        auto bs = B.get(p + ".Spade.mlp_shared.0.bias", HID);
        auto wg = B.get(p + ".Spade.mlp_gamma.weight", (size_t)C * HID * 9);
        auto bg = B.get(p + ".Spade.mlp_gamma.bias", C);
        auto wb = B.get(p + ".Spade.mlp_beta.weight", (size_t)C * HID * 9);
        auto bb = B.get(p + ".Spade.mlp_beta.bias", C);
        auto blg = B.get(p + ".blending_gamma", 1);
        auto blb = B.get(p + ".blending_beta", 1);
        if (!nvar || !rm || !rv || !ws || !bs || !wg || !bg || !wb || !bb || !blg || !blb) return false;
        if (a.styled) {
            s.ag = 1.f / (1.f + std::exp(-blg->f32()[0]));
            s.ab = 1.f / (1.f + std::exp(-blb->f32()[0]));
        }
        const float ag = s.ag, ab = s.ab;
        s.sg = 1.f - ag;
        s.sb = 1.f - ab;
        s.bs = bs->f32();
        s.wgp = wg->f32();
        s.wbp = wb->f32();
        // eval BN (eps 1e-5) + noise scaling as per-channel affine
        s.va.resize(C); s.vd.resize(C); s.vn.resize(C); s.vbg.resize(C); s.vbb.resize(C);
        for (int c = 0; c < C; ++c) {
            const float rstd = 1.f / std::sqrt(rv->f32()[c] + 1e-5f);
            s.va[c] = rstd;
            s.vd[c] = -rm->f32()[c] * rstd;
            s.vn[c] = nvar->f32()[c] * rstd;
            s.vbg[c] = (1.f - ag) * bg->f32()[c];
            s.vbb[c] = (1.f - ab) * bb->f32()[c];
        }
        // mlp_shared as label table
        std::vector<float>& T = s.T;
        T.resize((size_t)LABEL_NC * 9 * HID);
        for (int k = 0; k < HID; ++k)
            for (int j = 0; j < LABEL_NC; ++j)
                for (int t = 0; t < 9; ++t)
                    T[((size_t)j * 9 + t) * HID + k] = ws->f32()[((size_t)k * LABEL_NC + j) * 9 + t];
        a.actv_table = B.upload(T);
        a.actv_bias = B.upload(std::vector<float>(bs->f32(), bs->f32() + HID));
        // relu(bias + sum of one table entry per tap) <= bias + sum_t max(0, max_j T[j][t][k]): a bound that holds for
        // every label map, so the SH16 scale of the hidden activations can never saturate
        float bound = 0.f;
        for (int k = 0; k < HID; ++k) {
            float v = bs->f32()[k];
            for (int t = 0; t < 9; ++t) {
                float mx = 0.f;
                for (int j = 0; j < LABEL_NC; ++j) mx = std::max(mx, T[((size_t)j * 9 + t) * HID + k]);
                v += mx;
            }
            bound = std::max(bound, v);
        }
        a.actv_scale = sh16_scale_for_bound(bound);
        return true;
    }

    // part 2: per-label constants of the SPADE gamma/beta for pixels with a uniform 5x5 label neighbourhood (ace_sparse.h):
    // every tap sees a_j = relu(b_shared + sum_t' W_shared[:, j, t']), so gamma_j = (sum_t W[:, :, t]) a_j.  Double.
    // Then the host operands of the straight-edge table (contracted on the device by ace_edge_rows).
    void ace_region_tables(AceW& a, AceSrc& s) {
        const int C = s.C;
        const std::vector<float>& T = s.T;
        const float *bs = s.bs, *wgp = s.wgp, *wbp = s.wbp;
        std::vector<double> aj((size_t)LABEL_NC * HID);
        for (int j = 0; j < LABEL_NC; ++j)
            for (int k = 0; k < HID; ++k) {
                double v = bs[k];
                for (int t = 0; t < 9; ++t) v += T[((size_t)j * 9 + t) * HID + k];
                aj[(size_t)j * HID + k] = v > 0.0 ? v : 0.0;
            }
        std::vector<float> gc((size_t)LABEL_NC * 2 * C);
        std::vector<double> wsum(HID);
        for (int gb = 0; gb < 2; ++gb)
            for (int c = 0; c < C; ++c) {
                const float* w = (gb ? wbp : wgp) + (size_t)c * HID * 9;
                for (int k = 0; k < HID; ++k) {
                    double acc = 0.0;
                    for (int t = 0; t < 9; ++t) acc += w[k * 9 + t];
                    wsum[k] = acc;
                }
                for (int j = 0; j < LABEL_NC; ++j) {
                    double acc = 0.0;
                    for (int k = 0; k < HID; ++k) acc += wsum[k] * aj[(size_t)j * HID + k];
                    gc[((size_t)j * 2 + gb) * C + c] = (float)(acc * (gb ? s.sb : s.sg));
                }
            }
        a.gconst = B.upload(gc);
        // straight-edge and frame pixels (ace_sparse.h, options sean.edge / sean.frame): the per-code rows E[3040][gamma|beta][C] of the ACEs that can run at
        // 128 pixels and more (res_div <= 4), from the hidden vectors of the windows AAB / ABB (double, host) and the column / row sums
        // of the gamma / beta weights, contracted on the device in double (ace_edge_table).  vbg / vbb (blended biases) are added.
        a.edge_tab = nullptr;
        if (!m.level_marks(level_of(a.res_div), SeanModel::NOMINAL_SIZE / a.res_div, 0, false).edges) return;
        s.edge_hv.assign((size_t)2 * ACE_EDGE_HV * HID, 0.0);
        s.edge_W6.assign((size_t)2 * HID * 6 * C, 0.0);
        std::vector<double>&hv = s.edge_hv, &W6 = s.edge_W6;
        for (int o = 0; o < 2; ++o) {
            auto line = [&](int j, int u, int k) {       // shared conv's taps of label j summed across the split: column u (o = 0) / row u (o = 1)
                double v = 0.0;
                for (int w = 0; w < 3; ++w) v += T[((size_t)j * 9 + (o == 0 ? w * 3 + u : u * 3 + w)) * HID + k];
                return v;
            };
            for (int j = 0; j < LABEL_NC; ++j)
                for (int k = 0; k < HID; ++k) hv[((size_t)o * ACE_EDGE_HV + j) * HID + k] = aj[(size_t)j * HID + k];
            for (int A = 0; A < LABEL_NC; ++A)
                for (int Bl = 0; Bl < LABEL_NC; ++Bl) {
                    if (A == Bl) continue;
                    for (int k = 0; k < HID; ++k) {
                        const double aab = bs[k] + line(A, 0, k) + line(A, 1, k) + line(Bl, 2, k);
                        const double abb = bs[k] + line(A, 0, k) + line(Bl, 1, k) + line(Bl, 2, k);
                        hv[((size_t)o * ACE_EDGE_HV + 19 + (A * 19 + Bl) * 2 + 0) * HID + k] = aab > 0.0 ? aab : 0.0;
                        hv[((size_t)o * ACE_EDGE_HV + 19 + (A * 19 + Bl) * 2 + 1) * HID + k] = abb > 0.0 ? abb : 0.0;
                    }
                }
            // frame pixels (option sean.frame): the windows (outside, A, A) and (A, A, outside) -- a line outside the image adds nothing
            for (int A = 0; A < LABEL_NC; ++A)
                for (int k = 0; k < HID; ++k) {
                    const double oaa = bs[k] + line(A, 1, k) + line(A, 2, k);
                    const double aao = bs[k] + line(A, 0, k) + line(A, 1, k);
                    hv[((size_t)o * ACE_EDGE_HV + 741 + A * 2 + 0) * HID + k] = oaa > 0.0 ? oaa : 0.0;
                    hv[((size_t)o * ACE_EDGE_HV + 741 + A * 2 + 1) * HID + k] = aao > 0.0 ? aao : 0.0;
                }
        }
        for (int gb = 0; gb < 2; ++gb)
            for (int c = 0; c < C; ++c) {
                const float* w = (gb ? wbp : wgp) + (size_t)c * HID * 9;
                for (int k = 0; k < HID; ++k)
                    for (int d = 0; d < 3; ++d) {
                        double col = 0.0, row = 0.0;
                        for (int u = 0; u < 3; ++u) {
                            col += w[k * 9 + u * 3 + d];      // taps (dy = u - 1, dx = d - 1)
                            row += w[k * 9 + d * 3 + u];      // taps (dy = d - 1, dx = u - 1)
                        }
                        W6[(((size_t)gb * HID + k) * 6 + d) * C + c] = col;
                        W6[(((size_t)gb * HID + k) * 6 + 3 + d) * C + c] = row;
                    }
            }
    }
    // ... and its device contraction (after the style branch's biases went into vbg / vbb: the table rows are complete gamma / beta)
    void ace_edge_rows(const std::string& p, AceW& a, const AceSrc& s) {
        const std::vector<double>&hv = s.edge_hv, &W6 = s.edge_W6;
        double *dW = nullptr, *dH = nullptr;
        float *dbg_ = B.upload(s.vbg), *dbb_ = B.upload(s.vbb);
        a.edge_tab = B.falloc((size_t)ACE_EDGE_CODES * 2 * s.C);
        if (B.err.empty() && hipMalloc(&dW, W6.size() * 8) == hipSuccess && hipMalloc(&dH, hv.size() * 8) == hipSuccess &&
            hipMemcpy(dW, W6.data(), W6.size() * 8, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(dH, hv.data(), hv.size() * 8, hipMemcpyHostToDevice) == hipSuccess &&
            ace_edge_table(dW, dH, dbg_, dbb_, s.sg, s.sb, a.edge_tab, s.C, nullptr) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
        } else if (B.err.empty()) {
            B.err = "edge table of " + p + " failed";
        }
        if (dW) (void)hipFree(dW);
        if (dH) (void)hipFree(dH);
    }

    // part 3: SPADE gamma/beta rows: 64-row tiles = (gamma of 32 channels | beta of the same 32 channels)
    void ace_spade_rows(AceW& a, const AceSrc& s) {
        const int C = s.C, tiles = (C + 31) / 32;
        const float *wgp = s.wgp, *wbp = s.wbp;
        const float sg = s.sg, sb = s.sb;
        auto getsp = [&](int row, int ci, int t) {
            const int c = (row / 64) * 32 + (row & 31);
            if (c >= C) return 0.f;
            const bool beta = (row & 32) != 0;
            const float w = (beta ? wbp : wgp)[((size_t)c * HID + ci) * 9 + t];
            return w * (beta ? sb : sg);
        };
        if (opt.use_sh16) {
            auto kexp = sh16_row_exponents(tiles * 64, HID, 3, getsp);
            for (int t0 = 0; t0 < tiles * 64; t0 += 64) {     // one power of two per 64-row wave tile (a scalar in the ACE epilogue)
                int km = kexp[t0];
                for (int r = 0; r < 64; ++r) km = std::min(km, kexp[t0 + r]);
                for (int r = 0; r < 64; ++r) kexp[t0 + r] = km;
            }
            a.spade_wpk = B.upload(pack_A_sh16(tiles * 64, HID, 3, getsp, kexp, opt.terms == 2));
            a.spade_wscale = B.upload(sh16_wscale(kexp));
            return;
        }
        a.spade_wpk = B.upload(pack_A(tiles * 64, HID, 3, CK_KS3, getsp));
        if (!opt.wino) return;
        // Winograd path: row tiles of 16 channels, rows 0-15 = gamma, 16-31 = beta (conv_wino.h)
        auto getw = [&](int row, int ci, int t) {
            const int c = (row / 32) * 16 + (row & 15);
            if (c >= C) return 0.f;
            const bool beta = (row & 16) != 0;
            return (beta ? wbp : wgp)[((size_t)c * HID + ci) * 9 + t] * (beta ? sb : sg);
        };
        a.spade_wino = B.upload(pack_wino_A(((C + 15) / 16) * 32, HID, getw));
        if (opt.wino >= 2 && opt.wino4_ace_max_r >= 32 && C % 2 == 0) {      // (any level can fall to <= wino4_ace_max_r pixels at a smaller image size)
            // F(4x4,3x3) image for the low-resolution levels: rows interleaved so that a lane holds gamma and beta of two channels
            auto getw4 = [&](int row, int ci, int t) {
                int c, beta;
                wino4_ace_row(row, c, beta);
                if (c >= C) return 0.f;
                return (beta ? wbp : wgp)[((size_t)c * HID + ci) * 9 + t] * (beta ? sb : sg);
            };
            a.spade_wino4 = B.upload(pack_wino4_A(((C + 15) / 16) * 32, HID, getw4));
        }
    }

    // part 4: the style branch: fc_mu, the style convs as LUT rows (GEMM image / transposed / plain rows for the GEMV)
    bool ace_style(const std::string& p, AceW& a, AceSrc& s) {
        const int C = s.C;
        const float ag = s.ag, ab = s.ab;
        auto cg = B.get(p + ".conv_gamma.weight", (size_t)C * STYLE * 9);
        auto cgb = B.get(p + ".conv_gamma.bias", C);
        auto cb = B.get(p + ".conv_beta.weight", (size_t)C * STYLE * 9);
        auto cbb = B.get(p + ".conv_beta.bias", C);
        if (!cg || !cgb || !cb || !cbb) return false;
        for (int c = 0; c < C; ++c) {
            s.vbg[c] += ag * cgb->f32()[c];
            s.vbb[c] += ab * cbb->f32()[c];
        }
        std::vector<float> fw((size_t)LABEL_NC * STYLE * STYLE), fb((size_t)LABEL_NC * STYLE);
        for (int j = 0; j < LABEL_NC; ++j) {
            auto w = B.get(p + ".fc_mu" + std::to_string(j) + ".weight", (size_t)STYLE * STYLE);
            auto b = B.get(p + ".fc_mu" + std::to_string(j) + ".bias", STYLE);
            if (!w || !b) return false;
            std::memcpy(&fw[(size_t)j * STYLE * STYLE], w->f32(), sizeof(float) * STYLE * STYLE);
            std::memcpy(&fb[(size_t)j * STYLE], b->f32(), sizeof(float) * STYLE);
        }
        a.fcmu_w = B.upload(fw);
        a.fcmu_b = B.upload(fb);
        // LUT GEMM rows (t, gamma|beta, c) <- alpha * W[c][k][t]
        const float* cgp = cg->f32();
        const float* cbp = cb->f32();
        auto getl = [&](int row, int k, int) {
            const int t = row / (2 * C), gb = (row / C) & 1, c = row % C;
            return gb ? ab * cbp[((size_t)c * STYLE + k) * 9 + t] : ag * cgp[((size_t)c * STYLE + k) * 9 + t];
        };
        if (opt.use_sh16) {
            const auto kexp = sh16_row_exponents(18 * C, STYLE, 1, getl);
            a.lut_wpk = B.upload(pack_A_sh16(18 * C, STYLE, 1, getl, kexp, opt.terms == 2));
            a.lut_wscale = B.upload(sh16_wscale(kexp));
        } else {
            a.lut_wpk = B.upload(pack_A(18 * C, STYLE, 1, CK_KS1, getl));
            if (mb * LABEL_NC > 64) {      // grouped LUT build (conv_pw.h): [k][row] image
                std::vector<float> wt((size_t)STYLE * 18 * C);
                for (int row = 0; row < 18 * C; ++row)
                    for (int k = 0; k < STYLE; ++k) wt[(size_t)k * 18 * C + row] = getl(row, k, 0);
                a.lut_wt = B.upload(wt);
            }
        }
        if (mb * (LABEL_NC + 1) <= 64) {   // small batches (interactive use): the LUT build is a weight-streaming GEMV
            std::vector<float> rows((size_t)18 * C * STYLE);
            for (int row = 0; row < 18 * C; ++row) {
                const int t = row / (2 * C), gb = (row / C) & 1, cc = row % C;
                const float* src = gb ? cbp : cgp;
                const float al = gb ? ab : ag;
                // f16x3 path: the ACE epilogue expects the style LUT pre-multiplied by the output scale (conv_sh16.h)
                const float als = opt.use_sh16 ? al * a.out_scale : al;
                for (int k = 0; k < STYLE; ++k) rows[(size_t)row * STYLE + k] = als * src[((size_t)cc * STYLE + k) * 9 + t];
            }
            a.lut_rows = B.upload(rows);
        }
        return true;
    }

    // ---- Zencoder (optional: only when its tensors were loaded) ----------------------------------------------
    std::string zencoder() {
        m.has_zencoder = false;
        if (B.ts.find("Zencoder.model.1.weight") == B.ts.end()) return "";
        auto plain = [&](const std::string& p, int cout, int cin, int stride, ConvLayer& L) {
            L = make_conv(B, B.vec(p + ".weight", (size_t)cout * cin * 9), B.vec(p + ".bias", cout), cout, cin, 3, stride, 1, false);      // (z14: its own reflect-padded image)
        };
        plain("Zencoder.model.1", 32, 3, 1, m.z1);
        m.z1_w = B.upload(B.vec("Zencoder.model.1.weight", (size_t)32 * 3 * 9));      // raw [32][3][3][3] for the direct stem conv
        plain("Zencoder.model.4", 64, 32, 2, m.z4);
        plain("Zencoder.model.7", 128, 64, 2, m.z7);
        {   // ConvTranspose2d(128,256,k3,s2,p1,op1): weight [in=128][out=256][3][3] -> plain conv over the
            // zero-inserted input with flipped taps: W'[co][ci][ky][kx] = Wt[ci][co][2-ky][2-kx]
            auto wt = B.vec("Zencoder.model.10.weight", (size_t)128 * 256 * 9);
            std::vector<float> w((size_t)256 * 128 * 9);
            for (int co = 0; co < 256; ++co)
                for (int ci = 0; ci < 128; ++ci)
                    for (int t = 0; t < 9; ++t) w[((size_t)co * 128 + ci) * 9 + t] = wt[((size_t)ci * 256 + co) * 9 + (8 - t)];
            m.z10 = make_conv(B, w, B.vec("Zencoder.model.10.bias", 256), 256, 128, 3, 1, 1, false);      // (its Winograd form is the layer z10_wino: four phase convs)
        }
        plain("Zencoder.model.14", 512, 256, 1, m.z14);
        auto form = [&](int cout, int cin, int ks) {      // another conv that computes the ConvTranspose: z10's bias, its own images
            ConvLayer L;
            L.Cout = cout;
            L.Cin = cin;
            L.KS = ks;
            L.pad = ks / 2;
            L.bias = m.z10.bias;
            return L;
        };
        m.z10_wino = form(1024, 128, 3);
        m.z10_wino.d2s = 1;
        m.z10_d2s = form(1024, 128, 2);
        static const int cnt[4] = {1, 2, 2, 4};
        for (int ph = 0; ph < 4; ++ph) m.z10_pw[ph] = form(256, cnt[ph] * 128, 1);
        if (!opt.use_sh16 && opt.wino) zencoder_wino();
        if (opt.use_sh16) zencoder_sh16();
        if (!B.err.empty()) return B.err;
        m.has_zencoder = true;
        return "";
    }
    // exact-f32 path: the 256 -> 512 conv (91 % of the Zencoder FLOPs) as Winograd F(2x2,3x3), reflection-padded; the ConvTranspose
    void zencoder_wino() {
        auto w14 = B.vec("Zencoder.model.14.weight", (size_t)512 * 256 * 9);
        const float* wp = w14.data();
        auto g14 = [&](int row, int ci, int t) { return wp[((size_t)row * 256 + ci) * 9 + t]; };
        m.z14.wino = B.upload(pack_wino_A(512, 256, g14));
        // "sean.wino" = 2: the same conv as F(4x4,3x3) (conv_wino4.h, reflection instantiation) where the half-resolution grid is a multiple of 32
        if (opt.wino >= 2) m.z14.wino4 = B.upload(pack_wino4_A(512, 256, g14));
        if (opt.wino >= 2 && opt.wino4_split > 0)      // (512 GEMM rows: the V route by default; the split kernel only on request)
            m.z14.wino4s = B.upload(pack_wino4_A(512, 256, g14, true));
        // ConvTranspose2d(128, 256, k3, s2, p1, op1) (architecture.py:167-170) as four phase convs of the INPUT grid:
        //   out[2y+py][2x+px] = sum over dy, dx in {0, 1} of x[y+dy][x+dx] * Wt[ci][co][py+1-2dy][px+1-2dx]   (taps outside 0..2 absent)
        // each a 3x3 kernel with non-zero taps at offsets 0 / +1 only; as Winograd F(2x2,3x3) that is 4 products per output pixel,
        // against 9 of the plain conv over the zero-inserted view (three quarters of them on inserted zeros).  Row = 4 co + phase.
        auto wt10 = B.vec("Zencoder.model.10.weight", (size_t)128 * 256 * 9);
        const float* w10 = wt10.data();
        m.z10_wino.wino = B.upload(pack_wino_A(1024, 128, [&](int row, int ci, int t) {
            const int co = row >> 2, py = (row >> 1) & 1, px = row & 1, dy = t / 3 - 1, dx = t % 3 - 1;
            if (dy < 0 || dx < 0) return 0.f;
            const int ky = py + 1 - 2 * dy, kx = px + 1 - 2 * dx;
            return (ky >= 0 && ky < 3 && kx >= 0 && kx < 3) ? w10[((size_t)ci * 256 + co) * 9 + ky * 3 + kx] : 0.f;
        }));
        // The same four phases as plain GEMMs (conv_pw.h) over shifted views of the input (misc_kernels.hip convt_shift4: planes
        // (0,1) | (0,0) | (1,0) | (1,1)): phase (py, px) contracts only its OWN taps -- 1 + 2 + 2 + 4 = 9 products per 2 x 2 outputs and
        // channel pair, against 16 of the Winograd phase convs above (whose 3x3 kernels are mostly zeros).  Option "sean.convt_gemm".
        if (!opt.convt_gemm) return;
        static const int first[4] = {1, 0, 1, 0}, cnt[4] = {1, 2, 2, 4}, sdy[4] = {0, 0, 1, 1}, sdx[4] = {1, 0, 0, 1};
        for (int ph = 0; ph < 4; ++ph) {
            const int py = ph >> 1, px = ph & 1;
            m.z10_pw[ph].pw = B.upload(pack_pw_A(256, cnt[ph] * 128, [&](int co, int ci) {
                const int sh = first[ph] + ci / 128, c = ci % 128;
                const int ky = py + 1 - 2 * sdy[sh], kx = px + 1 - 2 * sdx[sh];
                return (ky >= 0 && ky < 3 && kx >= 0 && kx < 3) ? w10[((size_t)c * 256 + co) * 9 + ky * 3 + kx] : 0.f;
            }));
        }
    }
    // the 256->512 conv is 91 % of the Zencoder FLOPs: run it on the f16x3 path too
    void zencoder_sh16() {
        auto w14 = B.vec("Zencoder.model.14.weight", (size_t)512 * 256 * 9);
        const float* wp = w14.data();
        auto g14 = [&](int row, int ci, int t) { return wp[((size_t)row * 256 + ci) * 9 + t]; };
        const auto k14 = sh16_row_exponents(512, 256, 3, g14);
        m.z14.sh_wpk = B.upload(pack_A_sh16(512, 256, 3, g14, k14));
        m.z14.sh_wscale = B.upload(sh16_wscale(k14));
        // the ConvTranspose too (a 3x3 conv over the zero-inserted view, flipped taps as above)
        auto wt10 = B.vec("Zencoder.model.10.weight", (size_t)128 * 256 * 9);
        const float* w10 = wt10.data();
        auto g10 = [&](int row, int ci, int t) { return w10[((size_t)ci * 256 + row) * 9 + (8 - t)]; };
        const auto k10 = sh16_row_exponents(256, 128, 3, g10);
        m.z10.sh_wpk = B.upload(pack_A_sh16(256, 128, 3, g10, k10));
        m.z10.sh_wscale = B.upload(sh16_wscale(k10));
        {   // depth-to-space form of the same ConvTranspose: out[2y+py][2x+px] += x[y+dy][x+dx] * Wt[ci][co][py+1-2dy][px+1-2dx]
            auto gd = [&](int row, int ci, int t) {
                const int ph = row / 256, co = row % 256;
                const int ky = (ph >> 1) + 1 - 2 * (t / 2), kx = (ph & 1) + 1 - 2 * (t % 2);
                return (ky >= 0 && ky < 3 && kx >= 0 && kx < 3) ? w10[((size_t)ci * 256 + co) * 9 + ky * 3 + kx] : 0.f;
            };
            const auto kd = sh16_row_exponents(1024, 128, 2, gd);
            m.z10_d2s.sh_wpk = B.upload(pack_A_sh16(1024, 128, 2, gd, kd));
            m.z10_d2s.sh_wscale = B.upload(sh16_wscale(kd));
        }
        // and the two stride-2 convs (space-to-depth form)
        m.z4_s2d = make_conv_s2d(B, B.vec("Zencoder.model.4.weight", (size_t)64 * 32 * 9), B.vec("Zencoder.model.4.bias", 64), 64, 32, 3);
        m.z7_s2d = make_conv_s2d(B, B.vec("Zencoder.model.7.weight", (size_t)128 * 64 * 9), B.vec("Zencoder.model.7.bias", 128), 128, 64, 3);
    }

    // ---- run-ahead and overlap resources (after the scratch buffers every handle has) ------------------------------
    std::string run_ahead() {
        m.amax_slots = static_cast<unsigned*>(B.dalloc(64 * sizeof(unsigned)));   // 2 per ACE: [output, style projections]
        m.zero_page = static_cast<float*>(B.dalloc(256));
        if (m.zero_page) (void)hipMemset(m.zero_page, 0, 256);
        m.splitk_cap = (long long)16 << 20;     // 64 MiB of split-K slabs (low-resolution layers only)
        m.splitk_ws = B.falloc((size_t)m.splitk_cap);
        m.gb_small = nullptr;
        m.gb_small_cap = 0;
        if (!opt.use_sh16) {
            m.gb_small_cap = (long long)4 << 20;      // 16 MiB: rows x pixels of the tiny ACE launches that take the plain split-K route
            m.gb_small = B.falloc((size_t)m.gb_small_cap);
        }
        const int n_aces = m.n_aces;
        // Run-ahead mode of small jobs (Runner::prepare_all_ahead): a side stream, one join event and one set of buffers per ACE.
        // Only when the handle is sized for interactive work -- for large batches the convs own every CU and nothing co-schedules.
        // Default: interactive sizes only (up to 2 x 512^2 per chunk, where the win was measured: 3.3 -> 2.65 ms per render at
        // 256^2).  The per-ACE buffers of the full mode cost mb * r^2 * 128 * 4 bytes each -- 4.3 GB for an 8 x 512^2 handle, for
        // 1.6 % at that size -- so larger handles opt in explicitly: option "sean.ahead" = images of 512^2 per chunk (0 = never).
        long long limit = opt.ahead_pixels < 0 ? (long long)2 * 512 * 512 : opt.ahead_pixels;
        // Larger jobs keep the (HBM-write-bound) label-table kernels inline and run only the style LUT builds -- small,
        // latency-bound GEMMs -- ahead (ahead_full = false) -- unless the overlap mode serves them (sean_model.h): then the label
        // tables of every ACE run ahead too, on a side stream confined to a few CUs.
        int ncu = 0, dev = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) ncu = 0;
        if (ncu > 0) m.num_cus = ncu;
        m.overlap_on = false;
        if (opt.overlap > 0 && !opt.use_sh16 && opt.wino && (long long)mb * ms * ms > limit && ms >= 128) {
            const int want = std::min(opt.overlap, ncu / 2) & ~7;
            if (want >= 8) {
                uint32_t mask[16] = {};
                for (int i = 0; i < want; ++i) mask[i >> 5] |= 1u << (i & 31);      // (CU i of the mask sits on XCD i % 8)
                const uint32_t words = (uint32_t)((ncu + 31) / 32);
                if (hipExtStreamCreateWithCUMask(&m.side, words, mask) == hipSuccess && hipExtStreamCreateWithCUMask(&m.side_int, words, mask) == hipSuccess &&
                    hipStreamCreateWithFlags(&m.main_i, hipStreamNonBlocking) == hipSuccess &&
                    hipEventCreateWithFlags(&m.ev_in, hipEventDisableTiming) == hipSuccess && hipEventCreateWithFlags(&m.ev_out, hipEventDisableTiming) == hipSuccess &&
                    hipEventCreateWithFlags(&m.ev_fork, hipEventDisableTiming) == hipSuccess) {
                    m.overlap_on = true;
                } else {
                    return "overlap mode: stream creation failed (hipExtStreamCreateWithCUMask)";
                }
            }
        }
        if (m.overlap_on) {
            if (limit <= 0) limit = 1;      // (the per-ACE buffers below)
            m.ev_x.assign(n_aces, nullptr);
            m.ev_int.assign(n_aces, nullptr);
            for (auto& e : m.ev_x)
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return "event creation failed";
            for (auto& e : m.ev_int)
                if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return "event creation failed";
            m.claim_pool = static_cast<unsigned*>(B.dalloc((size_t)SeanModel::CLAIM_SLOTS * SeanModel::CLAIM_WORDS * sizeof(unsigned)));
        }
        m.ahead_limit = limit;
        if (limit <= 0) return "";
        m.ahead_full = m.overlap_on || (long long)mb * ms * ms <= limit;
        if (!m.overlap_on && (hipStreamCreateWithFlags(&m.side, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&m.ev_fork, hipEventDisableTiming) != hipSuccess))
            return "side stream creation failed";
        m.ev_join.assign(n_aces, nullptr);
        m.actv_ahead.assign(n_aces, nullptr);
        m.lut_ahead.assign(n_aces, nullptr);
        for (auto& e : m.ev_join)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return "event creation failed";
        for_each_ace(m.blocks, [&](const AceW& a) {
            const size_t r = (size_t)ms / a.res_div;
            if (m.ahead_full) m.actv_ahead[a.index] = B.falloc((size_t)mb * r * (r + 64) * (HID + 20));
            if (a.styled) m.lut_ahead[a.index] = B.falloc(npad() * 18 * a.C);
        });
        m.splitk_side = B.falloc((size_t)m.splitk_cap);
        return "";
    }

    // ---- workspace arena --------------------------------------------------------------------------------
    size_t npad() const { return (((size_t)mb * (LABEL_NC + 1) + 31) / 32) * 32; }     // f16x3 path: 20 columns per sample (19 = zero column)
    std::string arena() {
        const size_t MB = mb, S = ms;
        for (int k = 1; k <= 5; ++k)     // res_div 2^k
            m.levels[k].lab = static_cast<uint8_t*>(B.dalloc(MB * m.levels[k].r * m.levels[k].r));
        size_t nf = m.noise_floats(ms);
        m.noise_ws = static_cast<float*>(B.dalloc(MB * nf * 4));
        m.mu_img = static_cast<float*>(B.dalloc((size_t)STYLE * npad() * 4));
        if (m.mu_img) (void)hipMemset(m.mu_img, 0, (size_t)STYLE * npad() * 4);      // pad columns stay zero
        style_projections();
        style_lut_groups();
        size_t lutmax = 0, h0max = 0, midmax = 0, outmax = 0;
        for (const auto& b : m.blocks) {
            const size_t r = S / b.res_div, px = MB * r * r;
            if (b.styled) lutmax = std::max(lutmax, npad() * 18 * b.fin);      // npad columns: the f16x3 LUT GEMM writes the pad too
            h0max = std::max(h0max, px * b.fin);
            midmax = std::max(midmax, px * b.fmid);
            outmax = std::max(outmax, px * b.fout);
        }
        outmax = std::max(outmax, (size_t)MB * 16 * m.ngf * (S / 32) * (S / 32));
        if (m.has_zencoder) {   // Zencoder activations live in h0/hs (<= 512 ch at S/2) and dx/h1 (<= 64 ch at S/2)
            h0max = std::max(h0max, MB * S * S * 128);
            midmax = std::max(midmax, MB * S * S * (opt.use_sh16 ? 64 : 16));
        }
        m.lut = static_cast<float*>(B.dalloc(lutmax * 4));
        m.actv = static_cast<float*>(B.dalloc(MB * S * S * HID * 4));      // (direct kernels; the Winograd ACE levels own padded buffers, Level::actv)
        m.h0 = static_cast<float*>(B.dalloc(h0max * 4));
        m.hs = static_cast<float*>(B.dalloc(h0max * 4));
        m.dx = static_cast<float*>(B.dalloc(midmax * 4));
        m.h1 = static_cast<float*>(B.dalloc(midmax * 4));
        m.xs = static_cast<float*>(B.dalloc(outmax * 4));
        m.xa = static_cast<float*>(B.dalloc(outmax * 4));
        m.xb = static_cast<float*>(B.dalloc(outmax * 4));
        return "";
    }
    // one fc_mu launch per chunk for all styled ACEs (f16x3: SH16 images; exact f32: f32 images, batches of more than 64 (sample, label) columns)
    void style_projections() {
        const int n_aces = m.n_aces;
        m.fcmu_batched = opt.use_sh16 ? mb * (LABEL_NC + 1) > 64 : mb * LABEL_NC > 64;
        if (!m.fcmu_batched) return;
        m.mu_stride = (long long)STYLE * npad();
        m.mu_all = static_cast<float*>(B.dalloc((size_t)n_aces * m.mu_stride * 4));
        if (m.mu_all) (void)hipMemset(m.mu_all, 0, (size_t)n_aces * m.mu_stride * 4);
        std::vector<const float*> wp(n_aces, nullptr), bp(n_aces, nullptr);
        for_each_ace(m.blocks, [&](const AceW& a) {
            if (a.styled) { wp[a.index] = a.fcmu_w; bp[a.index] = a.fcmu_b; }
        });
        m.fcmu_w_ptrs = static_cast<const float**>(B.dalloc(n_aces * sizeof(float*)));
        m.fcmu_b_ptrs = static_cast<const float**>(B.dalloc(n_aces * sizeof(float*)));
        if (m.fcmu_w_ptrs && m.fcmu_b_ptrs) {
            (void)hipMemcpy(m.fcmu_w_ptrs, wp.data(), n_aces * sizeof(float*), hipMemcpyHostToDevice);
            (void)hipMemcpy(m.fcmu_b_ptrs, bp.data(), n_aces * sizeof(float*), hipMemcpyHostToDevice);
        }
    }
    // exact-f32 path: the group table of the one grouped GEMM launch that builds every style LUT of a chunk (Runner::luts_grouped)
    void style_lut_groups() {
        m.lut_groups = nullptr;
        m.lut_groups_wide = false;
        m.lut_ngroups = m.lut_group_tiles = 0;
        m.lut_group_rows = 0.0;
        m.code_copy = nullptr;
        m.code_state = nullptr;
        m.code_bytes = 0;
        m.code_dirty = false;
        if (!(m.fcmu_batched && !opt.use_sh16 && opt.lut_grouped)) return;
        if (m.lut_ahead.empty()) m.lut_ahead.assign(m.n_aces, nullptr);
        std::vector<PwGroup> g;
        bool ok = true;                           // all styled ACEs or none: the consumers take every LUT from the same place
        for_each_ace(m.blocks, [&](const AceW& a) {
            if (a.styled && (!a.lut_wt || (18 * a.C) % 128)) ok = false;
        });
        for_each_ace(m.blocks, [&](const AceW& a) {
            if (!ok || !a.styled) return;
            if (!m.lut_ahead[a.index]) m.lut_ahead[a.index] = B.falloc(npad() * 18 * a.C);
            PwGroup e{};
            e.in = a.lut_wt;
            e.wpk = m.mu_all + (size_t)a.index * m.mu_stride;
            e.out = m.lut_ahead[a.index];
            e.HW = 18 * a.C;                 // (C % 64 == 0: 18 C % 128 == 0)
            e.start = m.lut_group_tiles;     // in pixel tiles; the kernel multiplies by the call's row groups
            if (!e.out) { ok = false; return; }
            m.lut_group_tiles += e.HW / 128;
            m.lut_group_rows += e.HW;
            g.push_back(e);
        });
        if (ok && !g.empty()) {
            m.lut_groups = B.dalloc(g.size() * sizeof(PwGroup));
            if (m.lut_groups) (void)hipMemcpy(m.lut_groups, g.data(), g.size() * sizeof(PwGroup), hipMemcpyHostToDevice);
            m.lut_ngroups = (int)g.size();
            m.lut_groups_wide = true;
            for (const PwGroup& e : g) m.lut_groups_wide = m.lut_groups_wide && e.HW % 256 == 0;
        }
        // Code memo (sean_model.h): the copy of the codes and the state words, on handles with the grouped launch only
        if (!(opt.code_memo && m.lut_groups)) return;
        m.code_bytes = (size_t)mb * LABEL_NC * STYLE * 4 + CODE_WORDS * sizeof(int);
        m.code_copy = static_cast<float*>(B.dalloc((size_t)mb * LABEL_NC * STYLE * 4));
        m.code_state = static_cast<int*>(B.dalloc(CODE_WORDS * sizeof(int)));
        if (m.code_state && hipMemset(m.code_state, 0, CODE_WORDS * sizeof(int)) != hipSuccess) m.code_state = nullptr;      // (no memo)
        if (!m.code_copy) m.code_state = nullptr;
    }

    // ---- Winograd ACE path: boundary-quad lists per level, task lists per (level, row tiles), per-sample style images ------
    std::string wino_levels() {
        m.pad_state.clear();
        m.wsty = m.wsty4 = nullptr;
        if (!(opt.wino && !opt.use_sh16)) return "";
        size_t wsty_max = 0, wsty4_max = 0;
        for_each_ace(m.blocks, [&](const AceW& a) {
            if (!a.spade_wino) return;
            const int r = m.levels[level_of(a.res_div)].r;
            if (r < 32 || r % 32) return;
            SeanModel::WinoLevel& L = m.levels[level_of(a.res_div)].wq;
            if (!L.qlist) wino_level_lists(L, r);
            const int nrt = (a.C + 15) / 16;
            bool have = false;
            for (const auto& w : L.works) have = have || w.nrt == nrt;
            if (!have) {
                SeanModel::WinoWork w;
                w.nrt = nrt;
                w.work = static_cast<unsigned*>(B.dalloc(((size_t)L.cap_tiles * 4 + mb) * ((nrt + 1) / 2) * sizeof(unsigned)));
                w.total = static_cast<int*>(B.dalloc(8 * sizeof(int)));
                L.works.push_back(w);
            }
            if (a.styled) wsty_max = std::max(wsty_max, (size_t)mb * nrt * 5 * 2048);
            if (a.styled && a.spade_wino4) wsty4_max = std::max(wsty4_max, (size_t)mb * nrt * 6 * wino4::ADW);
        });
        if (wsty_max) m.wsty = B.falloc(wsty_max);
        // patch source of the gather kernel (conv_wino.h): up to 32 chunks of 64 boundary quads per sample (3 % of the quads of a 512^2
        // level) x 148 channels x 4 KB -- what the straight-edge reduction leaves on label maps with straight region borders
        m.patchbuf = nullptr;
        m.patch_cap_chunks = 0;
        if (opt.patch && opt.wino_gather && mb <= 32) {
            m.patch_cap_chunks = 32 * mb;
            m.patchbuf = B.falloc((size_t)m.patch_cap_chunks * (HID + 20) * 1024);
        }
        if (wsty4_max) m.wsty4 = B.falloc(wsty4_max);
        m.wsty4_floats = m.wsty4 ? wsty4_max : 0;
        wino4v_buffer();
        for (SeanModel::Level& V : m.levels)      // the planes its ACEs write (AcePlan::kout; up_3 is unstyled: 128 planes, no one-hot planes)
            if (V.wq.qlist) V.actv = B.falloc((size_t)mb * V.r * wino_apitch(V.r) * (V.styled ? HID + 20 : HID));
        return "";
    }
    void wino_level_lists(SeanModel::WinoLevel& L, int r) {
        const bool gather = opt.wino_gather && mb <= 32 && (r / 2) * (r / 2) <= 2048 * 64;
        L.TH = gather ? 16 : opt.wino_tile_h(r);
        L.cap_tiles = mb * (r / 32) * (r / L.TH);
        L.qlist = static_cast<uint8_t*>(B.dalloc((size_t)L.cap_tiles * 8 * L.TH));
        L.qcnt = static_cast<int*>(B.dalloc((size_t)L.cap_tiles * sizeof(int)));
        L.pcnt = static_cast<int*>(B.dalloc((size_t)L.cap_tiles * sizeof(int)));
        if (gather) {
            L.gq_cap = (r / 2) * (r / 2);
            L.gq = static_cast<unsigned*>(B.dalloc((size_t)mb * L.gq_cap * sizeof(unsigned)));
            L.gq_n = static_cast<int*>(B.dalloc(32 * sizeof(int)));
            L.qoff = static_cast<int*>(B.dalloc((size_t)L.cap_tiles * sizeof(int)));
            L.chunk_base = static_cast<int*>(B.dalloc(34 * sizeof(int)));
            L.patch_mode = static_cast<int*>(B.dalloc(sizeof(int)));
        }
    }
    // pre-transformed-input route (conv_wino4v.h): one V image, sized for the largest layer that takes it at (mb, ms)
    void wino4v_buffer() {
        m.vbuf = nullptr;
        m.vbuf_bytes = 0;
        if (!(opt.wino >= 2 && opt.wino4v)) return;
        size_t need = 0;
        auto level_r = [&](int res_div) {       // the level's size when it can take the route at max_size, else 0
            const int r = m.levels[level_of(res_div)].r;
            return (r < 32 || r % 32 || r > 64) ? 0 : r;
        };
        for (const auto& b : m.blocks)
            for (const ConvLayer* c : {&b.conv_0, &b.conv_1})
                if (const int r = level_r(b.res_div))
                    if (c->wino4 && wino4v_pays(c->Cout, r)) need = std::max(need, wino4v_bytes(mb, r, r, c->Cin / 4));
        for_each_ace(m.blocks, [&](const AceW& a) {
            if (const int r = level_r(a.res_div))
                if (m.ace_route_shape(a, r) == AceRoute::F4 && wino4v_pays(2 * a.C, r)) need = std::max(need, wino4v_bytes(mb, r, r, 38));
        });
        // the Zencoder's 256 -> 512 conv on the half-resolution grid: 9 bytes x 256 channels x (ms / 2)^2 per sample -- up to 2.5 GB only
        if (m.z14.wino4 && (ms / 2) % 32 == 0 && wino4v_bytes(mb, ms / 2, ms / 2, 64) <= ((size_t)5 << 29)) need = std::max(need, wino4v_bytes(mb, ms / 2, ms / 2, 64));
        if (need) {
            m.vbuf = static_cast<float*>(B.dalloc(need));
            m.vbuf_bytes = need;
        }
    }

    // ---- exact SPADE-interior reduction: classification buffers per level, work lists per (level, row tiles) ------------
    std::string sparse_levels() {
        m.prof_stats_cap = 16384;
        m.prof_stats_used = 0;
        m.prof_stats = static_cast<int*>(B.dalloc((size_t)m.prof_stats_cap * 4 * sizeof(int)));
        m.gtab = m.gtab_side = nullptr;
        if (!opt.sparse) return "";
        int cmax = 0;
        for_each_ace(m.blocks, [&](const AceW& a) {
            const int k = level_of(a.res_div), r = m.levels[k].r;
            if (r < opt.sparse_min_r || r < 32) return;
            const int mt = (a.C + 31) / 32;
            // f16x3 path: tile-skip mode of the wave-specialised kernel, whose tiles are 32 x 16
            const int th = opt.use_sh16 ? 16 : opt.sparse_tile_h(mt, r);
            const int ti = th == 16 ? 1 : 0;
            SparseLevel& L = m.levels[k].sp[ti];
            if (!L.u5) {
                L.TH = th;
                L.cap_tiles = mb * ((r + 31) / 32) * ((r + L.TH - 1) / L.TH);
                L.u5 = static_cast<uint8_t*>(B.dalloc((size_t)mb * r * r));
                L.e16 = m.level_marks(k, r, ti, false).edges ? static_cast<uint16_t*>(B.dalloc((size_t)mb * r * r * sizeof(uint16_t))) : nullptr;
                L.need = static_cast<uint8_t*>(B.dalloc((size_t)mb * r * r));
                L.list = static_cast<uint16_t*>(B.dalloc((size_t)L.cap_tiles * 32 * L.TH * sizeof(uint16_t)));
                L.cnt = static_cast<int*>(B.dalloc((size_t)L.cap_tiles * sizeof(int)));
            }
            bool have = false;
            for (const auto& w : m.levels[k].sp_work) have = have || w.mtiles == mt;
            if (!have) {
                SparseWork w;
                w.mtiles = mt;
                w.TH = L.TH;
                w.mode = opt.use_sh16 ? (opt.sh16_compact ? (opt.sh16_compact >= 2 ? 2 : 3) : 1) : 0;   // 3: with pair entries
                w.cap = (long long)L.cap_tiles * (opt.use_sh16 ? mt : sparse_max_tasks(L.TH, mt));
                w.work = static_cast<unsigned*>(B.dalloc((size_t)w.cap * sizeof(unsigned)));
                w.total = static_cast<int*>(B.dalloc(4 * sizeof(int)));
                if (w.mode == 3) {
                    w.work2 = static_cast<unsigned*>(B.dalloc((size_t)L.cap_tiles * ((mt + 1) / 2) * sizeof(unsigned)));
                    w.total2 = static_cast<int*>(B.dalloc(4 * sizeof(int)));
                    if (mt >= 4 && !(opt.dbg & DBG_NO_WORK_QUADS))
                        w.work3 = static_cast<unsigned*>(B.dalloc((size_t)L.cap_tiles * ((mt + 3) / 4) * sizeof(unsigned)));
                }
                m.levels[k].sp_work.push_back(w);
            }
            cmax = std::max(cmax, a.C);
        });
        if (cmax) m.gtab = B.falloc((size_t)mb * LABEL_NC * 2 * cmax);
        if (cmax && m.overlap_on) m.gtab_side = B.falloc((size_t)mb * LABEL_NC * 2 * cmax);
        m.p6 = (cmax && m.level_marks(0, SeanModel::NOMINAL_SIZE, 0, false).edges) ? B.falloc((size_t)mb * LABEL_NC * 6 * 2 * cmax) : nullptr;      // (straight-edge pixels: ace_sparse.h)
        return "";
    }

    // ---- ACE prologue (Runner::prologue): per-ACE destinations, sized by the route the ACE takes at (mb, ms) -----------------------
    // Handles beyond the run-ahead sizes only (interactive handles run everything ahead on the side stream); not in overlap mode, whose side
    // streams own the same work.  A call at a smaller S moves every ACE down a level: an ACE whose buffer exists and still fits its route uses
    // it, any other takes its inline launches -- Runner::prologue decides per call, from the chunk's plan (the same SeanModel::ace_route).
    std::string prologue_buffers() {
        const int n_aces = m.n_aces;
        m.pro_actv.assign(n_aces, nullptr);
        m.pro_gtab.assign(n_aces, nullptr);
        m.pro_p6.assign(n_aces, nullptr);
        m.pro_wsty.assign(n_aces, nullptr);
        m.memo_acc.assign(n_aces, nullptr);
        m.memo_acc_tasks.assign(n_aces, 0);
        m.memo_v1h[0] = m.memo_v1h[1] = nullptr;
        m.spade_memo_on = false;
        m.pro_bytes = 0;
        m.pro_on = opt.prologue && opt.wino && !opt.use_sh16 && !m.overlap_on && (long long)mb * ms * ms > m.ahead_limit;
        if (!m.pro_on) return "";
        auto alloc = [&](size_t floats) {
            m.pro_bytes += floats * 4;
            return B.falloc(floats);
        };
        for_each_ace(m.blocks, [&](const AceW& a) {
            const int r = m.levels[level_of(a.res_div)].r;
            if (!m.wino_work(a, r)) return;
            if (m.ace_route_shape(a, r) == AceRoute::F4) {
                m.pro_actv[a.index] = alloc((size_t)mb * r * wino_apitch(r) * (a.styled ? HID + 20 : HID));
                return;
            }
            if (opt.sparse && r >= opt.sparse_min_r && m.gtab) {
                m.pro_gtab[a.index] = alloc((size_t)mb * LABEL_NC * 2 * a.C);
                if (a.styled && m.p6) m.pro_p6[a.index] = alloc((size_t)mb * LABEL_NC * 6 * 2 * a.C);
            }
            if (a.styled && m.wsty) m.pro_wsty[a.index] = alloc((size_t)mb * ((a.C + 15) / 16) * 5 * 2048);
        });
        return label_memo_buffers();
    }
    // Label memo (sean_model.h): the copy of the labels, the state words, per gather-route ACE a patch buffer (styled: the size of the shared
    // patchbuf at the ACE's plane count) or the gamma / beta of its boundary quads (unstyled: 64 KB per task, as many tasks as a level in patch
    // mode can have -- patch_cap_chunks chunks x the ACE's row pairs)
    std::string label_memo_buffers() {
        m.memo_patch.assign(m.n_aces, nullptr);
        m.memo_gb.assign(m.n_aces, nullptr);
        m.memo_gb_cap.assign(m.n_aces, 0);
        m.memo_bytes = 0;
        m.memo_lab = nullptr;
        m.memo_state = nullptr;
        if (!opt.label_memo) return "";
        m.memo_bytes = (size_t)mb * ms * ms + MEMO_WORDS * sizeof(int);
        m.memo_lab = static_cast<uint8_t*>(B.dalloc((size_t)mb * ms * ms));
        m.memo_state = static_cast<int*>(B.dalloc(MEMO_WORDS * sizeof(int)));
        if (!m.memo_lab || !m.memo_state) return "";      // (B.err names the failure)
        if (hipMemset(m.memo_state, 0, MEMO_WORDS * sizeof(int)) != hipSuccess) return "hipMemset failed (label memo state)";
        for_each_ace(m.blocks, [&](const AceW& a) {
            const int r = m.levels[level_of(a.res_div)].r;
            if (!m.patchbuf || !m.wino_work(a, r) || m.ace_route_shape(a, r) != AceRoute::WinoQuads || !m.levels[level_of(a.res_div)].wq.gq) return;
            size_t floats = (size_t)m.patch_cap_chunks * (HID + 20) * 1024;
            if (a.styled) m.memo_patch[a.index] = B.falloc(floats);
            else {
                m.memo_gb_cap[a.index] = m.patch_cap_chunks * (((a.C + 15) / 16 + 1) / 2);
                floats = (size_t)m.memo_gb_cap[a.index] * 8 * 512 * 4;
                m.memo_gb[a.index] = B.falloc(floats);
            }
            m.memo_bytes += floats * 4;
        });
        // SPADE memo (sean_model.h): the accumulator cache of every styled ACE that takes the F(4x4) V route at (mb, ms), and the two
        // one-hot V images
        if (!(opt.spade_memo && opt.wino >= 2 && opt.wino4v && m.vbuf && m.wsty4)) return "";
        for_each_ace(m.blocks, [&](const AceW& a) {
            const int r = m.levels[level_of(a.res_div)].r;
            if (r < 32 || r % 32 || r > 64 || !a.styled || !m.pro_actv[a.index]) return;
            if (m.ace_route_shape(a, r) != AceRoute::F4 || !wino4v_pays(2 * a.C, r) || wino4v_bytes(mb, r, r, 38) > m.vbuf_bytes) return;
            const size_t bytes = wino4v_acc_bytes(mb, r, r, a.C);
            m.memo_acc[a.index] = static_cast<float*>(B.dalloc(bytes));
            m.memo_acc_tasks[a.index] = (long long)(bytes / (36 * 8192));
            m.memo_bytes += bytes;
            m.spade_memo_on = true;
        });
        if (m.spade_memo_on)
            for (int i = 0; i < 2; ++i) {
                const int r = 32 << i;
                m.memo_v1h[i] = static_cast<float*>(B.dalloc(wino4v_bytes(mb, r, r, 6)));
                m.memo_bytes += wino4v_bytes(mb, r, r, 6);
            }
        return "";
    }
};

}  // namespace

std::string SeanModel::build(const TensorStore& ts, int mb, int ms) {
    SeanBuild s(*this, ts, mb, ms);
    typedef std::string (SeanBuild::*Stage)();
    static const Stage stages[] = {&SeanBuild::dims,      &SeanBuild::fc_and_img, &SeanBuild::res_blocks,  &SeanBuild::zencoder,
                                   &SeanBuild::run_ahead, &SeanBuild::arena,      &SeanBuild::wino_levels, &SeanBuild::sparse_levels,
                                   &SeanBuild::prologue_buffers};
    for (Stage stage : stages) {
        const std::string e = (s.*stage)();
        if (!e.empty()) return e;
    }
    if (!s.B.err.empty()) return s.B.err;
    if (hipDeviceSynchronize() != hipSuccess) return "hipDeviceSynchronize failed after weight upload";
    return "";
}


void SeanModel::destroy() {
    for (void* p : allocs) (void)hipFree(p);
    allocs.clear();
    for (auto e : ev_join)
        if (e) (void)hipEventDestroy(e);
    ev_join.clear();
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    ev_fork = nullptr;
    if (side) (void)hipStreamDestroy(side);
    side = nullptr;
    if (side_int) (void)hipStreamDestroy(side_int);
    if (main_i) (void)hipStreamDestroy(main_i);
    side_int = main_i = nullptr;
    for (auto e : ev_x)
        if (e) (void)hipEventDestroy(e);
    for (auto e : ev_int)
        if (e) (void)hipEventDestroy(e);
    ev_x.clear();
    ev_int.clear();
    if (ev_in) (void)hipEventDestroy(ev_in);
    if (ev_out) (void)hipEventDestroy(ev_out);
    ev_in = ev_out = nullptr;
    overlap_on = false;
    claim_pool = nullptr;
    actv_ahead.clear();
    lut_ahead.clear();
    pro_actv.clear();
    pro_gtab.clear();
    pro_p6.clear();
    pro_wsty.clear();
    pro_on = false;
    memo_patch.clear();
    memo_gb.clear();
    memo_gb_cap.clear();
    memo_acc.clear();
    memo_acc_tasks.clear();
    memo_v1h[0] = memo_v1h[1] = nullptr;
    spade_memo_on = false;
    memo_lab = nullptr;
    memo_state = nullptr;
    memo_dirty = false;
    code_copy = nullptr;
    code_state = nullptr;
    code_dirty = false;
    splitk_side = nullptr;
    for (auto& r : prof) {
        ev_pool.push_back(r.e0);
        ev_pool.push_back(r.e1);
    }
    prof.clear();
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    ev_pool.clear();
    blocks.clear();
}

namespace {

// The operands of an ACE that depend on the label map and the style codes only -- never on the activations flowing through the generator:
// the SPADE hidden activations (label table) and the view of its style LUT (fc_mu + LUT GEMM / GEMV)
struct AcePrep {
    const float* actv = nullptr;
    const float* lut = nullptr;
    int lut_rs = 1, lut_ns = 0, lut_bs = LABEL_NC;
};
// What a chunk launches for one resolution level ahead of the level's ACEs: decided by Runner::plan_aces, launched by Runner::prepare
struct LevelPlan {
    bool classify[2] = {};                          // the SparseLevels classified [tiles of 32 x 8 | 32 x 16] (the direct exact-f32 route can need both) ...
    SeanModel::LevelMarks marks[2];                 // ... and the marks their interior maps carry (u5 == 253 + e16; frame marks)
    const SparseLevel* S = nullptr;                 // Winograd route: the classified level its quad lists and interior passes read (nullptr: every quad is a boundary quad)
    bool quads = false, gather = false;             // Winograd route: boundary-quad lists; ... with per-sample gather lists and chunk bases
    bool grouped = false;                           // ... the geometry joins the prologue's group instead of direct launches
    unsigned wino_lists = 0, sparse_lists = 0;      // the row-tile counts that need a Winograd task list / a sparse work list: bit i = entry i of Level::wq.works / Level::sp_work
    const uint8_t* hidden_u5 = nullptr;             // the interior map the level's hidden-activation passes may read (the rule: Runner::plan_aces)
};
// One ACE of one chunk: its route, what that route works on and where its operands come from, decided once (Runner::plan_aces) and read by everything else
struct AcePlan {
    const AceW* a = nullptr;
    AceRoute route = AceRoute::Dense;
    int r = 0, k = 0;                                    // level size of this call, level index
    const uint8_t* lab = nullptr;                        // the level's label map
    const SeanModel::WinoWork* W = nullptr;              // Winograd routes: the task list of the ACE's row tiles on its level (Level::wq)
    const SeanModel::WinoLevel* patch = nullptr;         // ... the level, when its pre-gathered patches may serve this ACE
    const SparseWork* sw = nullptr;                      // direct routes: work list to prepare (f16x3: also where the route then fell to Dense)
    int ti = -1;                                         // the classified SparseLevel this ACE's route reads: index into Level::sp / LevelPlan::classify (-1: none) ...
    SeanModel::LevelMarks marks;                         // ... and the marks of that classification
    bool compact = false;                                // Sparse, f16x3: pixel-level compaction inside the wave-specialised kernel
    const uint8_t* need = nullptr;                       // inline label-table kernel: the pixels / tiles the conv will read (nullptr: all)
    const int* tile_cnt = nullptr;
    const uint8_t* hidden_u5 = nullptr;                  // WinoQuads, sean.hidden_wq: LevelPlan::hidden_u5
    float* abuf = nullptr;                               // hidden activations of an inline launch: actv, or the level's padded planes
    int kout = HID;                                      // ... planes of the padded layout (one-hot planes behind the hidden channels)
    // where the operands come from: built inline before the ACE, ahead on the side stream, or by a grouped launch at the start of the chunk
    // (hidden planes: the prologue's HiddenGroup; LUT: the grouped GEMM)
    enum Src { NONE, INLINE, AHEAD, GROUP } hidden = INLINE, lut_src = NONE;      // (NONE: an unstyled ACE has no LUT)
    float* lut_buf = nullptr;                            // styled: where its LUT is built ...
    bool lut_gemv = false;                               // ... by the GEMV (else the GEMM) when it is built per ACE
    bool join = false;                                   // the ACE waits for its event of the side stream
    AcePrep q;                                           // the operands as the ACE kernels read them
    float *gtab = nullptr, *p6 = nullptr, *wsty = nullptr;            // interior tables and F(2x2) style images: the shared buffers, or this ACE's own ...
    bool pre_tables = false, pre_wsty = false;           // ... filled by the prologue's groups (else inline)
    bool wino() const { return route == AceRoute::F4 || route == AceRoute::WinoQuads; }      // padded layout, Winograd ACE kernels
};
struct AceIO { const float* noise; long long nf; const float* x; int x_up, act; float* out; };      // the operands every ACE parameter struct carries under the same names
struct SpStat { const int* stat = nullptr; double unit = 0.0, bytes_px = 0.0, bytes_fixed = 0.0, npix = 0.0; };      // work-list statistics of a sparse launch for its ProfRec (timed())

struct Runner {
    SeanModel& m;
    hipStream_t st;
    std::string err;
    int B, S;
    const SeanModel::ChunkMode mode;
    Runner(SeanModel& mm, hipStream_t s, int b, int sz, const uint8_t* labfull) : m(mm), st(s), B(b), S(sz), mode(mm.chunk_mode(b, sz)) { plan_aces(labfull); }

    void check(hipError_t e, const char* what) {
        if (e != hipSuccess && err.empty()) err = std::string(what) + ": " + hipGetErrorString(e);
    }
    hipEvent_t ev() {
        if (!m.ev_pool.empty()) {
            hipEvent_t e = m.ev_pool.back();
            m.ev_pool.pop_back();
            return e;
        }
        hipEvent_t e;
        check(hipEventCreate(&e), "hipEventCreate");
        return e;
    }
    template <class F>
    void timed(int kind, double flops, double bytes, F launch) { timed(kind, flops, bytes, SpStat(), launch); }
    double next_flops_exec = -1.0;      // set before a timed() whose matrix cores run fewer FLOPs than the dense count
    template <class F>
    void timed(int kind, double flops, double bytes, const SpStat& sp, F launch) {
        if (!m.prof_on) {
            next_flops_exec = -1.0;
            launch();
            return;
        }
        ProfRec r;
        r.kind = kind;
        r.flops = flops;
        r.bytes = bytes;
        r.sp_stat = sp.stat;
        if (sp.stat && m.prof_stats && m.prof_stats_used < m.prof_stats_cap) {
            // snapshot of the work list's statistics on the stream: a later chunk / step rebuilds the list
            int* slot = m.prof_stats + 4 * (size_t)m.prof_stats_used++;
            check(hipMemcpyAsync(slot, sp.stat, 4 * sizeof(int), hipMemcpyDeviceToDevice, st), "profile statistics snapshot");
            r.sp_stat = slot;
        }
        r.sp_flops_unit = sp.unit;
        r.sp_bytes_px = sp.bytes_px;
        r.sp_bytes_fixed = sp.bytes_fixed;
        r.sp_npix = sp.npix;
        r.flops_exec = next_flops_exec;
        next_flops_exec = -1.0;
        r.e0 = ev();
        r.e1 = ev();
        check(hipEventRecord(r.e0, st), "hipEventRecord");
        launch();
        check(hipEventRecord(r.e1, st), "hipEventRecord");
        m.prof.push_back(r);
    }
    void tap_sh16(const std::string& name, const float* src, int C, size_t hw, const AceW& producer) {
        auto it = m.taps.find(name);
        if (it == m.taps.end() || !it->second) return;
        if (m.opt.use_sh16)
            check(sh16_decode(src, it->second, B, C, (long long)hw, producer.out_scale, m.amax_slots + 2 * producer.index, st, m.opt.terms == 2,
                              m.opt.terms != 3), "tap decode");
        else check(hipMemcpyAsync(it->second, src, (size_t)B * C * hw * 4, hipMemcpyDeviceToDevice, st), "tap copy");
    }
    // f32 tensors between kernels are NCHW on the exact-f32 path and C4 ([B][C/4][HW][4]) on the f16x3 path
    void tap_c4(const std::string& name, const float* src, int C, size_t hw) {
        auto it = m.taps.find(name);
        if (it == m.taps.end() || !it->second) return;
        if (m.opt.use_sh16) check(c4_decode(src, it->second, B, C, (long long)hw, st), "tap decode");
        else check(hipMemcpyAsync(it->second, src, (size_t)B * C * hw * 4, hipMemcpyDeviceToDevice, st), "tap copy");
    }
    void tap(const std::string& name, const float* src, size_t floats) {
        auto it = m.taps.find(name);
        if (it != m.taps.end() && it->second)
            check(hipMemcpyAsync(it->second, src, floats * 4, hipMemcpyDeviceToDevice, st), "tap copy");
    }
    // overlap mode (sean_model.h, mode.overlap): interior passes on m.side_int beside the boundary convs, dynamic task claiming in the convs
    int claim_next = 0;
    unsigned* next_claim() {
        if (!m.claim_pool || claim_next >= SeanModel::CLAIM_SLOTS) return nullptr;
        return m.claim_pool + (size_t)SeanModel::CLAIM_WORDS * claim_next++;
    }
    // What this chunk has launched for a level so far -- bits only: what is launched at all is the LevelPlan's decision
    struct Launched {
        bool cls[2] = {}, quads = false;            // classification [tiles of 32 x 8 | 32 x 16]; boundary-quad lists
        unsigned wino_lists = 0, sparse_lists = 0;  // task / work lists, bits as in LevelPlan
        int geo_slot = -1;                          // the level's slot in the prologue's geometry group (set only while prologue() runs: geo)
    } launched[6];
    WinoGeoGroup* geo = nullptr;
    // The one prepare step: launches what the level plan lists for the route of this ACE and the chunk has not launched yet -- the classification
    // the ACE reads, the level's quad lists, the list of the ACE's row tiles.  Called for the first ACE that needs each piece on the inline path
    // (ace()), for every gather-route ACE up front by prepass() and prologue(); nothing is decided here.
    void prepare(const AcePlan& p) {
        const LevelPlan& lp = lplans[p.k];
        const SeanModel::Level& V = m.levels[p.k];
        Launched& ld = launched[p.k];
        const int r = p.r;
        if (p.ti >= 0 && lp.classify[p.ti] && !ld.cls[p.ti]) {
            const SparseLevel& S = V.sp[p.ti];
            const SeanModel::LevelMarks mk = lp.marks[p.ti];
            check(ace_classify(p.lab, S.u5, S.need, S.list, S.cnt, B, r, r, S.TH, st, mk.edges ? S.e16 : nullptr, mk.frame, memo_hit), "ace_classify");
            ld.cls[p.ti] = true;
        }
        if (p.route == AceRoute::WinoQuads) {
            const SeanModel::WinoLevel& L = V.wq;
            if (lp.quads && !ld.quads) {
                // the level's geometry: arguments of the grouped and of the direct launches alike (tile0: the grouped launcher's)
                const WinoGeoGroup::Level g{lp.S ? lp.S->u5 : nullptr, L.qlist, L.qcnt, L.pcnt, L.qoff, L.gq, L.gq_n, L.chunk_base, L.patch_mode,
                                            L.gq_cap, m.patchbuf ? m.patch_cap_chunks : 0, r, r, 0};
                if (lp.grouped && geo && geo->nl < WinoGeoGroup::MAX_L) {
                    ld.geo_slot = geo->nl;
                    geo->l[geo->nl++] = g;
                } else {
                    check(wino_quad_lists(g.u5, g.qlist, g.qcnt, g.pcnt, B, r, r, L.TH, st), "wino_quad_lists");
                    if (lp.gather) check(wino_gather_lists(g.qlist, g.qcnt, g.qoff, g.gq, g.gq_n, g.gq_cap, B, r, r, st), "wino_gather_lists");
                    if (lp.gather && g.chunk_base) check(wino_chunk_base(g.gq_n, B, g.cap_chunks, g.chunk_base, g.patch_mode, st), "wino_chunk_base");
                }
                ld.quads = true;
            }
            const unsigned bit = 1u << (p.W - L.works.data());
            if ((lp.wino_lists & bit) && !(ld.wino_lists & bit)) {
                if (geo && ld.geo_slot >= 0 && geo->nw < WinoGeoGroup::MAX_W) {
                    geo->w[geo->nw++] = WinoGeoGroup::Work{ld.geo_slot, p.W->nrt, p.W->work, p.W->total};
                } else {
                    // (a level collected by the prologue whose group has no room for this list: the group is launched first)
                    if (geo && ld.geo_slot >= 0) geo_flush();
                    const int tiles = (r / 32) * (r / L.TH);
                    if (lp.gather) check(wino_gather_worklist(L.gq_n, L.pcnt, B, tiles, p.W->nrt, p.W->work, p.W->total, st), "wino_gather_worklist");
                    else check(wino_ace_worklist(L.qcnt, L.pcnt, B * tiles, p.W->nrt, p.W->work, p.W->total, st), "wino_ace_worklist");
                }
                ld.wino_lists |= bit;
            }
        }
        if (p.sw) {
            const SparseWork& w = *p.sw;
            const SparseLevel& S = V.sp[p.ti];
            const unsigned bit = 1u << (p.sw - V.sp_work.data());
            if ((lp.sparse_lists & bit) && !(ld.sparse_lists & bit)) {
                const int ntiles = B * ((r + 31) / 32) * ((r + S.TH - 1) / S.TH);
                check(ace_worklist(S.cnt, ntiles, w.mtiles, w.work, w.total, st, w.mode, 32 * S.TH, w.work2, w.total2, w.work3), "ace_worklist");
                ld.sparse_lists |= bit;
            }
        }
    }
    // Label memo (sean_model.h): the device word the memoized launches of this chunk read, nullptr on a chunk that is not eligible.
    // memo_begin runs first in a chunk.  Eligible: the only chunk of its call, in prologue mode, with every gather level's geometry inside the
    // grouped launches (the direct launches of prepare() carry no memo word) and labels that can be read in 16-byte words.  Such a chunk
    // clears the pads of the memoized hidden planes where their geometry changed -- ahead of the decision: a memset must not follow it -- then
    // compares and decides; any other chunk of a handle with the memo clears MEMO_VALID, as does whatever left the memoized buffers in doubt.
    const int* memo_hit = nullptr;
    void memo_begin(const uint8_t* labfull, bool only_chunk) {
        if (!m.memo_state) return;
        bool ok = m.opt.label_memo && only_chunk && mode.prologue && (reinterpret_cast<uintptr_t>(labfull) & 15) == 0;
        int nl = 0, nw = 0;
        for (const LevelPlan& lp : lplans) {
            if (!lp.quads) continue;
            ok = ok && lp.grouped;
            ++nl;
            for (unsigned b = lp.wino_lists; b; b &= b - 1) ++nw;
        }
        ok = ok && nl <= WinoGeoGroup::MAX_L && nw <= WinoGeoGroup::MAX_W;
        bool fresh = m.memo_dirty;
        if (ok)
            for (const AcePlan& p : plans)
                if (p.hidden == AcePlan::GROUP) fresh = zero_pads(m.pro_actv[p.a->index], p.r, p.kout, st) || fresh;
        if (!ok || fresh) check(label_memo_invalidate(m.memo_state, st), "label memo (invalidate)");
        m.memo_dirty = false;
        if (!ok) return;
        check(label_memo_begin(labfull, m.memo_lab, (long long)B * S * S, m.memo_state, B, S, m.memo_epoch, st, (m.opt.spade_memo && m.spade_memo_on) ? 1 : 0),
              "label memo (compare, decide)");
        memo_hit = m.memo_state + MEMO_HIT;
        if (m.opt.spade_memo && m.spade_memo_on) spade_mode = m.memo_state + MEMO_SPADE_MODE;
    }
    // Code memo (sean_model.h): the device word that fc_mu_batched and the grouped LUT GEMM of this chunk read, nullptr on a chunk that is not
    // eligible.  Any chunk that is not eligible clears CODE_VALID: it may write mu_all or a lut_ahead buffer by another path.  Not while
    // profiling is enabled: its records time the launches that do the work (as the label memo, which needs the prologue, is off then).
    const int* code_hit = nullptr;
    void code_begin(const float* codes, bool only_chunk) {
        if (!m.code_state) return;
        const bool ok = m.opt.code_memo && only_chunk && mode.project_all && mode.grouped && !m.prof_on && (reinterpret_cast<uintptr_t>(codes) & 15) == 0;
        if (!ok || m.code_dirty) check(code_memo_invalidate(m.code_state, st), "code memo (invalidate)");
        m.code_dirty = false;
        if (!ok) return;
        check(code_memo_begin(codes, m.code_copy, (long long)B * LABEL_NC * STYLE * 4, m.code_state, B, m.memo_epoch, st), "code memo (compare, decide)");
        code_hit = m.code_state + CODE_HIT;
    }
    // SPADE memo (sean_model.h): the mode word of an eligible chunk, and which level sizes had their one-hot V image packed in this chunk
    const int* spade_mode = nullptr;
    bool v1h_done[2] = {false, false};
    void geo_flush() {
        if (!geo) return;
        geo->memo_hit = memo_hit;
        if (geo->nl) check(wino_geometry_grouped(*geo, st), "level geometry (grouped)");
        geo->nl = geo->nw = 0;
        for (Launched& l : launched) l.geo_slot = -1;
    }
    // The plan of the chunk: every ACE's route at (B, S), the lists, buffers and maps that route works on, where its operands come from, and what
    // is launched for its level first.  Decides only -- makes no HIP call, launches nothing; an inconsistency ends generate() here (err).
    //
    // The interior map a hidden-activation pass may read (LevelPlan::hidden_u5; with it the pass writes only the pixels a boundary quad's patch
    // reads): non-null only where the level's classification precedes the pass on the same stream or is joined to it by an event -- the inline
    // path (prepare() runs first in ace()), the prologue, and the prepass (classified on the main stream before the fork event of the side
    // stream).  In full run-ahead mode without prepass the hidden passes run on the side stream with no ordering to the classification, which
    // the main stream launches later: the map is null and they write every pixel.
    std::vector<AcePlan> plans;
    LevelPlan lplans[6];
    void plan_aces(const uint8_t* labfull) {
        const bool full = mode.ahead == SeanModel::ChunkMode::FULL;
        int n_hidden = 0, n_tables = 0, n_wsty = 0;      // members of the prologue's groups so far
        plans.assign(m.n_aces, AcePlan());
        for_each_ace(m.blocks, [&](const AceW& a) {
            AcePlan& p = plans[a.index];
            p.a = &a;
            p.k = level_of(a.res_div);
            p.r = S / a.res_div;
            const SeanModel::Level& V = m.levels[p.k];
            LevelPlan& lp = lplans[p.k];
            p.lab = a.res_div == 1 ? labfull : V.lab;
            p.route = m.ace_route(a, p.r, B);
            p.abuf = (p.wino() && V.actv) ? V.actv : m.actv;
            p.kout = a.styled ? HID + 20 : HID;
            p.gtab = m.gtab;
            auto classified = [&](int ti) {       // this ACE reads SparseLevel ti: classified once per chunk, with the level's marks
                const SeanModel::LevelMarks mk = m.level_marks(p.k, p.r, ti);
                if (lp.classify[ti] && (lp.marks[ti].edges != mk.edges || lp.marks[ti].frame != mk.frame) && err.empty())
                    err = "level plan: the ACEs of one level disagree on the straight-edge marks at " + a.name;
                lp.classify[ti] = true;
                lp.marks[ti] = p.marks = mk;
                p.ti = ti;
            };
            if (p.wino()) {
                p.W = m.wino_work(a, p.r);
                if (p.route == AceRoute::WinoQuads) {
                    // (pre-gathered patches: gather mode, not run-ahead -- the ahead buffers are per ACE -- and not beside an interior pass)
                    if (V.wq.gq && !full && m.patchbuf && !mode.overlap) p.patch = &V.wq;
                    // the interior reduction serves the level: the 32 x 16 classification if the handle has it, else the 32 x 8 one
                    if (m.opt.sparse && p.r >= m.opt.sparse_min_r && (V.sp[1].u5 || V.sp[0].u5)) {
                        classified(V.sp[1].u5 ? 1 : 0);
                        lp.S = &V.sp[p.ti];
                    }
                    lp.quads = true;
                    lp.gather = V.wq.gq != nullptr;
                    lp.grouped = mode.prologue && lp.gather && V.wq.TH == 16;      // (while the group has room: prepare())
                    lp.wino_lists |= 1u << (p.W - V.wq.works.data());
                    lp.hidden_u5 = (lp.S && !(full && !mode.prepass)) ? lp.S->u5 : nullptr;      // (the rule above)
                    p.hidden_u5 = m.opt.hidden_wq ? lp.hidden_u5 : nullptr;
                }
            } else if ((p.sw = m.sparse_work(a, p.r))) {
                // exact SPADE-interior reduction (ace_sparse.h).  f16x3 path: tile-skip mode, honoured by the wave-specialised kernel only
                // (conv_sh16.h) -- the lists of an ACE that kernel does not serve are still built
                classified(p.sw->TH == 16 ? 1 : 0);
                lp.sparse_lists |= 1u << (p.sw - V.sp_work.data());
                if (p.route == AceRoute::Sparse) {
                    p.compact = m.opt.use_sh16 && p.sw->mode >= 2;
                    // the label-table kernel only writes the hidden activations the conv will read -- not in full run-ahead mode (label tables
                    // ahead of the classification: every pixel)
                    // (exact-f32 path: skipping pixels of the NCHW planes made the kernel slower at every granularity tried -- it is bound by
                    // its LDS table reads, not by the writes; the map stays available behind sean.dbg bit 131072)
                    if (!full && (m.opt.use_sh16 ? p.compact : (m.opt.dbg & DBG_F32_NEED_MAP) != 0)) p.need = V.sp[p.ti].need;
                    if (!full && m.opt.use_sh16 && !p.compact) p.tile_cnt = V.sp[p.ti].cnt;
                }
            }
            // (every ACE of a level takes the Winograd routes or the direct ones: they read one interior map)
            if (lp.quads && lp.sparse_lists && err.empty()) err = "level plan: Winograd-route and direct-route ACEs on one level at " + a.name;
            // ---- operand sources ----
            // style LUT: the chunk's grouped GEMM, built ahead on the side stream (joined in ace()), or built inline before the ACE
            p.q.lut_ns = 18 * a.C;
            if (a.styled) {
                p.lut_src = mode.grouped ? AcePlan::GROUP : ((full || mode.ahead == SeanModel::ChunkMode::LUTS) ? AcePlan::AHEAD : AcePlan::INLINE);
                p.lut_buf = p.lut_src == AcePlan::INLINE ? m.lut : m.lut_ahead[a.index];
                p.q.lut = p.lut_buf;
                // built per ACE (build_lut): by a batched GEMV at interactive batch sizes, else a GEMM; on the f16x3 path one extra all-zero column per
                // sample (mu = 0 -> LUT = 0) that taps outside the image point at, and the GEMM writes C4
                p.q.lut_bs = (m.opt.use_sh16 && p.lut_src != AcePlan::GROUP) ? LABEL_NC + 1 : LABEL_NC;
                p.lut_gemv = p.lut_src != AcePlan::GROUP && a.lut_rows && B * p.q.lut_bs <= 64 && !m.opt.batch_inv;
                if (m.opt.use_sh16 && p.lut_src != AcePlan::GROUP && !p.lut_gemv) {
                    p.q.lut_rs = ((B * p.q.lut_bs + 31) / 32) * 32;
                    p.q.lut_ns = 4;
                }
            }
            // hidden planes: ahead on the side stream, from the prologue's group (F(4x4) route, its own buffer), or inline
            const bool pro_hidden = mode.prologue && p.route == AceRoute::F4 && m.pro_actv[a.index] && n_hidden < HiddenGroup::MAX;
            p.hidden = full ? AcePlan::AHEAD : (pro_hidden ? AcePlan::GROUP : AcePlan::INLINE);
            p.q.actv = full ? m.actv_ahead[a.index] : (pro_hidden ? m.pro_actv[a.index] : p.abuf);
            n_hidden += pro_hidden;
            p.join = full || p.lut_src == AcePlan::AHEAD;
            // gamma / beta table, column / row sums, F(2x2) style images: the prologue's (gather route; they read the style LUT, so styled ACEs
            // join only with the grouped LUT GEMM of the chunk) or the shared buffers, filled inline
            const bool with_lut = a.styled && p.q.lut;
            const bool p6 = p.marks.edges && with_lut;
            if (mode.prologue && p.route == AceRoute::WinoQuads && (!a.styled || (mode.grouped && p.q.lut))) {
                p.pre_tables = lp.S && m.pro_gtab[a.index] && (!p6 || m.pro_p6[a.index]) && n_tables < AceTableGroup::MAX;
                p.pre_wsty = a.styled && m.pro_wsty[a.index] && n_wsty < StylePackGroup::MAX;
                n_tables += p.pre_tables;
                n_wsty += p.pre_wsty;
            }
            if (p.pre_tables) p.gtab = m.pro_gtab[a.index];
            p.p6 = p6 ? (p.pre_tables ? m.pro_p6[a.index] : m.p6) : nullptr;
            p.wsty = with_lut ? (p.pre_wsty ? m.pro_wsty[a.index] : m.wsty) : nullptr;
        });
    }
    // classification, quad lists and task lists of every Winograd ACE level up front (labels only): the label tables that run ahead need the interior maps
    void prepass() {
        for (const AcePlan& p : plans)
            if (p.route == AceRoute::WinoQuads) prepare(p);
    }

    // The style LUT of one styled ACE (fc_mu + LUT GEMM / GEMV) into pl.lut_buf, on stream s; prof: the GEMM is a timed launch of the main stream.
    // (the view the consumers read: AcePlan::q, plan_aces)
    void build_lut(const AcePlan& pl, const float* codes, hipStream_t s, float* splitk, bool prof) {
        const AceW& a = *pl.a;
        float* lut_buf = pl.lut_buf;
        const int bs = pl.q.lut_bs;
        const int N = B * bs, npad = ((N + 31) / 32) * 32;
        const double fl = 2.0 * 18 * a.C * STYLE * N, by = 4.0 * (18.0 * a.C * STYLE + (double)STYLE * N + 18.0 * a.C * N);
        auto tm = [&](auto launch) { prof ? timed(2, fl, by, launch) : launch(); };
        if (pl.lut_gemv) {
            // interactive batch sizes: P[n][row] = sum_k W[row][k] mu[n][k] as a batched GEMV (weight-bandwidth bound)
            check(fc_mu(codes, a.fcmu_w, a.fcmu_b, m.mu_img, B, npad, s, m.mu_img, 0, bs, 1.f, nullptr, 0, 0, m.opt.pw_wide), "fc_mu");
            tm([&] { check(lut_gemv_mfma(m.mu_img, a.lut_rows, lut_buf, N, 18 * a.C, s), "lut gemv"); });
            return;
        }
        // LUT GEMM: 1x1 conv over the [npad/32 x 32] "image" of (sample, label) columns
        ConvParams p{};
        p.in = m.mu_img;
        p.wpk = a.lut_wpk;
        p.out = lut_buf;
        p.B = 1;
        p.Cin = STYLE;
        p.H = npad / 32;
        p.W = 32;
        p.Mrows = 18 * a.C;
        p.pad = -1;
        if (m.opt.use_sh16) {      // f16x3: C4 output
            unsigned* mu_slot = m.amax_slots + 2 * a.index + 1;
            if (m.fcmu_batched) {                    // projected at the start of the chunk, all ACEs in one launch
                p.in = m.mu_all + (size_t)a.index * m.mu_stride;
            } else {
                for (int pass = 0; pass < 2; ++pass)     // second pass: returns at once unless the first one left the f16 window
                    check(fc_mu(codes, a.fcmu_w, a.fcmu_b, m.mu_img, B, npad, s, nullptr, 1, bs, SH16_ACT_SCALE, mu_slot, pass, m.opt.terms == 2, m.opt.pw_wide), "fc_mu");
            }
            p.act = ACT_NONE;
            p.terms = m.opt.terms;
            p.wscale = a.lut_wscale;
            p.in_scale_inv = 1.f / SH16_ACT_SCALE;
            p.in_amax = mu_slot;
            p.out_mul = a.out_scale;           // the ACE epilogue takes the LUT pre-multiplied by its output scale
            p.partial = splitk;                // K = 512 in 32 chunks on few tiles (C <= 512): split-K fills the chip
            p.partial_cap = m.splitk_cap;
            tm([&] { check(conv_sh16_plain(p, 1, s), "lut gemm"); });
        } else {
            if (m.fcmu_batched && (N > 64 || m.opt.batch_inv)) p.in = m.mu_all + (size_t)a.index * m.mu_stride;      // projected at the start of the chunk (generate())
            else check(fc_mu(codes, a.fcmu_w, a.fcmu_b, m.mu_img, B, npad, s, nullptr, 0, 19, 1.f, nullptr, 0, 0, m.opt.pw_wide), "fc_mu");
            p.npix_valid = N;
            tm([&] { check(conv_nhwc1x1(p, s), "lut gemm"); });
        }
    }
    // the zero columns left and right of the image in a padded hidden buffer: the label-table kernels never write them, so they are cleared
    // whenever the buffer changes its geometry (first use, another image size) -- per-pixel pad stores cost 200 us per 512^2 launch
    // (returns whether it cleared the buffer)
    bool zero_pads(float* buf, int r, int kout, hipStream_t s) {
        const long long geo = ((long long)r << 20) | ((long long)kout << 8) | 1;
        auto it = m.pad_state.find(buf);
        if (it != m.pad_state.end() && it->second == geo) return false;
        check(hipMemsetAsync(buf, 0, (size_t)m.max_batch * kout * r * wino_apitch(r) * sizeof(float), s), "hidden activations: zero pads");
        m.pad_state[buf] = geo;
        return true;
    }
    // The SPADE hidden activations of one ACE (label table) into actv_buf, on stream s.  The route decides both the layout (Winograd routes:
    // padded planes, the one-hot planes of a styled ACE behind the hidden channels; else [B][128][H][W]) and the kernel that reads it.
    // the patch buffer of a gather-route ACE: its own on a chunk with the label memo, else the shared one
    float* patch_buf(const AcePlan& pl) const { return (memo_hit && m.memo_patch[pl.a->index]) ? m.memo_patch[pl.a->index] : m.patchbuf; }
    // ... the gamma / beta cache of an unstyled one (its patches, in the shared buffer, are not needed on a hit: the conv does not run)
    float* gb_cache(const AcePlan& pl) const { return (memo_hit && pl.patch && !pl.wsty) ? m.memo_gb[pl.a->index] : nullptr; }
    void build_hidden(const AcePlan& pl, hipStream_t s, float* actv_buf) {
        const AceW& a = *pl.a;
        const int r = pl.r, kout = pl.kout;
        const uint8_t* lab = pl.lab;
        // a buffer that held the padded planes of a Winograd level (zero columns cleared once per geometry) and now receives the
        // direct [B][HID][r][r] layout -- the same ACE at another image size on a run-ahead handle -- must have its pads cleared again
        // before the next padded use: the direct kernels write over them
        if (!pl.wino()) m.pad_state.erase(actv_buf);
        if (m.opt.use_sh16)
            check(onehot_conv3x3_sh16(lab, a.actv_table, a.actv_bias, actv_buf, B, r, r, HID, 1, a.actv_scale, s, m.opt.terms == 2, pl.need, pl.tile_cnt,
                                      (m.opt.dbg & DBG_ONEHOT_NO_COMPACT) ? 1 : 0), "mlp_shared");
        else if (pl.wino()) {
            // Winograd ACE path: hidden activations (+ the one-hot planes of a styled ACE, which feed the style k-steps) in one
            // persistent pass into the padded planes the ACE kernels read (conv_wino.h WINO_AXOFF), whole 64-byte groups of pixels
            // that a boundary quad's patch touches only (sean.hidden_wq = 0, F(4x4) levels, no interior map this pass may read: every pixel)
            zero_pads(actv_buf, r, kout, s);
            const uint8_t* u5 = pl.hidden_u5;
            const SeanModel::WinoLevel* PL = pl.patch;
            const bool pm = PL && PL->gq && PL->patch_mode && m.patchbuf;
            if (pm && mode.prologue && PL->chunk_base) {
                // chunks with the prologue: both sources from one launch, the device flag picks the body (kernels.h); with the label memo the
                // patches go to the ACE's own buffer and stay (patch_buf)
                check(spade_hidden_level(lab, u5, PL->gq, PL->gq_n, PL->gq_cap, PL->chunk_base, PL->patch_mode, a.actv_table,
                                         a.actv_bias, actv_buf, patch_buf(pl), B, r, r, kout, a.styled ? 1 : 0, wino_apitch(r), WINO_AXOFF, s,
                                         (patch_buf(pl) != m.patchbuf || gb_cache(pl)) ? memo_hit : nullptr),
                      "mlp_shared (planes or pre-gathered patches)");
                return;
            }
            check(spade_hidden_wq(lab, u5, a.actv_table, a.actv_bias, actv_buf, B, r, r, kout, a.styled ? 1 : 0, s,
                                  wino_apitch(r), WINO_AXOFF, pm ? PL->patch_mode : nullptr), "mlp_shared (boundary-quad patches)");
            // few, scattered boundary quads: their patches pre-gathered instead (one of the two kernels returns at once: device flag)
            if (pm) check(spade_hidden_patch(lab, PL->gq, PL->gq_n, PL->gq_cap, PL->chunk_base, PL->patch_mode, a.actv_table, a.actv_bias, m.patchbuf,
                                             B, r, r, kout, s), "mlp_shared (pre-gathered patches)");
        } else
            check(onehot_conv3x3(lab, a.actv_table, a.actv_bias, actv_buf, B, r, r, HID, 1, s, 0, pl.need), "mlp_shared");
    }

    // Small jobs (interactive renders: the chip is mostly empty) run every ACE's prepare step AHEAD on the model's side
    // stream, into per-ACE buffers, while the main stream walks the dependent chain of convs; an event per ACE joins them.
    // mode.ahead == LUTS (large jobs): only the style LUT builds run ahead; the label-table kernels stay inline.
    void prepare_all_ahead(const float* codes) {
        check(hipEventRecord(m.ev_fork, st), "fork");
        check(hipStreamWaitEvent(m.side, m.ev_fork, 0), "fork wait");
        for (const AcePlan& p : plans) {
            const AceW& a = *p.a;
            if (!p.join) continue;
            // (grouped LUT build: the launch on the main stream built it)
            if (p.lut_src == AcePlan::AHEAD) build_lut(p, codes, m.side, m.splitk_side, false);
            if (p.hidden == AcePlan::AHEAD) build_hidden(p, m.side, m.actv_ahead[a.index]);
            check(hipEventRecord(m.ev_join[a.index], m.side), "join record");
        }
    }

    // Exact-f32 path, more than 64 (sample, label) columns: the style LUTs P[(sample, label)][18 C] of ALL styled ACEs from one
    // grouped GEMM launch on the main stream (conv_pw.h; 15 separate launches of the generic 1x1 kernel took 3.6 ms of GPU time per
    // step on the side stream and delayed the persistent conv kernels they shared CUs with by 1.8 ms; inline 2.8 ms).  Operands
    // swapped: GEMM rows = the (sample, label) columns (A = the projected codes, packed by fc_mu_batched), "pixels" = the 18 C rows
    // of conv_gamma / conv_beta (normalization.py:172-173), so the output is the [n][18 C] layout the consumers read.
    void luts_grouped() {
        const int N = B * LABEL_NC;
        PwParams q{};
        q.Cin = STYLE;
        q.Cout = N;
        q.groups = static_cast<const PwGroup*>(m.lut_groups);
        q.ngroups = m.lut_ngroups;
        q.wide = m.opt.pw_wide && m.lut_groups_wide;
        q.skip = code_hit;
        const int nrg = ((N + 31) / 32 + 3) / 4;
        timed(2, 2.0 * m.lut_group_rows * STYLE * N, 4.0 * (m.lut_group_rows * STYLE + m.lut_group_rows * N + (double)m.lut_ngroups * STYLE * N),
              [&] { check(conv_pw_grouped(q, m.lut_group_tiles * nrg, st), "style LUTs (grouped GEMM)"); });
    }

    // ACE prologue (SeanModel::pro_on; large chunks of the exact-f32 Winograd path): what the ACEs of the chunk build from labels, codes and
    // weights alone, from a few grouped launches ahead of the first conv instead of small launches per level and per ACE between the convs
    // (profiles/r10_ace_prologue_kernel_trace.md: the dispatches of a step run back to back, a launch of a few blocks costs its 4.6 us floor
    // or, the 16 / 64-block hidden passes, 35 us of set-up latency whatever its size):
    //   * quad lists, per-sample lists, task lists and chunk bases of every gather-mode level (wino_geometry_grouped: four launches);
    //   * the padded hidden planes of every F(4x4)-route ACE (spade_hidden_wq_grouped);
    //   * gtab and P6 of every gather-route ACE (ace_tables_grouped) and its F(2x2) style images (wino_style_pack_grouped) -- these read the
    //     style LUTs, so they need the grouped LUT GEMM of the chunk (mode.grouped); without it only unstyled ACEs join.
    // The groups are filled here, per call, from the plan, which names their members (AcePlan::hidden == GROUP, pre_tables, pre_wsty: the set of
    // ACEs, their level sizes and label pointers follow B and S); every other ACE keeps its inline launches.  The level geometry of the gather-route
    // ACEs (classification, quad lists, task lists: prepare()) runs here too, ahead of the tables that follow its marks.
    // With the prologue on, the gather-mode levels also take their hidden activations -- planes or pre-gathered patches, a device flag decides
    // -- from one launch per ACE (spade_hidden_level) instead of two of which one returns at once.  Runs where mode.prologue says so.
    void prologue() {
        HiddenGroup hg{};
        AceTableGroup tg{};
        StylePackGroup sg{};
        WinoGeoGroup gg{};
        hg.B = tg.B = sg.B = gg.B = B;
        hg.memo_hit = memo_hit;
        geo = &gg;
        tg.lut_rs = 1;
        tg.lut_bs = LABEL_NC;
        tg.lut_mul = 1.f;
        for (const AcePlan& p : plans) {
            const AceW& a = *p.a;
            const int r = p.r;
            if (p.hidden == AcePlan::GROUP) {
                float* buf = m.pro_actv[a.index];
                zero_pads(buf, r, p.kout, st);
                // (lab, u5 = nullptr: F(4x4) levels, every pixel is read; table, bias, out, H, W, kout, onehot, pitch, xoff; the rest is the launcher's)
                hg.e[hg.n++] = HiddenGroup::Entry{p.lab, nullptr, a.actv_table, a.actv_bias, buf, r, r, p.kout, a.styled ? 1 : 0, wino_apitch(r), WINO_AXOFF};
            }
            if (p.route != AceRoute::WinoQuads) continue;
            prepare(p);      // (lists and task lists: into the geometry group)
            if (p.pre_tables) tg.e[tg.n++] = AceTableGroup::Entry{a.bias_g, a.bias_b, a.gconst, p.q.lut, p.gtab, p.p6, a.C};
            if (p.pre_wsty) sg.e[sg.n++] = StylePackGroup::Entry{p.q.lut, p.wsty, a.C};
        }
        geo_flush();
        geo = nullptr;
        check(spade_hidden_wq_grouped(hg, st), "mlp_shared (grouped, F(4x4)-route ACEs)");
        check(ace_tables_grouped(tg, st), "ace tables (grouped)");
        check(wino_style_pack_grouped(sg, st), "wino_style_pack (grouped)");
    }

    // one ACE: SPADE hidden activations (label LUT) -> fused gamma/beta conv + modulation -> h.  The plan names the route; what the routes
    // share -- the level's lists, the operands -- is launched here, then the route's own function runs.
    void ace(const AceW& a, const float* codes, const float* noise, size_t nf, size_t noff, const float* x, int x_up, int act, float* hout) {
        const AcePlan& p = plans[a.index];
        const AceIO io{noise + noff, (long long)nf, x, x_up, act, hout};
        prepare(p);
        // the operands (AcePlan::q) that are not in place yet: the LUT and the hidden planes the plan wants built inline, then the join with the side
        // stream for what was built ahead
        if (p.lut_src == AcePlan::INLINE) build_lut(p, codes, st, m.splitk_ws, true);
        if (p.hidden == AcePlan::INLINE) build_hidden(p, st, p.abuf);
        if (p.join) check(hipStreamWaitEvent(st, m.ev_join[a.index], 0), "join wait");
        switch (p.route) {
            case AceRoute::F4: return ace_f4(p, io);
            case AceRoute::WinoQuads: return ace_wino(p, io);
            case AceRoute::Sparse: return ace_sparse(p, io);
            case AceRoute::TinySplitK: return ace_tiny(p, io);
            case AceRoute::Dense: return ace_dense(p, io);
        }
    }
    // the same-named modulation operands of any ACE parameter struct (the interior pass takes its biases through gtab)
    template <class P>
    void fill_mod(P& t, const AcePlan& p, const AceIO& io) {
        const AceW& a = *p.a;
        t.x = io.x;
        t.x_up = io.x_up;
        t.act = io.act;
        t.out = io.out;
        t.B = B;
        t.C = a.C;
        t.H = t.W = p.r;
        t.bn_a = a.bn_a;
        t.bn_d = a.bn_d;
        t.nv = a.nv;
        t.noise = io.noise;
        t.noise_bstride = io.nf;
        if constexpr (!std::is_same<P, AceInteriorParams>::value) {
            t.bias_g = a.bias_g;
            t.bias_b = a.bias_b;
        }
    }
    // the interior pass over the classified level L: elementwise with the per-(sample, label) gamma/beta rows (ace_sparse.h); the route
    // sets what differs (impl, fill_min, variant, straight-edge tables, overlap and f16 fields)
    AceInteriorParams interior_params(const AcePlan& p, const AceIO& io, const SparseLevel& L) {
        AceInteriorParams ip{};
        fill_mod(ip, p, io);
        ip.u5 = L.u5;
        ip.cnt = L.cnt;
        ip.gtab = p.gtab;
        if (p.marks.edges) {      // straight-edge pixels served by the interior pass: table row of the code + three column / row sums of the style LUT
            ip.e16 = L.e16;
            ip.etab = p.a->edge_tab;
            ip.p6 = p.p6;
        }
        return ip;
    }
    double dense_flops(const AcePlan& p) const { return 2.0 * 2 * p.a->C * HID * 9 * ((double)B * p.r * p.r); }

    // F(4x4,3x3) over every tile of a low-resolution level (conv_wino4.h): nearly every tile holds a boundary pixel there -- no classification,
    // no interior pass, hidden activations at every pixel
    void ace_f4(const AcePlan& p, const AceIO& io) {
        const AceW& a = *p.a;
        const AcePrep& q = p.q;
        const int r = p.r;
        const double npix = (double)B * r * r;
        Wino4AceParams w{};
        fill_mod(w, p, io);
        w.actv = q.actv;
        w.wpk = a.spade_wino4;
        w.wsty = (a.styled && q.lut) ? m.wsty4 : nullptr;
        const int nks = w.wsty ? 38 : 32, ktot = 4 * nks;             // (38 / 32 k-steps of four channels)
        next_flops_exec = 2.0 * 32.0 * ((a.C + 15) / 16) * ktot * 36.0 * npix / 16.0;
        // 2 C GEMM rows over 128 (+ 20) input planes: the input transform once for all C / 8 row tiles (conv_wino4v.h; K: the buffer's plane count)
        Wino4vPackParams vp;
        const bool vroute = m.wino4v_route(wino4v_pays(2 * a.C, r), q.actv, B, r, p.kout, nks, vp, true);
        timed(1, dense_flops(p), 4.0 * (npix * p.kout + npix * a.C / (io.x_up ? 4.0 : 1.0) + npix * a.C), [&] {
            if (w.wsty) {
                const int rows = m.opt.pw_wide ? 1 : 0;
                if (rows && m.pad_state[m.wsty4] != 1) {      // the units that are zero at every B and C: once (conv_inst_wino4.hip)
                    check(hipMemsetAsync(m.wsty4, 0, m.wsty4_floats * sizeof(float), st), "wino4 style images: zero units");
                    m.pad_state[m.wsty4] = 1;
                }
                check(wino4_style_pack(q.lut, m.wsty4, B, a.C, st, rows), "wino4_style_pack");
            }
            if (vroute) {
                // SPADE memo: the same launches every call, the mode word picks which of them run -- PLAIN: pack + kernel<1> as ever;
                // STORE: the one-hot pack of the level (first memoized ACE of the level), pack + the memo instantiation; LOAD: the
                // memo instantiation alone, from the cache and the one-hot image of the STORE call
                const int vi = r == 64 ? 1 : 0;
                const long long tasks = (long long)B * (r / 32) * (r / 32) * ((a.C + 15) / 16);
                const bool memo = spade_mode && w.wsty && (r == 32 || r == 64) && m.memo_acc[a.index] && m.memo_v1h[vi] && tasks <= m.memo_acc_tasks[a.index];
                if (memo) {
                    if (!v1h_done[vi]) {
                        Wino4vPackParams v1 = vp;
                        v1.v = m.memo_v1h[vi];
                        v1.c0 = HID;
                        v1.nks = 6;
                        v1.memo_mode = spade_mode;
                        v1.memo_skip = (1 << SPADE_PLAIN) | (1 << SPADE_LOAD);
                        check(wino4v_pack(v1, st), "one-hot plane transform (winograd F(4x4,3x3), SPADE memo)");
                        v1h_done[vi] = true;
                    }
                    vp.memo_mode = spade_mode;
                    vp.memo_skip = 1 << SPADE_LOAD;
                    w.memo_mode = spade_mode;
                }
                check(wino4v_pack(vp, st), "hidden activation transform (winograd F(4x4,3x3))");
                w.v = m.vbuf;
                check(conv_wino4v_ace(w, st), "spade conv (winograd F(4x4,3x3), every tile, pre-transformed input)");
                if (memo) {
                    w.v1h = m.memo_v1h[vi];
                    w.acc_cache = m.memo_acc[a.index];
                    check(conv_wino4v_ace_memo(w, m.memo_acc_tasks[a.index], st), "spade conv (winograd F(4x4,3x3), SPADE memo)");
                }
            } else
                check(conv_wino4_ace(w, st), "spade conv (winograd F(4x4,3x3), every tile)");
        });
    }
    // F(2x2,3x3) over the boundary quads of the level (gather or tile mode, conv_wino.h); where the interior reduction serves the level
    // (LevelPlan::S), the interior pixels first, from tables
    void ace_wino(const AcePlan& p, const AceIO& io) {
        const AceW& a = *p.a;
        const AcePrep& q = p.q;
        const SparseLevel* S = lplans[p.k].S;
        const int r = p.r, x_up = io.x_up;
        const double npix = (double)B * r * r;
        const double xpp = 4.0 * a.C / (x_up ? 4.0 : 1.0), opp = 4.0 * a.C;
        const int ktot = p.kout;
        if (S) {
            AceInteriorParams ip = interior_params(p, io, *S);      // (P6 is built below)
            // four pixels per thread (16-byte stores) from 128 pixels of width: 530 -> 420 us on the up-sampled 512^2 launches
            // (tools/interior_bench.hip); level in the 100 ms step of round 3, measurable in this one
            ip.impl = r >= 128 ? 2 : 0;
            ip.groups = m.opt.int_groups;       // (tile4 kernel: channel groups per block, 0 = the launcher's rule; ace_sparse.hip)
            ip.onepass = m.opt.int_onepass;     // (tile4 kernel: 128 key slots and the narrow channel step for code-dense blocks)
            // (tile4 kernel, r >= 128: 0 = whole 128-byte lines that hold an interior pixel, ace_sparse.hip; sean.dbg bit 134217728: the
            //  block rule of rounds 3-5 for A/B)
            ip.fill_min = (x_up && r < 128) ? 257 : ((r >= 128 && !(m.opt.dbg & DBG_INTERIOR_FILL128)) ? 0 : 128);
            if (mode.overlap) {
                // beside the boundary conv of the same ACE (disjoint output pixels -- so no block may fill its boundary pixels),
                // on the few CUs of the side stream; the consumer of `out` waits for ev_int below
                ip.fill_min = 257;
                ip.quad_only = 1;
                ip.gtab = m.gtab_side;
                check(hipEventRecord(m.ev_x[a.index], st), "x ready");
                check(hipStreamWaitEvent(m.side_int, m.ev_x[a.index], 0), "x ready wait");
                check(ace_gtable(a.bias_g, a.bias_b, a.gconst, q.lut, q.lut_rs, q.lut_ns, q.lut_bs, 1.f, m.gtab_side, B, a.C, m.side_int), "ace_gtable");
                check(ace_interior_f32(ip, m.side_int), "ace interior");
                check(hipEventRecord(m.ev_int[a.index], m.side_int), "interior done");
            } else {
                timed(3, 0.0, 0.0, SpStat{p.W->total + 4, 0.0, xpp + opp + 5.0, 4.0 * 19 * 2 * a.C * B, npix}, [&] {
                    if (!p.pre_tables) {      // (else: the prologue filled this ACE's own)
                        check(ace_gtable(a.bias_g, a.bias_b, a.gconst, q.lut, q.lut_rs, q.lut_ns, q.lut_bs, 1.f, p.gtab, B, a.C, st), "ace_gtable");
                        if (p.p6) check(ace_p6table(q.lut, q.lut_rs, q.lut_ns, q.lut_bs, 1.f, p.p6, B, a.C, st), "ace_p6table");
                    }
                    check(ace_interior_f32(ip, st), "ace interior");
                });
            }
        }
        const SeanModel::WinoLevel& L = m.levels[p.k].wq;
        WinoAceParams w{};
        fill_mod(w, p, io);
        w.actv = q.actv;
        w.wpk = a.spade_wino;
        w.wsty = p.wsty;      // (style images: the shared buffer, packed below, or the prologue's)
        w.patch = p.patch ? patch_buf(p) : nullptr;
        w.chunk_base = L.chunk_base;
        w.patch_mode = L.patch_mode;
        w.qlist = L.qlist;
        w.TH = L.TH;
        w.qcnt = L.qcnt;
        w.work = p.W->work;
        w.total = p.W->total;
        w.zero = m.zero_page;
        w.gq = L.gq;
        w.gq_n = L.gq_n;
        w.gq_cap = L.gq_cap;
        w.claim = w.gq ? next_claim() : nullptr;
        w.cache = gb_cache(p);
        w.cache_cap = w.cache ? m.memo_gb_cap[a.index] : 0;
        w.memo_hit = w.cache ? memo_hit : nullptr;
        // executed FLOPs = wave tasks x (32 rows x 16 quads x 16 positions x K) x 2; dense = the direct conv over every pixel
        timed(1, dense_flops(p), 0.0, SpStat{p.W->total + 4, 2.0 * 32 * 16 * 16 * ktot, 4.0 * ktot + xpp + opp, 4.0 * 2.0 * a.C * ktot * 16, npix}, [&] {
            if (p.wsty && !p.pre_wsty) check(wino_style_pack(q.lut, p.wsty, B, a.C, st), "wino_style_pack");
            check(conv_wino_ace(w, st), "spade conv (winograd, boundary quads)");
        });
        if (mode.overlap && S) check(hipStreamWaitEvent(st, m.ev_int[a.index], 0), "interior done wait");
    }
    // the fused ACE conv of the direct routes (conv_mfma.h / conv_sh16.h): every pixel, or the work list the Sparse route adds
    ConvParams ace_conv_params(const AcePlan& pl, const AceIO& io) {
        const AceW& a = *pl.a;
        const AcePrep& q = pl.q;
        ConvParams p{};
        fill_mod(p, pl, io);
        p.in = q.actv;
        p.wpk = a.spade_wpk;
        p.Cin = HID;
        p.Mrows = 2 * a.C;
        p.lab = pl.lab;
        p.lut = q.lut;
        p.lut_rs = q.lut_rs;
        p.lut_ns = q.lut_ns;
        p.lut_bs = q.lut_bs;
        p.pad = -1;
        p.dbg = m.opt.dbg;
        p.terms = m.opt.terms;
        p.wscale = a.spade_wscale;
        p.in_scale_inv = 1.f / a.actv_scale;
        p.out_scale = a.out_scale;
        p.out_amax = m.amax_slots + 2 * a.index;
        if ((m.opt.dbg & DBG_STAMP) && a.index == m.opt.dbg_sel) p.partial = m.splitk_ws;      // cycle stamps of this launch (profiling)
        else p.dbg &= ~DBG_STAMP;
        return p;
    }
    double dense_bytes(const AcePlan& p, const AceIO& io) const {
        const double npix = (double)B * p.r * p.r, xin = npix * p.a->C / (io.x_up ? 4.0 : 1.0);
        return 4.0 * (npix * HID + xin + npix * p.a->C + 2.0 * p.a->C * HID * 9);
    }
    // interior pixels: elementwise with the per-(sample, label) gamma/beta rows; the others: conv over the compacted
    // boundary pixels (exact-f32 path) / over the tiles that hold a boundary pixel (f16x3 path)
    void ace_sparse(const AcePlan& pl, const AceIO& io) {
        const AceW& a = *pl.a;
        const AcePrep& q = pl.q;
        const SparseLevel& L = m.levels[pl.k].sp[pl.ti];
        const SparseWork* sw = pl.sw;
        const int r = pl.r, x_up = io.x_up;
        const bool compact = pl.compact;
        const double npix = (double)B * r * r;
        const double xpp = 4.0 * a.C / (x_up ? 4.0 : 1.0), opp = 4.0 * a.C;
        ConvParams p = ace_conv_params(pl, io);
        AceInteriorParams ip = interior_params(pl, io, L);
        ip.out_scale = a.out_scale;
        ip.out_amax = m.amax_slots + 2 * a.index;
        ip.bf16 = m.opt.terms == 2;
        ip.single = (m.opt.use_sh16 && m.opt.terms != 3 && !(m.opt.dbg & DBG_INTERIOR_NO_SINGLE)) ? 1 : 0;      // (dbg bit: A/B)
        ip.variant = m.opt.use_sh16 ? (compact ? 1 : 0) : (CH_ABL(m.opt.dbg & DBG_INTERIOR_VEC4) ? 1 : (CH_ABL(m.opt.dbg & DBG_INTERIOR_SECTORS) ? 2 : 0));
        // blocks of 32 x 8 pixels; mostly-interior blocks write every pixel (the conv below overwrites the boundary pixels).
        // Exact-f32 pass: filling pays only where x is read at full size (measured, tools/interior_bench.hip).
        // dbg bit 2097152: the row-shaped kernels of the first version (A/B)
        ip.impl = CH_ABL(m.opt.dbg & DBG_INTERIOR_ROWS) ? 1 : 0;
        ip.fill_min = m.opt.use_sh16 ? 128 : (x_up ? 257 : 128);
        // (impl 2, four pixels per thread: 10 % ahead at 512^2 in tools/interior_bench.hip, no difference in the generator
        // step -- 159.7 vs 159.9 images/s -- so the one-pixel kernel stays; dbg bit 16777216 selects it)
        if (!m.opt.use_sh16 && CH_ABL(m.opt.dbg & DBG_INTERIOR_TILE4) && r >= 128) {
            ip.impl = 2;
            ip.fill_min = 128;
        }
        p.sp_list = (m.opt.use_sh16 && !compact) ? nullptr : L.list;      // f16x3: the lists request the compacting kernel
        p.sp_cnt = L.cnt;
        p.sp_work = sw->work;
        p.sp_total = sw->total;
        p.sp_work2 = sw->work2;
        p.sp_total2 = sw->total2;
        p.sp_work3 = sw->work3;
        timed(3, 0.0, 0.0, SpStat{sw->total, 0.0, xpp + opp + 5.0, 4.0 * 19 * 2 * a.C * B, npix}, [&] {
            // (the f16x3 LUT is stored pre-multiplied by the ACE output scale)
            check(ace_gtable(a.bias_g, a.bias_b, a.gconst, q.lut, q.lut_rs, q.lut_ns, q.lut_bs, m.opt.use_sh16 ? 1.f / a.out_scale : 1.f,
                             m.gtab, B, a.C, st), "ace_gtable");
            if (pl.p6) check(ace_p6table(q.lut, q.lut_rs, q.lut_ns, q.lut_bs, 1.f / a.out_scale, pl.p6, B, a.C, st), "ace_p6table");
            check(m.opt.use_sh16 ? ace_interior_sh16(ip, st) : ace_interior_f32(ip, st), "ace interior");
        });
        timed(1, dense_flops(pl), 0.0, SpStat{sw->total, 32.0 * 64 * 2.0 * HID * 9, 4.0 * HID + xpp + opp, 4.0 * 2.0 * a.C * HID * 9, npix}, [&] {
            if (m.opt.use_sh16) check(conv_sh16_ace(p, st), "spade conv (tiles with boundary pixels)");
            else check(conv_ace_sparse(p, L.TH, st), "spade conv (boundary pixels)");
        });
        if (m.opt.use_sh16) {      // second passes: return at once unless the recorded maximum left the f16 window (sh16.h)
            ip.pass = 1;
            check(ace_interior_sh16(ip, st), "ace interior (second pass)");
            p.pass = 1;
            check(conv_sh16_ace(p, st), "spade conv (second pass)");
        }
    }
    // Tiny levels at small batches (one image at 16 x 16: 16 blocks of the fused kernel, 8 % of the CUs, 200 us): the SPADE conv as a
    // PLAIN conv over the same packed image -- which splits K over blocks when its grid is small (conv_mfma.h launch_conv) -- into
    // a scratch of gamma | beta sums, then ace_finish_f32 (style-LUT gathers, biases, modulation).  Same sums per element, the
    // split-K slabs added in order: deterministic.
    void ace_tiny(const AcePlan& pl, const AceIO& io) {
        const AceW& a = *pl.a;
        const AcePrep& q = pl.q;
        const int r = pl.r, rowsP = ((a.C + 31) / 32) * 64;
        ConvParams c = ace_conv_params(pl, io);
        c.out = m.gb_small;
        c.Mrows = rowsP;
        c.act = ACT_NONE;
        c.partial = m.splitk_ws;
        c.partial_cap = m.splitk_cap;
        c.dbg &= ~DBG_STAMP;
        timed(1, dense_flops(pl), dense_bytes(pl, io), [&] {
            check(conv_plain3(c, st), "spade conv (plain, split-K)");
            check(ace_finish_f32(m.gb_small, rowsP, io.x, io.x_up, a.bias_g, a.bias_b, a.bn_a, a.bn_d, a.nv, io.noise, io.nf, pl.lab, q.lut,
                                 io.out, B, a.C, r, r, io.act, st), "ace finish");
        });
    }
    void ace_dense(const AcePlan& pl, const AceIO& io) {
        ConvParams p = ace_conv_params(pl, io);
        timed(1, dense_flops(pl), dense_bytes(pl, io), [&] {
            if (!m.opt.use_sh16) {
                check(conv_ace(p, st), "spade conv");
                return;
            }
            check(conv_sh16_ace(p, st), "spade conv");
            p.pass = 1;        // returns at once unless the recorded maximum left the f16 window (sh16.h)
            check(conv_sh16_ace(p, st), "spade conv (second pass)");
        });
    }

    // fuse: optional (weights, input) of a 1x1 conv added into this 3x3 conv's accumulators (f16x3 path, W >= 32, no split-K)
    bool can_fuse_1x1(const ConvLayer& w, int r) const {
        return !(m.opt.dbg & DBG_NO_FUSE_1X1) && w.KS == 3 && r >= 32 && !conv_few_tiles(w.Cout, (long long)B * r * r);
    }
    // one plain conv call of this chunk as the routes see it (net_common.h): the handle's environment, the residual, split-K scratch
    ConvOpts conv_opts(const float* res, int res_up) const {
        ConvOpts o = m.conv_env();
        o.res = res;
        o.res_up = res_up;
        o.partial = m.opt.batch_inv ? nullptr : m.splitk_ws;      // (split-K follows the task count, i.e. the batch)
        o.partial_cap = m.splitk_cap;
        return o;
    }
    ConvRoute route(const ConvLayer& w, int r, const ConvOpts& o) const { return m.opt.use_sh16 ? ConvRoute::Direct : conv_route(w, B, r, r, o); }
    bool use_wino(const ConvLayer& w, int r) const { return route(w, r, conv_opts(nullptr, 0)) != ConvRoute::Direct; }
    // `prod` / `prod2`: the ACEs that wrote `in` / `in2` (their slots hold the scale in effect).  The generator's own: the fused second operand
    // w2 / in2 (direct kernels only), the amax slots, timed()
    void conv(const ConvLayer& w, const float* in, const AceW& prod, float* out, int r, const float* res, int res_up,
              const ConvLayer* w2 = nullptr, const float* in2 = nullptr, const AceW* prod2 = nullptr) {
        ConvOpts o = conv_opts(res, res_up);
        const ConvRoute rt = w2 ? ConvRoute::Direct : route(w, r, o);
        const ConvFigures f = conv_figures(rt, w, (double)B * r * r, res != nullptr, w2 ? w2->Cin : 0);
        next_flops_exec = f.flops_exec;
        if (rt != ConvRoute::Direct) {
            if (rt == ConvRoute::F2) o.claim = next_claim();
            timed(0, f.flops, f.bytes, [&] { check(run_conv(rt, w, in, out, B, r, r, o, st), "conv (winograd / 1x1 GEMM)"); });
            return;
        }
        ConvParams p = conv_direct_params(w, in, out, B, r, r, o);
        if (w2) {
            p.in2 = in2;
            p.wpk2 = m.opt.use_sh16 ? w2->sh_wpk : w2->wpk;
            p.Cin2 = w2->Cin;
            p.in2_amax = m.amax_slots + 2 * prod2->index;
        }
        p.in_amax = m.amax_slots + 2 * prod.index;
        p.dbg = m.opt.dbg;
        p.terms = m.opt.terms;
        if (m.opt.use_sh16) p.wpk = w.sh_wpk;
        p.wscale = w.sh_wscale;                    // shared with w2's rows when a 1x1 operand is fused (build())
        p.in_scale_inv = 1.f / prod.out_scale;     // inputs are ACE outputs (a fused second operand: see sh16_in_scale_inv)
        p.mtiles_hint_small = conv_few_tiles(w.Cout, (long long)B * r * r) ? 1 : 0;
        timed(0, f.flops, f.bytes, [&] {
            if (m.opt.use_sh16) check(conv_sh16_plain(p, w.KS, st), "conv");
            else check(w.KS == 3 ? conv_plain3(p, st) : conv_plain1(p, st), "conv");
        });
    }
};

// ---- encode(): one chunk of the Zencoder (architecture.py:158-207), stage by stage --------------------------------------------------
// Buffers: stem -> hs; f16x3 kernels (f16path): h0 -> dx -> h1 -> hs -> dx -> hs -> h1 -> h0; exact f32: hs -> dx -> h1 -> hs -> h0.
struct ZencRunner {
    SeanModel& m;
    const int B, S;
    hipStream_t st;
    const int h2 = S / 2, h4 = S / 4;
    const bool f16path = m.opt.use_sh16 && h4 * h4 >= 4096;      // every conv after the stem on the f16x3 kernels
    ConvOpts env = zenc_env(m);
    static ConvOpts zenc_env(const SeanModel& m) {      // the Zencoder's routes follow its images alone (build() packs them by sean.wino)
        ConvOpts o = m.conv_env();
        o.wino = 2;
        return o;
    }
    std::string err;
    void ck(hipError_t e, const char* what) {
        if (e != hipSuccess && err.empty()) err = std::string(what) + ": " + hipGetErrorString(e);
    }
    // the f16x3 conv of layer L over an instance-normalised input of hw_in pixels (bounded by sqrt(HW): static scale), output side H
    ConvParams sh16(const ConvLayer& L, const float* in, float* out, int hw_in, int H) const {
        return sh16_conv_params(L, in, out, B, H, H, instnorm_sh16_scale(hw_in));
    }
    void stem(const float* x) {
        ck(conv3x3_c3_reflect(x, m.z1_w, m.z1.bias, m.hs, B, 32, S, S, st), "zenc conv1");
        if (f16path) ck(instnorm_act(m.hs, B * 32, S * S, 1e-5f, ACT_LRELU, st, m.h0, 32, m.splitk_ws), "zenc in1");
        else ck(instnorm_act(m.hs, B * 32, S * S, 1e-5f, ACT_LRELU, st), "zenc in1");
    }
    // the two stride-2 convs, each followed by its InstanceNorm + lrelu (f16x3: space-to-depth form, SH16 -> C4 -> SH16)
    void down() {
        if (f16path) {
            ck(conv_sh16_s2d(sh16(m.z4_s2d, m.h0, m.dx, S * S, h2), m.z4_s2d.KS, st), "zenc conv2 (f16x3)");
            ck(instnorm_c4_to_sh16(m.dx, B, 64, h2 * h2, 1e-5f, ACT_LRELU, m.h1, st, m.splitk_ws), "zenc in2");
            ck(conv_sh16_s2d(sh16(m.z7_s2d, m.h1, m.hs, h2 * h2, h4), m.z7_s2d.KS, st), "zenc conv3 (f16x3)");
            ck(instnorm_c4_to_sh16(m.hs, B, 128, h4 * h4, 1e-5f, ACT_LRELU, m.dx, st, m.splitk_ws), "zenc in3");
        } else {
            ck(run_conv(m.z4, m.hs, m.dx, B, S, S, env, st), "zenc conv2");
            ck(instnorm_act(m.dx, B * 64, h2 * h2, 1e-5f, ACT_LRELU, st), "zenc in2");
            ck(run_conv(m.z7, m.dx, m.h1, B, h2, h2, env, st), "zenc conv3");
            ck(instnorm_act(m.h1, B * 128, h4 * h4, 1e-5f, ACT_LRELU, st), "zenc in3");
        }
    }
    // exact f32, enough pixel tiles to fill the device: four phase GEMMs over shifted views (the V buffer is free until conv5's transform pass);
    // the InstanceNorm + lrelu that follows reads the phase planes and writes the depth-to-space plane
    bool convt_phase_gemms() {
        const long long hw4 = (long long)h4 * h4;
        if (!(m.z10_pw[3].pw && !m.opt.use_sh16 && !m.opt.batch_inv && pw_supported(128, 256, (int)hw4) && (h4 & 3) == 0 && (long long)B * hw4 >= 16384 && m.vbuf &&
              (size_t)B * (512 + 4 * 256) * hw4 * sizeof(float) <= m.vbuf_bytes))
            return false;
        float *xs = m.vbuf, *tph = m.vbuf + (size_t)B * 512 * hw4;
        ck(convt_shift4(m.h1, xs, B, 128, h4, h4, st), "zenc convT shifted views");
        static const int first[4] = {1, 0, 1, 0};
        for (int ph = 0; ph < 4; ++ph) {
            const ConvLayer& L = m.z10_pw[ph];
            PwParams q{};
            q.in = xs + (size_t)first[ph] * 128 * hw4;
            q.in_bs = 512 * hw4;
            q.wpk = L.pw;
            q.out = tph + (size_t)ph * B * 256 * hw4;
            q.B = B;
            q.Cin = L.Cin;
            q.Cout = L.Cout;
            q.HW = (int)hw4;
            q.wide = m.opt.pw_wide;
            ck(conv_pw(q, st), "zenc convT (phase GEMM)");
        }
        ck(instnorm_act_d2s(tph, m.z10.bias, m.hs, B, 256, h4, h4, 1e-5f, ACT_LRELU, st), "zenc in4 (depth-to-space)");
        return true;
    }
    // the ConvTranspose and the InstanceNorm + lrelu that follows it
    void conv_transpose() {
        if (f16path) {
            if (m.opt.dbg & DBG_ZENC_ZEROINS) {         // the earlier form, kept for comparison: 3x3 conv over the zero-inserted x2 view
                ConvParams t = sh16(m.z10, m.dx, m.hs, h4 * h4, h2);
                t.in_mode = IN_UP2_ZEROINS;
                ck(conv_sh16_plain(t, 3, st), "zenc convT (f16x3)");
            } else                           // 2x2-tap conv at the input resolution, depth-to-space store
                ck(conv_sh16_d2s(sh16(m.z10_d2s, m.dx, m.hs, h4 * h4, h4), st), "zenc convT (f16x3, depth-to-space)");
            ck(instnorm_c4_to_sh16(m.hs, B, 256, h2 * h2, 1e-5f, ACT_LRELU, m.h1, st, m.splitk_ws), "zenc in4");
            return;
        }
        if (convt_phase_gemms()) return;
        if (conv_route(m.z10_wino, B, h4, h4, env) == ConvRoute::F2)
            ck(run_conv(ConvRoute::F2, m.z10_wino, m.h1, m.hs, B, h4, h4, env, st), "zenc convT (winograd phase convs)");
        else {
            ConvOpts zins = env;
            zins.in_mode = IN_UP2_ZEROINS;
            ck(run_conv(m.z10, m.h1, m.hs, B, h4, h4, zins, st), "zenc convT");
        }
        if (m.opt.use_sh16) ck(instnorm_act(m.hs, B * 256, h2 * h2, 1e-5f, ACT_LRELU, st, m.h1, 256), "zenc in4");
        else ck(instnorm_act(m.hs, B * 256, h2 * h2, 1e-5f, ACT_LRELU, st), "zenc in4");
    }
    // the reflection-padded 256 -> 512 conv with tanh (91 % of the Zencoder FLOPs)
    void conv5() {
        if (m.opt.use_sh16) {
            ConvParams p = sh16(m.z14, m.h1, m.h0, h2 * h2, h2);
            p.act = ACT_TANH;
            p.pad_mode = PAD_REFLECT;
            ck(conv_sh16_plain(p, 3, st), "zenc conv5 (f16x3)");
            return;
        }
        ConvOpts last = env;
        last.pad_mode = PAD_REFLECT;
        last.act = ACT_TANH;
        if (last.v_pays) last.v_pays = 1;      // 512 GEMM rows: the (reflected) input transform in its own pass at every size V fits
        ck(run_conv(m.z14, m.hs, m.h0, B, h2, h2, last, st), "zenc conv5");
    }
    void means(const uint8_t* labels, float* codes) {
        ck(region_mean(m.h0, labels, codes, B, STYLE, h2, h2, S, st, m.opt.use_sh16 ? 1 : 0), "region_mean");
        auto it = m.taps.find("zenc.feat");
        if (it != m.taps.end() && it->second) {
            if (m.opt.use_sh16) ck(c4_decode(m.h0, it->second, B, STYLE, (long long)h2 * h2, st), "tap");
            else ck(hipMemcpyAsync(it->second, m.h0, (size_t)B * STYLE * h2 * h2 * 4, hipMemcpyDeviceToDevice, st), "tap");
        }
    }
};

}  // namespace

// seed of the planes of the batch chunk that starts at sample `bo` (ch_sean_generate with noise == NULL, ch_sean_draw_noise)
static uint64_t chunk_seed(uint64_t seed, int bo) { return seed + 0x632BE59BD9B4E019ull * (uint64_t)(bo + 1); }

std::string SeanModel::draw_noise(uint64_t seed, float* out, int Btot, int S, hipStream_t st) {
    if (blocks.empty()) return "model not finalized";
    if (S % 32 != 0 || S < 32 || S > max_size) return "S must be a multiple of 32 and <= max_size";
    const size_t nf = noise_floats(S);
    for (int bo = 0; bo < Btot; bo += max_batch) {
        const int B = std::min(max_batch, Btot - bo);
        if (gen_noise(out + (size_t)bo * nf, (long long)B * nf, chunk_seed(seed, bo), st) != hipSuccess) return "gen_noise failed";
    }
    return "";
}

std::string SeanModel::generate(const uint8_t* labels, const float* codes, const float* noise, uint64_t seed,
                                float* out, int Btot, int S, hipStream_t st) {
    if (blocks.empty()) return "model not finalized";
    if (S % 32 != 0 || S < 32 || S > max_size) return "S must be a multiple of 32 and <= max_size";
    if (Btot < 1) return "B must be >= 1";
    const size_t nf = noise_floats(S);
    // overlap handles: everything runs on the internal main stream (the CU-masked side streams are blocking streams: work on the
    // caller's stream, if that is the NULL stream, would serialise with them), forked from and joined to the caller's stream
    hipStream_t st_user = st;
    if (overlap_on) {
        if (hipEventRecord(ev_in, st_user) != hipSuccess || hipStreamWaitEvent(main_i, ev_in, 0) != hipSuccess) return "overlap mode: fork failed";
        st = main_i;
    }
    auto join = [&](const std::string& e) {
        if (overlap_on && (hipEventRecord(ev_out, main_i) != hipSuccess || hipStreamWaitEvent(st_user, ev_out, 0) != hipSuccess) && e.empty())
            return std::string("overlap mode: join failed");
        return e;
    };
    for (int bo = 0; bo < Btot; bo += max_batch) {
        const int B = std::min(max_batch, Btot - bo);
        const uint8_t* lab = labels + (size_t)bo * S * S;
        Runner R(*this, st, B, S, lab);
        if (!R.err.empty()) return join(R.err);      // (the plan: nothing has been launched)
        const ChunkMode& mode = R.mode;
        if (claim_pool) R.check(hipMemsetAsync(claim_pool, 0, (size_t)CLAIM_SLOTS * CLAIM_WORDS * sizeof(unsigned), st), "claim counters");
        const float* cd = codes + (size_t)bo * LABEL_NC * STYLE;
        const float* nz;
        if (noise) {
            nz = noise + (size_t)bo * nf;
        } else {
            R.check(gen_noise(noise_ws, (long long)B * nf, chunk_seed(seed, bo), st), "gen_noise");
            nz = noise_ws;
        }
        R.memo_begin(lab, Btot <= max_batch);
        for (int k = 1; k <= 5; ++k) R.check(label_downsample(lab, levels[k].lab, B, S, S >> k, st, R.memo_hit), "label_downsample");
        if (opt.use_sh16) R.check(hipMemsetAsync(amax_slots, 0, 64 * sizeof(unsigned), st), "amax slots");
        R.code_begin(cd, Btot <= max_batch);
        if (mode.project_all) {     // (smaller batches take the GEMV branch of Runner::build_lut, which projects per ACE)
            // grouped LUT build: the projections are its A operand, written in fragment order (sh16 = 2: pack_pw_A layout); with the code memo
            // both launches return at once on a chunk that brings the codes of the previous one
            R.check(fc_mu_batched(cd, fcmu_w_ptrs, fcmu_b_ptrs, mu_all, mu_stride, n_aces, B, ((B * LABEL_NC + 31) / 32) * 32, LABEL_NC, 1.f,
                                  nullptr, 0, 0, st, mode.grouped ? 2 : 0, opt.pw_wide, R.code_hit), "fc_mu (all ACEs)");
            if (mode.grouped) R.luts_grouped();
        } else if (fcmu_batched && opt.use_sh16) {
            const int npad_c = ((B * (LABEL_NC + 1) + 31) / 32) * 32;
            for (int pass = 0; pass < 2; ++pass)         // second pass: returns at once unless a projection left the f16 window
                R.check(fc_mu_batched(cd, fcmu_w_ptrs, fcmu_b_ptrs, mu_all, mu_stride, n_aces, B, npad_c, LABEL_NC + 1, SH16_ACT_SCALE,
                                      amax_slots, pass, opt.terms == 2, st, 1, opt.pw_wide), "fc_mu (all ACEs)");
        }
        // interactive-size jobs: everything that depends on labels / codes only runs ahead on the side stream
        // (chunk_mode; large jobs run only the style LUT builds -- small, latency-bound GEMMs -- ahead, in the tails of the conv kernels: exact-f32
        // path, B = 16 at 512^2: 147.2 -> 148.3 images/s)
        if (mode.prepass) R.prepass();
        if (mode.ahead != ChunkMode::NONE) R.prepare_all_ahead(cd);
        // large chunks: the label / code-only products of the ACEs from grouped launches, ahead of the first conv (no tap reads any of them)
        if (mode.prologue) R.prologue();

        const int sw = S / 32;
        float* x = xa;
        float* y = xb;
        R.check(onehot_conv3x3(levels[5].lab, fc_table, fc_bias, x, B, sw, sw, 16 * ngf, 0, st, opt.use_sh16 ? 1 : 0), "fc");
        R.tap_c4("fc", x, 16 * ngf, (size_t)sw * sw);
        size_t noff = 0;
        for (const auto& b : blocks) {
            const int r = S / b.res_div;
            const size_t rr = (size_t)r * r;
            const int up = b.up_before ? 1 : 0;
            const float* xsrc = x;   // block input (at r/2 when up_before)
            const float* shortcut;
            int sc_up;
            bool fuse_s = false;
            if (b.learned) {
                R.ace(b.ace_s, cd, nz, nf, noff, xsrc, up, ACT_NONE, hs);
                noff += rr;
                R.tap_sh16(b.name + ".hs", hs, b.fin, rr, b.ace_s);
                // the 1x1 shortcut conv is folded into conv_1 (extra K chunks on a second input) unless a test taps its output
                // (not on the Winograd path: there the shortcut stays a direct 1x1 GEMM whose output conv_1 adds as its residual)
                fuse_s = R.can_fuse_1x1(b.conv_1, r) && !taps.count(b.name + ".xs") && !R.use_wino(b.conv_1, r);
                if (!fuse_s) {
                    R.conv(b.conv_s, hs, b.ace_s, xs, r, nullptr, 0);
                    R.tap_c4(b.name + ".xs", xs, b.fout, rr);
                }
                shortcut = fuse_s ? nullptr : xs;
                sc_up = 0;
            } else {
                shortcut = xsrc;
                sc_up = up;
            }
            R.ace(b.ace_0, cd, nz, nf, noff, xsrc, up, ACT_LRELU, h0);
            noff += rr;
            R.tap_sh16(b.name + ".h0", h0, b.fin, rr, b.ace_0);
            R.conv(b.conv_0, h0, b.ace_0, dx, r, nullptr, 0);
            R.tap_c4(b.name + ".dx", dx, b.fmid, rr);
            R.ace(b.ace_1, cd, nz, nf, noff, dx, 0, ACT_LRELU, h1);
            noff += rr;
            R.tap_sh16(b.name + ".h1", h1, b.fmid, rr, b.ace_1);
            R.conv(b.conv_1, h1, b.ace_1, y, r, shortcut, sc_up, fuse_s ? &b.conv_s : nullptr, fuse_s ? hs : nullptr, fuse_s ? &b.ace_s : nullptr);
            R.tap_c4(b.name, y, b.fout, rr);
            std::swap(x, y);
        }
        R.check(conv_img_tanh(x, img_w, img_b, out + (size_t)bo * 3 * S * S, B, ngf, S, S, st, opt.use_sh16 ? 1 : 0, img_w4), "conv_img");
        if (!R.err.empty()) memo_dirty = code_dirty = true;      // (the decision kernels may have run ahead of a launch that failed)
        if (!R.err.empty()) return join(R.err);
    }
    return join("");
}

// phase: 0 = the whole encoder; 1 = the convolutional part only (feature map stays in the workspace; one chunk: Btot <=
// max_batch); 2 = the region means over the feature map of the preceding phase-1 call (same Btot, S).  The split lets a caller
// compute the label map concurrently with the convs: the labels are only needed by the means (architecture.py:185-205).
std::string SeanModel::encode(const float* img, const uint8_t* labels, float* codes_out, int Btot, int S,
                              hipStream_t st, int phase) {
    if (blocks.empty() || !has_zencoder) return "Zencoder weights not loaded/finalized";
    if (S % 32 != 0 || S < 32 || S > max_size) return "S must be a multiple of 32 and <= max_size";
    if (phase != 0 && Btot > max_batch) return "split encode: B must not exceed max_batch";
    if (phase == 1) { enc_pending_B = Btot; enc_pending_S = S; }
    if (phase == 2 && (enc_pending_B != Btot || enc_pending_S != S)) return "split encode: no matching ch_sean_encode_features call";
    if (phase == 2) enc_pending_B = 0;
    for (int bo = 0; bo < Btot; bo += max_batch) {
        ZencRunner R{*this, std::min(max_batch, Btot - bo), S, st};
        if (phase != 2) {
            R.stem(img + (size_t)bo * 3 * S * S);
            R.down();
            R.conv_transpose();
            R.conv5();
        }
        if (phase != 1) R.means(labels + (size_t)bo * S * S, codes_out + (size_t)bo * LABEL_NC * STYLE);
        if (!R.err.empty()) return R.err;
    }
    return "";
}

std::string SeanModel::label_memo_stats(int* calls, int* hits) {
    int st[MEMO_WORDS] = {};
    if (memo_state && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(st, memo_state, sizeof st, hipMemcpyDeviceToHost) != hipSuccess))
        return "label memo: state read failed";
    *calls = st[MEMO_CALLS];
    *hits = st[MEMO_HITS];
    return "";
}
std::string SeanModel::spade_memo_stats(int* stores, int* loads) {
    int st[MEMO_WORDS] = {};
    if (memo_state && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(st, memo_state, sizeof st, hipMemcpyDeviceToHost) != hipSuccess))
        return "SPADE memo: state read failed";
    *stores = st[MEMO_STORES];
    *loads = st[MEMO_LOADS];
    return "";
}

std::string SeanModel::code_memo_stats(int* calls, int* hits) {
    int st[CODE_WORDS] = {};
    if (code_state && (hipDeviceSynchronize() != hipSuccess || hipMemcpy(st, code_state, sizeof st, hipMemcpyDeviceToHost) != hipSuccess))
        return "code memo: state read failed";
    *calls = st[CODE_CALLS];
    *hits = st[CODE_HITS];
    return "";
}

ConvOpts SeanModel::conv_env() const {
    ConvOpts o;
    o.wino = opt.wino;
    o.wino4_force = opt.wino4_force;
    o.batch_inv = opt.batch_inv;
    o.wino4_split = opt.wino4_split;
    o.v_pays = opt.wino4v ? -1 : 0;
    o.pw_wide = opt.pw_wide;
    o.num_cus = num_cus;
    o.vbuf = vbuf;
    o.vbuf_bytes = vbuf_bytes;
    o.zero = zero_page;
    return o;
}

// ---- routes and modes: host decisions only ----------------------------------------------------------------------------------------
// The Winograd ACE routes need the level's quad lists and the task list of this row-tile count, sized at build time (they exist where
// (max_size >> k) % 32 == 0; a smaller S can reach a 32-grid level that max_size does not have, e.g. max_size = 96, S = 64 -- ADVICE r04);
// else the ACE takes the direct kernels and their [B][128][H][W] layout
const SeanModel::WinoWork* SeanModel::wino_work(const AceW& a, int r) const {
    if (!(opt.wino && !opt.use_sh16 && a.spade_wino && r >= 32 && r % 32 == 0)) return nullptr;
    const WinoLevel& L = levels[level_of(a.res_div)].wq;
    if (!L.qlist) return nullptr;
    for (const auto& w : L.works)
        if (w.nrt == (a.C + 15) / 16) return &w;
    return nullptr;
}
const SparseWork* SeanModel::sparse_work(const AceW& a, int r) const {
    if (!opt.sparse || r < opt.sparse_min_r || r < 32) return nullptr;
    const Level& L = levels[level_of(a.res_div)];
    for (const auto& w : L.sp_work)
        if (w.mtiles == (a.C + 31) / 32) return L.sp[w.TH == 16 ? 1 : 0].u5 ? &w : nullptr;
    return nullptr;
}
SeanModel::LevelMarks SeanModel::level_marks(int k, int r, int ti, bool built) const {
    const Level& L = levels[k];
    // the interior passes that know the codes: the tile4 kernel of the exact-f32 Winograd path and the compacting f16 kernels, from 128 pixels
    bool e = opt.edge && (opt.use_sh16 ? opt.sparse : opt.wino) && r >= 128;
    if (e && built) {
        // ... on a classified level with a code plane whose ACEs carry the table rows and, styled ACEs, have room for their column / row sums
        e = opt.sparse && L.sp[ti].e16 && L.edge_tab && (!L.styled || p6);
        // f16 paths: work lists of the compacting kernel (sean.sh16_compact: mode >= 2).  Exact f32: the level takes the Winograd route at r,
        // and not on an overlap handle (quad_only interior pass)
        if (opt.use_sh16) e = e && !L.sp_work.empty() && L.sp_work[0].mode >= 2;
        else e = e && L.wq.qlist && r % 32 == 0 && !overlap_on;
    }
    LevelMarks mk;
    mk.edges = e;
    mk.frame = e && !opt.use_sh16 && opt.frame;      // frame pixels: only the tile4 kernel knows their codes
    return mk;
}
AceRoute SeanModel::ace_route_shape(const AceW& a, int r) const {
    if (wino_work(a, r)) {
        // F(4x4,3x3) over every tile: the low-resolution levels, where nearly every tile holds a boundary pixel
        const bool f4 = opt.wino >= 2 && a.spade_wino4 && r <= opt.wino4_ace_max_r && wino4_ace_supported(r, r, a.C) && (!a.styled || wsty4);
        return f4 ? AceRoute::F4 : AceRoute::WinoQuads;
    }
    return sparse_work(a, r) ? AceRoute::Sparse : AceRoute::Dense;
}
AceRoute SeanModel::ace_route(const AceW& a, int r, int B) const {
    const AceRoute s = ace_route_shape(a, r);
    if (s == AceRoute::F4)      // (few tasks per CU -- single images -- : the gather kernel)
        return (opt.wino4_force || opt.batch_inv || wino4_pays((long long)B * (r / 32) * (r / 32) * ((a.C + 15) / 16), num_cus)) ? s : AceRoute::WinoQuads;
    if (s == AceRoute::Sparse && opt.use_sh16) {      // tile-skip mode: honoured by the wave-specialised kernel only (conv_sh16.h)
        ConvParams t{};
        t.C = a.C;
        t.W = t.H = r;
        t.B = B;
        t.Cin = HID;
        t.dbg = opt.dbg;
        return sh16_ace_uses_ws(t) ? s : AceRoute::Dense;
    }
    if (s == AceRoute::Dense && !opt.use_sh16 && gb_small && !opt.batch_inv) {      // tiny levels at small batches (Runner::ace_tiny)
        const int rowsP = ((a.C + 31) / 32) * 64;
        const long long tiles = ((long long)B * r * r + 255) / 256;
        if (((rowsP + 127) / 128) * tiles < 128 && (long long)rowsP * B * r * r <= gb_small_cap) return AceRoute::TinySplitK;
    }
    return s;
}
SeanModel::ChunkMode SeanModel::chunk_mode(int B, int S) const {
    ChunkMode c;
    const bool large = (long long)B * S * S > ahead_limit;
    c.project_all = fcmu_batched && !opt.use_sh16 && (B * LABEL_NC > 64 || opt.batch_inv);
    c.grouped = c.project_all && lut_groups && lut_ngroups > 0;
    // interactive-size jobs: everything that depends on labels / codes only runs ahead on the side stream
    const bool side_ok = side && !prof_on && !(opt.dbg & DBG_NO_SIDE_STREAM);
    c.prepass = side_ok && overlap_on && large && c.grouped;      // large job on an overlap handle
    c.overlap = c.prepass && gtab_side;
    if (c.prepass || (side_ok && ahead_full && !large)) c.ahead = ChunkMode::FULL;
    else if (side_ok && (fcmu_batched || !opt.use_sh16) && !(opt.dbg & DBG_NO_LUT_AHEAD) && !c.grouped) c.ahead = ChunkMode::LUTS;
    c.prologue = pro_on && !prof_on && c.ahead != ChunkMode::FULL && large;
    return c;
}

}  // namespace chk
