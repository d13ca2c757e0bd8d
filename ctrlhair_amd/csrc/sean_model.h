// sean_model.h -- host side of the SEAN generator path: weight folding/packing at load, workspace arena,
// and the launch sequence of one batched forward.  No torch types; plain HIP runtime.
// Plain convs (ResBlock convs, 1x1 shortcut, Zencoder) are net_common.h ConvLayers, routed by conv_route and launched by run_conv
// with SeanModel::conv_env(); the ACEs have their own routes (AceRoute).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <string>
#include <vector>

#include "ace_sparse.h"
#include "net_common.h"

namespace chk {
struct AceW {
    std::string name;
    int C = 0, res_div = 1, index = 0;
    bool styled = false;
    float* spade_wpk = nullptr;                 // (gamma|beta) 64-row tiles, K = 128*9
    float *bias_g = nullptr, *bias_b = nullptr; // blended biases
    float *bn_a = nullptr, *bn_d = nullptr, *nv = nullptr;
    float *actv_table = nullptr, *actv_bias = nullptr;   // mlp_shared as label LUT [19*9][128]
    float *fcmu_w = nullptr, *fcmu_b = nullptr;          // [19][512][512], [19][512]
    float* lut_wpk = nullptr;                   // rows (tap, gamma|beta, c) x K=512
    float* lut_rows = nullptr;                  // same rows, plain [18C][512] (GEMV path for batches <= 3)
    float* lut_wt = nullptr;                    // the same matrix transposed, [512][18C]: the "image" of the grouped LUT build (exact f32)
    float *spade_wscale = nullptr, *lut_wscale = nullptr;   // f16x3 path: per-row 2^-k of the packed rows (sh16.h)
    float out_scale = 8.f;                      // f16x3 path: first-pass SH16 scale of this ACE's output (SH16_ACT_SCALE; the
                                                //   shortcut's ace_s carries the 2^D aligning conv_s with conv_1, sean_model.cpp)
    float actv_scale = 1.f;                     // f16x3 path: SH16 scale of the SPADE hidden activations (from a table bound)
    float* spade_wino = nullptr;                // exact-f32 Winograd path: pack_wino_A image of the (gamma | beta) rows, 16-channel row tiles
    float* edge_tab = nullptr;                  // sean.edge: E[3040][gamma|beta][C] of the straight-edge and frame pixels (ace_sparse.h), ACEs with res_div <= 4
    float* spade_wino4 = nullptr;               // sean.wino = 2: the same rows as an F(4x4,3x3) image (conv_wino4.h wino4_ace_row), levels <= wino4_ace_max_r
    float* gconst = nullptr;                    // [19][gamma|beta][C]: SPADE gamma/beta of a pixel whose 5x5 label neighbourhood
                                                //   is uniformly j (blend factor folded in, biases not) -- ace_sparse.h
};

struct BlockW {
    std::string name;
    int fin = 0, fout = 0, fmid = 0, res_div = 1;
    bool up_before = false, styled = false, learned = false;
    ConvLayer conv_0, conv_1, conv_s;          // (f16x3 handles: sh_wpk / sh_wscale, like every ConvLayer; exact-f32 handles: wpk and the Winograd / GEMM images)
    AceW ace_0, ace_1, ace_s;
};

struct ProfRec {
    hipEvent_t e0, e1;
    int kind;       // 0 plain conv, 1 ACE conv, 2 LUT gemm, 3 interior pass of a sparse ACE (table build + elementwise kernel)
    double flops, bytes;            // flops: the dense evaluation of the layer (every pixel through the conv)
    double flops_exec = -1.0;       // FLOPs the matrix cores ran when they differ from `flops` (Winograd convs: 16 / 36); < 0: = flops
    const int* sp_stat = nullptr;   // sparse ACE launch: snapshot of the statistics of its work list (read back at ch_profile_read)
    double sp_flops_unit = 0.0;     //   executed FLOPs = sp_stat[3] * sp_flops_unit
    double sp_bytes_px = 0.0, sp_bytes_fixed = 0.0, sp_npix = 0.0;   // algorithmic bytes = fixed + per-pixel x (boundary pixels
                                    //   sp_stat[1] for kind 1, interior pixels sp_npix - sp_stat[1] for kind 3)
};

// The three ACEs of a block are visited in launch order (shortcut, ace_0, ace_1); blocks with an identity shortcut have no ace_s.
// `blocks` may be const or not: fn receives const AceW& / AceW& accordingly.
template <class Blocks, class F>
void for_each_ace(Blocks& blocks, F fn) {
    for (auto& b : blocks)
        for (auto* a : {b.learned ? &b.ace_s : nullptr, &b.ace_0, &b.ace_1})
            if (a) fn(*a);
}
// index of a resolution level: log2(res_div) (res_div 1, 2, ..., 32 -> 0 ... 5)
inline int level_of(int res_div) {
    int k = 0;
    while ((1 << k) < res_div) ++k;
    return k;
}

enum class AceRoute {      // the route of one ACE (SeanModel::ace_route): decided once per chunk (sean_model.cpp AcePlan), read everywhere else
    F4,          // SPADE conv as F(4x4,3x3) over every tile of a low-resolution level (conv_wino4.h)
    WinoQuads,   // F(2x2,3x3) over the boundary quads, gather or tile mode (conv_wino.h), interior pixels from tables (ace_sparse.h)
    Sparse,      // direct conv over the boundary pixels: exact-f32 compacted kernel / f16x3 wave-specialised kernel
    TinySplitK,  // exact f32, tiny levels at small batches: plain split-K conv into gb_small + ace_finish_f32
    Dense        // every pixel through the fused ACE conv
};

// Everything ch_set_option writes (ch_api.cpp holds the table of keys).  build() and the forward passes only read these.
struct SeanOptions {
    bool use_sh16 = false;     // generator convs on the f16x3 split-operand MFMA path (conv_sh16.h)
    int terms = 3;             // f16 MFMA path: 3 = split operands (f32-class), 1 = f16 operands (BASELINE configs[4] class)
    int wino = 2;                              // option "sean.wino": exact-f32 path, 3x3 convs as Winograd on the f32 matrix cores:
                                               //   1 = F(2x2,3x3) everywhere (conv_wino.h); 2 = the ResBlock convs from 32 x 32 pixels as
                                               //   F(4x4,3x3) (conv_wino4.h), the rest F(2x2,3x3); 0 = direct evaluation (conv_mfma.h)
    int lut_grouped = 1;                       // option "sean.lut_grouped": exact-f32 path, style LUTs of all styled ACEs from one grouped GEMM launch
    int pw_wide = 1;                           // option "sean.pw_wide": exact-f32 path, 1 = 64-row wave tiles of the 1x1 GEMM kernel where its launcher takes them
                                               // (conv_pw.h pw_wide_rule; the grouped style-LUT launch when every group has 18 C % 256 == 0), the transposed wave
                                               // reduction of fc_mu and the one-thread-per-(row, label) F(4x4) style pack; 0 = the kernels of round 11.  Same bits.
    int prologue = 1;                          // option "sean.prologue": exact-f32 Winograd path, handles beyond the run-ahead sizes: what the ACEs build from
                                               //   labels, codes and weights alone comes from a few grouped launches at the start of a chunk, into per-ACE
                                               //   buffers (SeanModel::pro_on); 0 = every ACE launches its own, inline
    int label_memo = 1;                        // option "sean.label_memo": handles with the ACE prologue, calls of one chunk: 1 = the label-only products of a chunk
                                               //   (SeanModel::memo_state) are kept on the device and their launches return at once while the calls bring
                                               //   the same label maps; 0 = every call rebuilds them (launch for launch as without the memo)
    int spade_memo = 1;                        // option "sean.spade_memo": with the label memo, the styled ACEs on the F(4x4) V route: 1 = the 36 accumulators of a task
                                               //   after its 32 hidden k-steps are kept (SeanModel::memo_acc) and a call with the same maps runs the six style
                                               //   k-steps only; 0 = launch for launch as without it
    int code_memo = 1;                         // option "sean.code_memo": handles with the grouped style-LUT launch, calls of one chunk: 1 = the projections and
                                               //   the style LUTs (mu_all, lut_ahead) are kept and fc_mu_batched and the grouped GEMM return at once while the
                                               //   calls bring the same style codes (SeanModel::code_state); 0 = every call rebuilds them
    // Overlap mode (round 5; option "sean.overlap" = CUs of the side streams, 0 = off; exact-f32 Winograd path, jobs beyond the
    // run-ahead sizes): the HBM-bound kernels -- label tables of all ACEs, interior passes -- run on streams whose CU mask holds
    // `overlap` CUs (hipExtStreamCreateWithCUMask: every XCD gives overlap / 8 of its CUs), beside the matrix-bound convs on the
    // internal main stream, which claim their tasks dynamically (conv_wino.h) and so lose only the CUs, not the time, the side
    // kernels hold.  CU-masked streams are blocking streams (they synchronise with the NULL stream), so the whole generate() runs
    // on `main_i`, forked from and joined to the caller's stream by events.
    int overlap = 0;                           // (measured, DESIGN.md section 7: the side kernels are CU-bound, not HBM-bound, once confined -- no gain; default off)
    int wino4_force = 0;                       // option "sean.wino4_force": 1 = F(4x4,3x3) wherever the shape allows, whatever the task count (tests)
    int patch = 1;                             // option "sean.patch": 0 = the gather kernel always fetches from the hidden planes
    int convt_gemm = 1;                        // option "sean.convt_gemm": the Zencoder's ConvTranspose as four phase GEMMs (SeanModel::z10_pw), 0 = four Winograd phase convs
    int edge = 1;                              // option "sean.edge": 1 = straight-edge pixels of the levels >= 128 pixels are modulated by the interior pass from
                                               //   per-code table rows instead of going through the boundary conv (exact-f32 Winograd path, f16 paths in compaction mode; ace_sparse.h)
    int frame = 1;                             // option "sean.frame": 1 = with sean.edge on the exact-f32 Winograd path, the pixels of the two outermost rings of a level
                                               //   >= 128 pixels whose in-image 5x5 window is uniform are served the same way (frame codes, ace_sparse.h); 0 = boundary conv
    int int_groups = 0;                        // option "sean.int_groups": channel groups of 32 per block of the four-pixel interior kernel (levels >= 128 pixels,
                                               //   exact-f32 Winograd path): 0 = chosen per launch (ace_interior_groups), n >= 1 = at most n (1 = one group per block)
    int int_onepass = 1;                       // option "sean.int_onepass": 1 = a block of the four-pixel interior kernel hashes its straight-edge codes into 128 slots
                                               //   and, holding more than 64, serves them in one round with steps of 16 channels (bit-identical results); 0 = 64
                                               //   slots and a second round beyond them
    int batch_inv = 0;                         // option "sean.batch_invariant": 1 = every choice that follows the number of tasks of a call (F(4x4) vs F(2x2),
                                               //   split-K, sample-pair tiles at 16 pixels, the small-batch LUT / tiny-level routes) is made as for a large
                                               //   batch: sample i alone == sample i in any batch, bit for bit (exact-f32 path)
    int wino4v = 1;                            // option "sean.wino4v": 1 = F(4x4,3x3) layers with >= 512 GEMM rows at <= 64 pixels (and the Zencoder's 256 -> 512
                                               //   conv) take their input pre-transformed by one extra pass (conv_wino4v.h; bit-identical results)
    int wino4_split = -1;                      // option "sean.wino4_split": the plain F(4x4,3x3) convs that do not take the V route on wino4_plain_split_kernel
                                               //   (conv_wino4_split.h; bit-identical results): 0 = never, 1 = every one, -1 = where wino4_split_pays says so.
                                               //   Second weight images: -1: layers below 512 GEMM rows (the others take the V route), 1: every F(4x4,3x3) layer
    int wino4_ace_max_r = 64;                  // option "sean.wino4_ace": largest level whose SPADE convs run as F(4x4,3x3) over EVERY tile (0 = none)
    int hidden_wq = 1;                         // option "sean.hidden_wq": Winograd ACE path from 128 pixels, SPADE hidden activations + one-hot planes
                                               //   from one persistent kernel, only where a boundary quad's patch reads them (0: every pixel, two kernels)
    int wino_gather = 1;                       // option "sean.wino_gather": 1 = gather mode of the Winograd ACE kernel (default), 0 = tile mode
    int wino_th = 0;                           // option "sean.wino_th": tile height 16 / 32 of the Winograd ACE kernel (0 = by level)
    // measured per level at B = 16, 512^2 on the benchmark labels (ms for the level's three ACEs, tiles of 32 x 16 / 32 x 32):
    // 512^2 13.8 / 9.6, 256^2 8.1 / 9.6, 128^2 7.9 / 7.1, 64^2 4.1 / 4.8
    int wino_tile_h(int r) const { return (wino_th == 16 || wino_th == 32) ? (r % wino_th ? 16 : wino_th) : ((r >= 512 || r == 128) ? 32 : 16); }
    int sparse = 1;                            // option "sean.sparse" (0 = every pixel through the conv)
    int sh16_compact = 1;                      // option "sean.sh16_compact": f16x3 path, 1 = pixel-level compaction inside the
                                               //   wave-specialised ACE kernel (3-term path) with pair / quad entries for
                                               //   sparse tiles, 2 = without those entries (A/B), 0 = tile skipping only
    int sparse_th = 0;                         // option "sean.sparse_th": tile height 8 / 16 (0 = by the layer's row tiles)
    // Taller tiles where a tile of 32 x 8 carries few sub-tiles: few row tiles (C <= 64: the four waves of a block split the
    // sub-tiles), and the full-resolution level of large images (measured at 512^2, B = 16: 5.26 vs 5.64 ms per C = 128 ACE;
    // at 256^2 and below the 32 x 8 tiles are faster: 5.44 vs 5.62, 4.13 vs 4.27, 2.69 vs 2.80 ms)
    int sparse_tile_h(int mtiles, int r) const {
        return sparse_th == 8 || sparse_th == 16 ? sparse_th : ((mtiles <= 2 || r >= 512) ? 16 : 8);
    }
    int sparse_min_r = 64;                     // option "sean.sparse_min": smallest resolution served by the sparse path
    long long ahead_pixels = -1;               // option "sean.ahead": largest B*S*S served in run-ahead mode (-1: default 2 x 512^2; build() resolves it
                                               //   into SeanModel::ahead_limit)
    int dbg = 0;               // perf experiments: bits of chk::Dbg (dbg_bits.h)
    int dbg_sel = 16;          // DBG_STAMP: index of the ACE launch whose tiles are cycle-stamped
};

struct SeanModel {
    SeanOptions opt;
    int ngf = 0, max_batch = 0, max_size = 0;
    int num_cus = 256;                         // compute units of the handle's device (build())
    std::vector<void*> allocs;                         // everything to hipFree

    // ---- weights ----
    std::vector<BlockW> blocks;
    int n_aces = 0;
    float *fc_table = nullptr, *fc_bias = nullptr;     // fc conv as label LUT [19*9][16ngf]
    float *img_w = nullptr, *img_b = nullptr;          // conv_img raw [3][ngf][3][3]
    float* img_w4 = nullptr;                           // the same, [ngf/4][tap][co][4] (conv_img_c4_kernel's scalar loads)
    bool has_zencoder = false;
    float* z1_w = nullptr;                             // Zencoder stem weights, unpacked (direct VALU conv)
    // architecture.py:158-176.  Each layer carries the images of every route it can take: z10 (the ConvTranspose as a 3x3 conv over the zero-inserted view)
    // direct + f16x3; z14 direct, F(2x2), F(4x4) (sean.wino = 2), its split order (sean.wino4_split = 1) + f16x3
    ConvLayer z1, z4, z7, z10, z14;
    ConvLayer z4_s2d, z7_s2d;                          // the two stride-2 convs in the space-to-depth form (conv_sh16.h S2D)
    // the forms of the ConvTranspose that are different convs (bias: z10's):
    ConvLayer z10_wino;                                // exact f32: four Winograd phase convs of the input grid (1024 rows = 4 co + phase, depth-to-space store)
    ConvLayer z10_d2s;                                 // f16x3: 2x2 taps at the input resolution, depth-to-space store (1024 rows = phase * 256 + co)
    ConvLayer z10_pw[4];                               // option "sean.convt_gemm": four phase GEMMs over shifted views (conv_pw.h; phase = 2 py + px)

    // ---- workspace ----
    float* gb_small = nullptr;                  // exact-f32 path: gamma | beta sums of a tiny ACE level whose SPADE conv runs as a plain split-K conv (ace())
    long long gb_small_cap = 0;
    float* splitk_ws = nullptr;
    long long splitk_cap = 0;
    unsigned* amax_slots = nullptr;            // f16x3 path: recorded maxima of the dynamically scaled SH16 tensors (sh16.h)
    float* zero_page = nullptr;                // 256 bytes of zeros
    float *noise_ws = nullptr, *mu_img = nullptr, *lut = nullptr, *actv = nullptr;
    // f16x3 path, batches above the GEMV threshold: the style projections of ALL styled ACEs come from one launch
    // (fc_mu_batched) into per-ACE images mu_all + index * mu_stride; device arrays of the per-ACE weight / bias pointers
    bool fcmu_batched = false;
    float* mu_all = nullptr;
    long long mu_stride = 0;
    const float** fcmu_w_ptrs = nullptr;
    const float** fcmu_b_ptrs = nullptr;
    float *h0 = nullptr, *hs = nullptr, *dx = nullptr, *h1 = nullptr, *xs = nullptr, *xa = nullptr, *xb = nullptr;
    int enc_pending_B = 0, enc_pending_S = 0;   // split encode: set by phase 1, consumed by phase 2

    // ---- run-ahead / overlap ----
    // run-ahead mode of interactive-size jobs: label / style-only kernels of every ACE on a side stream (sean_model.cpp)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_join;
    std::vector<float*> actv_ahead, lut_ahead;
    // exact-f32 path, more than 64 (sample, label) columns: the style LUTs of all styled ACEs from ONE grouped GEMM launch at the
    // start of a chunk (conv_pw.h: operands swapped -- the projected codes are the A operand, packed by fc_mu_batched) into lut_ahead
    void* lut_groups = nullptr;                 // device array of PwGroup
    bool lut_groups_wide = false;               // every group of lut_groups has 18 C % 256 == 0: the grouped launch may take the wide tiles (sean.pw_wide)
    int lut_ngroups = 0, lut_group_tiles = 0;   // total pixel tiles (tasks = tiles x row groups of the call's batch)
    double lut_group_rows = 0.0;                // sum of 18 C over the groups (profiling figures)
    bool ahead_full = false;                   // handle sized for the full run-ahead mode (else: style LUTs only)
    long long ahead_limit = 0;                 // largest B*S*S served in run-ahead mode: opt.ahead_pixels resolved by build() (default; 1 where overlap mode
                                               //   needs the per-ACE buffers of a handle whose run-ahead mode is off); 0 = never
    float* splitk_side = nullptr;
    bool overlap_on = false;                   // streams / buffers of the overlap mode (SeanOptions::overlap) exist (build())
    hipStream_t main_i = nullptr, side_int = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    std::vector<hipEvent_t> ev_x, ev_int;      // per ACE: its input is ready (main -> side_int), its interior pass is done (side_int -> main)
    unsigned* claim_pool = nullptr;            // dynamic task claiming: CLAIM_SLOTS launches x CLAIM_WORDS words (8 counters + mailboxes), zeroed per chunk
    static constexpr int CLAIM_SLOTS = 96, CLAIM_WORDS = 1024;

    // ---- levels ----
    // Winograd ACE path (conv_wino.h wino_ace_kernel): per resolution level the boundary quads of every 32 x 16 tile and one task
    // list per distinct row-tile count; per-sample style images of the ACE being run
    struct WinoWork { int nrt = 0; unsigned* work = nullptr; int* total = nullptr; };
    struct WinoLevel {
        uint8_t* qlist = nullptr; int* qcnt = nullptr; int* pcnt = nullptr; int cap_tiles = 0, TH = 16; std::vector<WinoWork> works;
        // gather mode (conv_wino.h): one list of boundary quads per sample, tasks of 64 consecutive entries
        unsigned* gq = nullptr; int* gq_n = nullptr; int* qoff = nullptr; int gq_cap = 0;
        int* chunk_base = nullptr;        // [33] first chunk of 64 quads of every sample (patch source of the gather kernel, conv_wino.h)
        int* patch_mode = nullptr;        // device flag: 1 = this chunk's patches come pre-gathered from SeanModel::patchbuf
    };
    // One resolution level (index = log2(res_div)): the facts build() fixes for every ACE of the level -- it returns an error if they disagree --
    // and the buffers the level's ACEs share.  The Runner's per-chunk LevelPlan (sean_model.cpp) decides what a call launches on them.
    struct Level {
        int r = 0;                                 // the level's size at max_size
        bool used = false, styled = false, edge_tab = false;      // an ACE runs here; its ACEs are styled; ... carry AceW::edge_tab
        uint8_t* lab = nullptr;                    // down-sampled label map (levels 1-5; level 0 reads the caller's)
        WinoLevel wq;                              // Winograd ACE routes: quad lists and one task list per distinct row-tile count (16-channel tiles)
        float* actv = nullptr;                     // ... hidden activations in the padded layout (conv_wino.h WINO_AXOFF)
        // exact SPADE-interior reduction (ace_sparse.h): classification buffers and one work list per distinct number of 64-row tiles
        SparseLevel sp[2];                         // [0: tiles of 32 x 8 | 1: tiles of 32 x 16]
        std::vector<SparseWork> sp_work;
    };
    Level levels[6];
    // The one statement of "the classification of level k carries straight-edge marks (u5 == 253 + e16) and frame marks": r = the level's size,
    // ti = the SparseLevel classified.  built = true: a call asks (r of the call; the buffers and the level's route are part of the answer).
    // built = false: build() asks what to allocate (e16: r of max_size; edge_tab: r at NOMINAL_SIZE; p6: level 0 at NOMINAL_SIZE) -- options and size only.
    struct LevelMarks { bool edges = false, frame = false; };
    static constexpr int NOMINAL_SIZE = 512;
    LevelMarks level_marks(int k, int r, int ti, bool built = true) const;
    std::map<const float*, long long> pad_state;   // geometry (size, planes) a padded buffer's zero columns were last cleared for
    float* patchbuf = nullptr;                 // pre-gathered hidden-activation patches of the ACE being run (few, scattered boundary quads)
    int patch_cap_chunks = 0;
    float* wsty = nullptr;
    float* wsty4 = nullptr;                    // per-sample F(4x4,3x3) style images of the ACE being run (conv_wino4.h)
    size_t wsty4_floats = 0;                   // its size; pad_state[wsty4] == 1: zeroed since it was allocated (wino4_style_pack, rows = 1)
    float* vbuf = nullptr;                     // the pre-transformed input V of the layer being run (conv_wino4v.h)
    size_t vbuf_bytes = 0;
    // the V route of an ACE's F(4x4,3x3) conv (net_common.h wino4v_plan; padded: the hidden planes of an ACE level; the plain convs: conv_route)
    bool wino4v_route(bool pays, const float* in, int Bn, int r, int K, int nks, Wino4vPackParams& vp, bool padded = false) const {
        return wino4v_plan(opt.wino4v && pays, vbuf, vbuf_bytes, in, Bn, r, r, K, nks, vp, padded);
    }
    // what the plain-conv routes read of this handle (net_common.h conv_route / run_conv); the caller adds the call's epilogue, split-K scratch and claim slot
    ConvOpts conv_env() const;
    const WinoWork* wino_work(const AceW& a, int r) const;        // task list of the ACE's row tiles on its Winograd level; nullptr: no Winograd route at r
    const SparseWork* sparse_work(const AceW& a, int r) const;    // work list of the ACE's row tiles on its sparse level; nullptr: not served at r
    AceRoute ace_route_shape(const AceW& a, int r) const;         // from shape, weights and options: F4 / WinoQuads / Sparse / Dense (build() sizes buffers by it)
    AceRoute ace_route(const AceW& a, int r, int B) const;        // ... and the task count of the call: F4 may fall to WinoQuads, f16x3 Sparse to Dense, Dense to TinySplitK
    // How one chunk of B samples at S pixels runs on this handle (decided once, by chunk_mode; generate() and the Runner read it)
    struct ChunkMode {
        bool project_all = false, grouped = false;      // exact f32, more than 64 (sample, label) columns: the style projections of every styled ACE from one launch; ... feeding ONE grouped LUT GEMM
        enum Ahead { NONE, LUTS, FULL } ahead = NONE;      // run-ahead on the side stream: nothing / the style LUT builds / LUTs and label tables
        bool prepass = false, overlap = false;      // overlap handle, large chunk: level geometry up front, label tables ahead on the CU-masked side stream; ... and interior passes on side_int
        bool prologue = false;         // grouped launches of the label / code-only products ahead of the first conv (Runner::prologue)
    };
    ChunkMode chunk_mode(int B, int S) const;
    // ACE prologue (option "sean.prologue", Runner::prologue): per-ACE destinations of the grouped launches, sized by the route the ACE takes at
    // (max_batch, max_size), SeanModel::ace_route_shape -- F(4x4) route (32 / 64 pixels): its own padded hidden planes; gather route (128 pixels and more): its own gamma / beta
    // table, column / row sums and F(2x2) style images.  nullptr: the ACE keeps its inline launches and the shared buffers above.
    bool pro_on = false;
    std::vector<float*> pro_actv, pro_gtab, pro_p6, pro_wsty;
    size_t pro_bytes = 0;                      // what these buffers add to the handle
    // Label memo (option "sean.label_memo"; handles with pro_on): sliders, sweeps and direction searches render one mask with many codes, call
    // after call, so what a chunk builds from labels and weights alone -- level label maps, classification, level geometry, the hidden planes of
    // the F(4x4)-route ACEs, the pre-gathered patches of the gather-route ACEs -- is still in place when the next call brings the same maps.
    // The device decides (kernels.h label_memo_begin): `memo_lab` is the handle's copy of the last eligible chunk's maps, `memo_state` the words
    // MEMO_*; a memoized kernel reads memo_state[MEMO_HIT] at its top and returns on 1.  The host never learns the answer and enqueues the same
    // launches either way (eager or in a captured graph).  Eligible: the only chunk of a call, in prologue mode, whose level geometry fits the
    // grouped launches (Runner::memo_begin); any other chunk clears MEMO_VALID in stream order.  A memoized kernel reads labels and memoized
    // products only, and writes buffers nothing else writes: the level buffers, pro_actv and `memo_patch` (one patch buffer per styled
    // gather-route ACE in place of the shared patchbuf).  `memo_epoch` is part of the key: ch_set_option bumps it.
    uint8_t* memo_lab = nullptr;
    int* memo_state = nullptr;
    int memo_epoch = 0;
    bool memo_dirty = false;                   // a generate() ended in an error after its decision kernel: the next eligible chunk invalidates first
    std::vector<float*> memo_patch;
    // unstyled gather-route ACEs (up_3): gamma and beta of the boundary quads are label-only too.  In patch mode the conv launch stores them per
    // task (conv_wino.h WinoAceParams::cache); on a hit it returns at once and wino_ace_cached_kernel modulates from the stored values.
    std::vector<float*> memo_gb;
    std::vector<int> memo_gb_cap;              // tasks each holds
    size_t memo_bytes = 0;                     // what the memo adds to the handle
    std::string label_memo_stats(int* calls, int* hits);      // synchronous read-back of MEMO_CALLS / MEMO_HITS (tests and tools)
    // SPADE memo (option "sean.spade_memo", conv_wino4v.h): the SPADE conv of a styled ACE contracts 128 hidden channels (labels and weights
    // only) and then 20 one-hot planes with the style images of the sample (the codes).  `memo_acc` keeps, per ACE that takes the F(4x4) V
    // route with style images at (max_batch, max_size), the raw accumulators of every task after the hidden k-steps; `memo_v1h` the V image
    // of the one-hot planes per level size (32 / 64 pixels; the same for every ACE of a level).  The decision kernel sets MEMO_SPADE_MODE
    // per call: PLAIN on a label miss, STORE on the first hit of a label set, LOAD from the second on.  Each of these ACEs enqueues the
    // plain kernel and the memo instantiation, one of which returns at once; whatever clears MEMO_VALID clears MEMO_ACC_VALID.
    std::vector<float*> memo_acc;
    std::vector<long long> memo_acc_tasks;     // tasks each holds
    float* memo_v1h[2] = {nullptr, nullptr};
    bool spade_memo_on = false;                // any memo_acc allocated: the decision kernel keeps the mode
    std::string spade_memo_stats(int* stores, int* loads);     // synchronous read-back of MEMO_STORES / MEMO_LOADS
    // Code memo (option "sean.code_memo"; handles with lut_groups): a shape-slider drag, a mask warp or a shape sweep changes the label maps
    // and keeps every style code; a repeat render keeps both.  fc_mu_batched and the grouped LUT GEMM read codes and weights only and write
    // buffers that nothing else writes on such a chunk and that outlive the call (mu_all, lut_ahead), so a chunk that brings the codes of the
    // previous one skips both.  The device decides, as for the label memo and independent of it (kernels.h code_memo_begin): `code_copy` is
    // the handle's copy of the last eligible chunk's codes, `code_state` the words CODE_*; the two launches read code_state[CODE_HIT] at
    // their top and return on 1.  Eligible: the only chunk of its call, with mode.project_all && mode.grouped, profiling off and codes that
    // can be read in 16-byte words.  Any other chunk clears CODE_VALID in stream order: the GEMV branch of Runner::build_lut and the run-ahead LUT builds
    // (lut_src == AHEAD) write lut_ahead, the f16x3 and the ungrouped projections write mu_all in another layout.  encode() touches neither.
    // The key is (B, memo_epoch).  Left out: ace_tables_grouped and wino_style_pack_grouped (80 us; their member set follows the plan of the
    // call, not the codes alone) and the wino4_style_pack launches (they write the shared wsty4).
    float* code_copy = nullptr;
    int* code_state = nullptr;
    bool code_dirty = false;                   // a generate() ended in an error after its decision kernel: the next eligible chunk invalidates first
    size_t code_bytes = 0;                     // what the code memo adds to the handle
    std::string code_memo_stats(int* calls, int* hits);        // synchronous read-back of CODE_CALLS / CODE_HITS

    // ---- exact SPADE-interior reduction (ace_sparse.h; per-level buffers: Level) ----
    float* gtab = nullptr;                     // [max_batch][19][2][C max]
    float* gtab_side = nullptr;                // overlap mode: the table of the interior passes on the side stream
    float* p6 = nullptr;                       // per-call column / row sums of the style LUT of the ACE being run: [mb][19][6][2][C]

    // ---- profiling ----
    bool prof_on = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> ev_pool;
    int* prof_stats = nullptr;                 // profiling: snapshots of the work-list statistics of sparse launches (16 B each)
    int prof_stats_cap = 0, prof_stats_used = 0;
    std::map<std::string, float*> taps;

    size_t noise_floats(int S) const;
    // returns empty string on success, else error message; reads `opt`, never writes it
    std::string build(const TensorStore& ts, int max_batch, int max_size);
    std::string generate(const uint8_t* labels, const float* codes, const float* noise, uint64_t seed, float* out,
                         int B, int S, hipStream_t stream);
    // the planes generate() draws on device when it is given noise == nullptr, written out explicitly
    std::string draw_noise(uint64_t seed, float* out, int B, int S, hipStream_t stream);
    // Zencoder (style encoder + region average pooling), architecture.py:177-207
    std::string encode(const float* img, const uint8_t* labels, float* codes_out, int B, int S, hipStream_t stream, int phase = 0);
    void destroy();
};

}  // namespace chk
