// kernels.h -- launchers of the non-MFMA kernels (sean_kernels.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <utility>
#include <vector>

namespace chk {
// memo_hit (here and below; optional): device word of the label memo (SeanModel::memo_state); the kernel returns at once where it reads 1
hipError_t label_downsample(const uint8_t* in, uint8_t* out, int B, int S, int r, hipStream_t s, const int* memo_hit = nullptr);
// Label memo: the words of its device state, and the two launches at the start of an eligible chunk (compare `bytes` of labels with the
// copy, 16-byte aligned both; then decide MEMO_HIT from MEMO_VALID, MEMO_DIFF and the key (B, S, epoch)) / of any other chunk (MEMO_VALID = 0)
// SPADE memo (conv_wino4v.h, the memo instantiation): MEMO_ACC_VALID = the accumulator caches of the F(4x4)-route ACEs hold the sums of these
// labels; MEMO_SPADE_MODE = what this call's launches do with them.  spade = 0: the mode stays PLAIN and the caches invalid.  Store on the
// SECOND sight of a label set: no hit -> PLAIN, valid = 0; hit with valid = 0 -> STORE, valid = 1; hit with valid = 1 -> LOAD.
enum { MEMO_VALID = 0, MEMO_DIFF = 1, MEMO_HIT = 2, MEMO_KEY = 3, MEMO_CALLS = 6, MEMO_HITS = 7, MEMO_ACC_VALID = 8, MEMO_SPADE_MODE = 9, MEMO_STORES = 10,
       MEMO_LOADS = 11, MEMO_WORDS = 12 };
enum { SPADE_PLAIN = 0, SPADE_STORE = 1, SPADE_LOAD = 2 };
hipError_t label_memo_begin(const uint8_t* labels, uint8_t* copy, long long bytes, int* state, int B, int S, int epoch, hipStream_t s, int spade = 0);
hipError_t label_memo_invalidate(int* state, hipStream_t s);
// Code memo (SeanModel::code_state): the same two launches over the style codes of an eligible chunk, with words of their own -- compare `bytes`
// of codes with the copy as integer words (16-byte aligned both), then decide CODE_HIT from CODE_VALID, CODE_DIFF and the key (B, epoch)
enum { CODE_VALID = 0, CODE_DIFF = 1, CODE_HIT = 2, CODE_KEY = 3, CODE_CALLS = 6, CODE_HITS = 7, CODE_WORDS = 8 };
hipError_t code_memo_begin(const float* codes, float* copy, long long bytes, int* state, int B, int epoch, hipStream_t s);
hipError_t code_memo_invalidate(int* state, hipStream_t s);
// need (optional, [B][H][W]): pixels with need == 0 are not written (ace_sparse.h: nothing reads them)
hipError_t onehot_conv3x3(const uint8_t* lab, const float* table, const float* bias, float* out, int B, int H, int W,
                          int K, int relu, hipStream_t s, int c4 = 0, const uint8_t* need = nullptr, int kout = 0);
// kout > K (NCHW output only): the output tensor has kout channel planes per sample; the table channels fill the first K.
// label_onehot_planes writes planes k0 .. k0 + 19 of such a tensor: plane k0 + j = (label == j), plane k0 + 19 = 0 (the Winograd ACE
// kernel's style k-steps, conv_wino.h)
hipError_t label_onehot_planes(const uint8_t* lab, float* out, int B, int H, int W, int kout, int k0, hipStream_t s);
// Winograd ACE path: the SPADE hidden activations (K = 128 table channels, relu) + optionally the 20 one-hot planes behind them, written
// only at the pixels some boundary quad's 4 x 4 patch reads (u5: the interior map of ace_classify, 255 = boundary pixel; nullptr:
// every quad is a boundary quad).  out has kout planes per sample, each H rows of `pitch` floats with image column x at x + xoff
// (pitch = 0: plain [H][W] planes; xoff > 0: the padded layout of the Winograd ACE kernels, conv_wino.h WINO_AXOFF -- the columns
// left and right of the image must hold zeros, the kernel never writes them: the caller clears them).  Shapes: spade_hidden_wq_supported (H, W multiples of 32).
bool spade_hidden_wq_supported(int H, int W);
// Second half of an ACE whose SPADE gamma / beta conv ran as a PLAIN conv (tiny levels at small batches: sean_model.cpp ace()):
//   gb [B][rowsP][H*W] holds the raw conv sums in the row order of the direct kernels' packed image (wave tile of 64 rows = gamma rows |
//   beta rows of 32 channels); adds the blended biases and the style-LUT gathers (lut [B*19][9][2][C] or null), modulates
//   act((bn_a x + nv noise + bn_d)(1 + gamma) + beta) -- normalization.py:111-112,117-153,172-187; the arithmetic of ace_epilogue_f32.
hipError_t ace_finish_f32(const float* gb, int rowsP, const float* x, int x_up, const float* bias_g, const float* bias_b, const float* bn_a,
                          const float* bn_d, const float* nv, const float* noise, long long noise_bstride, const uint8_t* lab, const float* lut,
                          float* out, int B, int C, int H, int W, int act, hipStream_t s);
hipError_t spade_hidden_wq(const uint8_t* lab, const uint8_t* u5, const float* table, const float* bias, float* out, int B, int H, int W,
                           int kout, int onehot, hipStream_t s, int pitch = 0, int xoff = 0, const int* skip_if_patch = nullptr);
// ACE prologue (sean_model.cpp): the same pass for several ACEs in ONE launch.  The group travels by value as the kernel argument: it is
// filled per call (the label pointers, the level sizes and the set of ACEs follow the call's B and S), so no device copy of it can go stale.
// The caller fills lab .. xoff of each entry; the launcher fills tcs, start, nblk.
struct HiddenGroup {
    static constexpr int MAX = 24;
    struct Entry {
        const uint8_t* lab;
        const uint8_t* u5;
        const float* table;
        const float* bias;
        float* out;
        int H, W, kout, onehot, pitch, xoff;
        int tcs, start, nblk;
    };
    Entry e[MAX];
    int n, B;
    const int* memo_hit;      // optional (label memo): the whole launch returns at once where it reads 1
};
hipError_t spade_hidden_wq_grouped(HiddenGroup& g, hipStream_t s);
// the same activations as pre-gathered 4 x 4 patches of the boundary quads, chunk by chunk of 64 (conv_wino.h WinoAceParams::patch); both
// kernels read the device flag *mode (wino_chunk_base): exactly one of them does the work
hipError_t spade_hidden_patch(const uint8_t* lab, const unsigned* gq, const int* gq_n, int gq_cap, const int* chunk_base, const int* mode,
                              const float* table, const float* bias, float* patch, int B, int H, int W, int kout, hipStream_t s);
// spade_hidden_wq(..., skip_if_patch = mode) followed by spade_hidden_patch(..., mode) as ONE launch: each block reads the flag and runs the
// body of the kernel that would not have returned at once (chunks with the ACE prologue, sean_model.cpp)
hipError_t spade_hidden_level(const uint8_t* lab, const uint8_t* u5, const unsigned* gq, const int* gq_n, int gq_cap, const int* chunk_base, const int* mode,
                              const float* table, const float* bias, float* out, float* patch, int B, int H, int W, int kout, int onehot, int pitch,
                              int xoff, hipStream_t s, const int* memo_hit = nullptr);      // memo_hit: returns at once on 1 in patch mode (`patch` then is the caller's to keep)
hipError_t wino_chunk_base(const int* gq_n, int B, int cap_chunks, int* chunk_base, int* mode, hipStream_t s);
// `scale`: power-of-two scale of an SH16 output / input tensor (sh16.h)
hipError_t onehot_conv3x3_sh16(const uint8_t* lab, const float* table, const float* bias, void* out, int B, int H, int W,
                               int K, int relu, float scale, hipStream_t s, int bf16 = 0, const uint8_t* need = nullptr,
                               const int* tile_cnt = nullptr,    // tile_cnt: boundary pixels per tile of 32 x 16 (tile-skip mode)
                               int need_impl = 0);               // need-masked launches: 0 = compacting kernel at W >= 512,
                                                                 // 1 = never, 2 = always (A/B, tools/onehot_bench.hip)
// amax: device slot of a dynamically scaled tensor (sh16.h), null = static scale
hipError_t sh16_decode(const void* in, float* out, int B, int C, long long HW, float scale, const unsigned* amax,
                       hipStream_t s, int bf16 = 0, int single = 0);
hipError_t fc_mu(const float* codes, const float* Wt, const float* bias, float* mu_img, int B, int Npad, hipStream_t s,
                 float* mu_rows = nullptr, int sh16 = 0, int bs = 19, float scale = 1.f, unsigned* amax = nullptr,
                 int pass = 0, int bf16 = 0, int transposed = 1);      // transposed: the wave reduction as one transposed butterfly (same bits; 0 = 32 butterflies)
hipError_t fc_mu_batched(const float* codes, const float* const* Wts, const float* const* biases, float* mu_base,
                         long long mu_stride, int n_aces, int B, int Npad, int bs, float scale, unsigned* amax_slots, int pass,
                         int bf16, hipStream_t s, int sh16 = 1, int transposed = 1,
                         const int* skip = nullptr);      // skip (optional): device word of the code memo; the launch returns at once where it reads 1
// w4 (C4 path): the same weights packed [Cin/4][tap][co][4 channels] for scalar loads
hipError_t conv_img_tanh(const float* x, const float* w, const float* bias, float* out, int B, int Cin, int H, int W,
                         hipStream_t s, int c4 = 0, const float* w4 = nullptr);
hipError_t c4_decode(const float* in, float* out, int B, int C, long long HW, hipStream_t s);
hipError_t gen_noise(float* out, long long n, uint64_t seed, hipStream_t s);
// mfma_peak.hip: sustained MFMA-only rate of the device (kind 0: f32 32x32x2, 1: f16 32x32x16), ~ms_target ms, synchronises
hipError_t mfma_peak(int kind, int ms_target, double* tflops, hipStream_t s);
// misc_kernels.hip
// instance-norm outputs are bounded by sqrt(HW): their SH16 scale is instnorm_sh16_scale(HW), no saturation possible
float instnorm_sh16_scale(int HW);
// scratch (optional, >= 64 KiB of floats): enables the sliced two-kernel form for tensors with few (sample, 8-channel group)
// pairs and large planes, where one block per pair would leave most CUs idle
hipError_t instnorm_act(float* x, int planes, int HW, float eps, int act, hipStream_t s, void* sh16 = nullptr, int C = 0,
                        float* scratch = nullptr);
// ConvTranspose2d(k3, s2, p1, op1) as four phase GEMMs (misc_kernels.hip): the four shifted views of x [B][C][H][W] as xs [B][4][C][H][W]
// (shift order (0,1) | (0,0) | (1,0) | (1,1)); InstanceNorm + activation over the phase planes t [4][B][C][H][W] (+ bias), written
// depth-to-space into out [B][C][2H][2W]
hipError_t convt_shift4(const float* x, float* xs, int B, int C, int H, int W, hipStream_t s);
hipError_t instnorm_act_d2s(const float* t, const float* bias, float* out, int B, int C, int H, int W, float eps, int act, hipStream_t s);
hipError_t instnorm_c4_to_sh16(const float* x_c4, int B, int C, int HW, float eps, int act, void* sh16, hipStream_t s,
                               float* scratch = nullptr);
hipError_t layernorm_act(float* x, const float* gamma, const float* beta, float* part, int B, int C, int HW, float eps,
                         int act, hipStream_t s);
// LayerNorm + activation with layout conversion: in NCHW / C4 -> out SH16 (scaled) / NCHW f32 (shape decoder, f16x3 convs)
hipError_t layernorm_act_conv(const float* x, int in_c4, void* out, int out_sh16, float out_scale, const float* gamma,
                              const float* beta, float* part, int B, int C, int HW, float eps, int act, hipStream_t s);
hipError_t region_mean(const float* codes, const uint8_t* lab, float* out, int B, int F, int h, int w, int S,
                       hipStream_t s, int c4 = 0);
hipError_t maxpool3x3s2(const float* in, float* out, long long planes, int H, int W, hipStream_t s);
hipError_t global_avg_pool(const float* in, float* out, int planes, int HW, hipStream_t s);
hipError_t chan_affine(const float* in, const float* sc, float sc_add, const float* sh, const float* other, float* out,
                       long long planes, int HW, hipStream_t s);
hipError_t stem7x7(const float* in, const float* w, const float* bias, float* out, int B, int H, int W, hipStream_t s);
hipError_t conv3x3_c3_reflect(const float* in, const float* w, const float* bias, float* out, int B, int Cout, int H, int W,
                              hipStream_t s);
hipError_t bilinear_argmax(const float* lg, uint8_t* out, float* logits_out, const uint8_t* remap, int B, int h, int w,
                           int H, int W, hipStream_t s, int c4 = 0);
// C4-layout variants (f16x3 BiSeNet trunk); `amax`: device slot receiving max |out| * SH16_ACT_SCALE, or null
hipError_t maxpool3x3s2_c4(const float* in_nchw, float* out_c4, unsigned* amax, int B, int C, int H, int W, hipStream_t s);
hipError_t global_avg_pool_c4(const float* in, float* out, int B, int C, int HW, hipStream_t s);
hipError_t chan_affine_c4(const float* in, const float* sc, float sc_add, const float* sh, const float* other, float* out,
                          unsigned* amax, int B, int C, int HW, hipStream_t s);
hipError_t shape_softmax(const float* hair, const float* face, uint8_t* lab, float* probs, int B, int HW, hipStream_t s,
                         int c4 = 0);
hipError_t c4_rows_to_nchw(const float* in, float* out, int B, int C, int Cpad, int HW, hipStream_t s);
// layer 0 of both shape encoders from the label map: out = posconst + 16 table rows per pixel (misc_kernels.hip); either output may be null
hipError_t shape_enc_l0(const uint8_t* lab, const float* tab, const float* pc_hair, const float* pc_face, float* out_hair, float* out_face,
                        int B, int S, hipStream_t s);
hipError_t shape_inputs(const uint8_t* lab, const float* pos, float* hair_in, float* face_in, int B, int HW,
                        hipStream_t s);
hipError_t shape_inputs_sh16(const uint8_t* lab, const float* pos, void* hair_in, void* face_in, int B, int HW, float scale,
                             hipStream_t s);      // SH16, 48 / 64 channels
hipError_t linear(const float* x, const float* W, const float* bias, const float* scale, const float* shift, float* out,
                  int B, int K, int O, int ldx, int ldo, int act, hipStream_t s);
// out[n][rows] = W[rows][512] x[n][:]: the style LUT of one ACE for N <= 64 (sample, label) columns on the f32 matrix cores (misc_kernels.hip)
hipError_t lut_gemv_mfma(const float* x, const float* W, float* out, int N, int rows, hipStream_t s);
hipError_t subspace_add(float* h, const float* z, int zld, const float* U, const float* L, const float* mu, int B, int D,
                        int Z, hipStream_t s);
// poisson_kernels.hip: blending step after the generator (hair_editor.py:285-310, poisson_blending.py:29-87)
// Batched over B images of one size ([B,H,W,3] / [B,H,W]); ws holds B * poisson_workspace_bytes(H, W) bytes, iters_out (host, optional)
// B counts.  Image i is bit-identical to a B = 1 call on the same inputs.
size_t poisson_workspace_bytes(int H, int W);      // per image
hipError_t poisson_blend_batch(const uint8_t* src_hwc, const uint8_t* tgt_hwc, const uint8_t* mask, uint8_t* out_hwc, int B, int H, int W,
                               int with_gamma, int max_iters, double rel_tol, void* ws, int* iters_out, hipStream_t s);
hipError_t blend_mask_batch(const uint8_t* target_parsing, const uint8_t* face_parsing, uint8_t* out, int B, int H, int W, hipStream_t s);

// color_stats.hip: hair colour statistics (script_get_rgb_hsv_label.py:52-63, script_get_color_var_label.py:52-90)
constexpr int HAIR_ERODE_MAX_R = 15;          // ksize <= 31
constexpr int HAIR_COLOR_NSTAT = 22;          // == CH_COLOR_STATS
struct HairErodeRows {                        // MORPH_ELLIPSE element: half-width of row dy = -r..r at hw[dy + r]
    int r;
    int hw[2 * HAIR_ERODE_MAX_R + 1];
};
hipError_t resize_linear_u8(const uint8_t* src, uint8_t* dst, int B, int Hs, int Ws, int C, int Hd, int Wd, hipStream_t s);
hipError_t hair_erode(const uint8_t* labels, int B, int Hl, int Wl, int label, const HairErodeRows& rows, uint8_t* mask, int H, int W,
                      hipStream_t s);
hipError_t hair_color_stats(const uint8_t* img, const uint8_t* mask, int B, int H, int W, int64_t* sums, hipStream_t s);

// ingest.hip: a ragged batch of decoded uint8 images -> float32 [N,3,P,P] network input (Pillow's antialiased BILINEAR or cv2's
// INTER_LINEAR resize, then a float table [3][256] indexed by the resized byte), and of label maps -> uint8 [N,S,S] (nearest).
// batch: HOST bytes, N descriptors and then the coefficient tables they point to (ingest_batch.h); the launchers take only a batch
// that ingest_check has passed, and a workspace of the size it returned.
hipError_t ingest_images(const void* batch, size_t batch_bytes, int N, int P, int mode, const float* lut, float* out, void* ws,
                         hipStream_t s);
hipError_t ingest_labels(const void* batch, size_t batch_bytes, int N, int S, uint8_t* out, void* ws, hipStream_t s);

// orient.hip: EXIF orientations 1..8 of a ragged batch of uint8 images in one launch.  batch: HOST bytes, N descriptors (orient_batch.h);
// the launcher takes only a batch that orient_check has passed, and a workspace of the size it returned.
hipError_t orient_u8(const void* batch, size_t batch_bytes, int N, uint8_t* dst, void* ws, hipStream_t s);

// sheet.hip: contact sheets and per-render measurements of a direction search (shape_branch/script_find_direction.py:55-76,
// util/canvas_grid.py:15-31).  See ch_sheet_compose / ch_sweep_stats in ctrlhair_hip.h.
constexpr int SWEEP_NSTAT = 16;               // == CH_SWEEP_STATS
hipError_t sheet_compose(const void* src, int kind, int n, int Hs, int Ws, const int* cells, const uint8_t* lut, uint8_t* canvas, int rows,
                         int cols, int H, int W, int margin, hipStream_t s);
hipError_t sweep_stats(const void* img, int kind, const uint8_t* labels, const int* ref, int N, int H, int W, int h, int w, int64_t* stats,
                       hipStream_t s);

// mask_warp.hip: hair-shape transfer warp (wrap_codes/mask_adaptor.py:87-143): batched ARAP solve of packed 2-D triangle meshes, then
// UV render + mask sampling + compose into uint8 [B,512,512] label maps.  desc_host: B x {v_off, n_v, f_off, n_f, b_off, n_b} (host).
constexpr int WARP_MAX_V = 2048;              // vertices / triangles of one pair's mesh (LDS budget of arap_solve_kernel)
constexpr int WARP_MAX_F = 4096;
constexpr int WARP_DESC_PAIRS = 16;           // descriptors reach the workspace as kernel arguments, this many pairs per store launch
struct WarpDesc {
    int n, pair0;
    int d[WARP_DESC_PAIRS][6];
};
size_t mask_warp_workspace_bytes(int B);
hipError_t mask_warp_batch(const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int* F, const int* bidx,
                           const float* bc, const int* desc_host, const float* U_in, uint8_t* labels_out, float* uv_out, float* U_out,
                           void* ws, int B, int outer_iters, int max_cg, float rel_tol, hipStream_t s);
// the same with the descriptors in device memory (desc_dev int [B,6]): they are copied to the workspace by a kernel that validates
// them (counts within the caps, n_f >= 1, offsets >= 0); a pair that fails is drawn with the identity map
hipError_t mask_warp_batch_dev(const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int* F, const int* bidx,
                               const float* bc, const int* desc_dev, const float* U_in, uint8_t* labels_out, float* uv_out, float* U_out,
                               void* ws, int B, int outer_iters, int max_cg, float rel_tol, hipStream_t s);

// delaunay.hip: exact Delaunay triangulation of B planar point sets on the 2^-20 grid of [0, 1024), one workgroup per set.
// v_desc_host: B x {v_off, n_v} (host).  F int [B, WARP_MAX_F, 3], n_f int [B], status int [B] (device).
constexpr int DELAUNAY_DESC_SETS = 64;        // descriptors reach the workspace as kernel arguments, this many sets per store launch
struct DelaunayDesc {
    int n, set0;
    int d[DELAUNAY_DESC_SETS][2];
};
enum DelaunayStatus {                         // == CH_DELAUNAY_* in ctrlhair_hip.h
    DELAUNAY_OK = 0,
    DELAUNAY_BAD_COUNT = 1,
    DELAUNAY_OFF_GRID = 2,
    DELAUNAY_DUPLICATE = 3,
    DELAUNAY_COLLINEAR = 4,
    DELAUNAY_INTERNAL = 5,
};
size_t delaunay_workspace_bytes(int B);
hipError_t delaunay_batch(const float* V, const int* v_desc_host, int* F, int* n_f, int* status, void* ws, int B, hipStream_t s);

// face_align.hip: FFHQ face alignment of one photo (external_code/crop.py:20-107): Pillow's 8-bit Lanczos resample, its QUAD / BILINEAR
// transform fused into the horizontal Lanczos pass, and the reflect-pad / Gaussian-feather / median branch of the reference, all exact.
struct LanczosTable {                          // Pillow's precompute_coeffs + normalize_coeffs_8bpc for one (in, out) size pair
    int in_size = 0, out_size = 0, ksize = 0;
    std::vector<int32_t> data;                 // bounds [out][2] (first tap, tap count) | kk [out][ksize] | the same transposed [ksize][out]
};
struct AlignCache {                            // host tables, built on first use and kept (the handle owns one)
    std::map<std::pair<int, int>, LanczosTable> tables;
};
struct AlignPlan {                             // ctrlhair_amd/alignment.py align_plan, see CH_ALIGN_PLAN_LEN in ctrlhair_hip.h
    int shrink, rw, rh;                        // shrink > 1: Lanczos-resize the photo to rw x rh first
    int cx0, cy0, cx1, cy1;                    // crop box in the (resized) photo
    int do_pad, pl, pt, pr, pb;                // padding branch and its widths (left, top, right, bottom)
    double q[8];                               // Pillow's bilinear-quad coefficients
    int T, S;                                  // transform_size, output_size
};
// ws sizes in bytes; every launcher enqueues on s without synchronising (host tables are copied with hipMemcpyAsync from pageable memory)
size_t lanczos_workspace_bytes(int Hs, int Ws, int C, int Hd, int Wd);
hipError_t lanczos_resample_u8(AlignCache& cache, const uint8_t* src, long long stride, int Hs, int Ws, int C, uint8_t* dst, int Hd, int Wd,
                               void* ws, hipStream_t s);
size_t quad_warp_workspace_bytes(int T, int S);
hipError_t quad_warp_resample_u8(AlignCache& cache, const uint8_t* src, long long stride, int Hs, int Ws, const double* coef, int T, int S,
                                 uint8_t* dst, void* ws, hipStream_t s);
size_t align_pad_workspace_bytes(int Hp, int Wp, int radius);
hipError_t align_pad_feather_u8(const uint8_t* src, long long stride, int Hs, int Ws, const int* pads, const double* gauss_w, int radius,
                                uint8_t* dst, void* ws, hipStream_t s);
size_t face_align_workspace_bytes(int H, int W, const AlignPlan& p, int radius);
hipError_t face_align(AlignCache& cache, const uint8_t* src, int H, int W, const AlignPlan& p, const double* gauss_w, int radius, uint8_t* dst,
                      void* ws, hipStream_t s);

// face_unalign.hip: paste N edited crops back into the photo (the inverse map of an alignment plan: ctrlhair_amd/alignment.py
// unalign_plan): rotated scale-adaptive Lanczos-3 resample fused with a feathered composite.  See ch_face_unalign in ctrlhair_hip.h.
struct UnalignPlan {
    double A[6];                               // photo pixel centre -> crop coordinates, row-major [2][3]
    int x0, y0, x1, y1;                        // the quad's bounding box, clipped to the photo
    double scale;                              // crop pixels per photo pixel
    int S;                                     // the crop's side
};
hipError_t face_unalign(const uint8_t* photo, const uint8_t* edits, const uint8_t* weight, const UnalignPlan& p, int H, int W, int N,
                        double feather_px, uint8_t* out, hipStream_t s);

// face_matte.hip: the same paste-back with alpha = a colour guided filter of the nearest-sampled weight map (guide: the photo's RGB
// over the bounding box, exact integer window moments, float64 solve) times the border ramp.  ws: face_matte_workspace_bytes(bw, bh)
// bytes, 256-byte aligned; alpha_out: optional float [bh,bw].  See ch_face_unalign_matte in ctrlhair_hip.h.
size_t face_matte_workspace_bytes(int bw, int bh);
hipError_t face_unalign_matte(const uint8_t* photo, const uint8_t* edits, const uint8_t* weight, const UnalignPlan& p, int H, int W, int N,
                              double feather_px, int radius, double eps, uint8_t* out, float* alpha_out, void* ws, hipStream_t s);

// style_medoid.hip: per-segment medoid (first minimum of the float64 row sums of float32 difference-form distances) and float64 mean
// of compacted style codes (sean_codes/get_mean_code.py); seg_offsets is a host array [R + 1].  See ch_style_medoid in ctrlhair_hip.h.
size_t style_medoid_workspace_bytes(const int64_t* seg_offsets, int R, int n_split);
hipError_t style_medoid(const float* codes, const int64_t* seg_offsets, int R, int dim, int n_split, int* index, double* sums, float* mean,
                        void* ws, hipStream_t s);

// png_encode.hip: N uint8 images [N,H,W,C] -> N complete zlib streams of their PNG-filtered bytes (row filters, chunk-wise deflate with
// distance-1 matches and a dynamic Huffman code per chunk, gather + Adler-32).  See ch_png_encode in ctrlhair_hip.h.
constexpr int PNG_CHUNK = 32768;              // == ch_png_chunk_bytes(): bytes of the filtered stream one workgroup deflates
size_t png_zlib_bound(int H, int W, int C);
size_t png_encode_workspace_bytes(int N, int H, int W, int C);
hipError_t png_encode(const uint8_t* img, int N, int H, int W, int C, int filter, uint8_t* out, int64_t* sizes, void* ws, hipStream_t s);
// the same with matches at ndist (0..3) further distances dist[] (host values, 2..32767, distinct); ndist = 0 is png_encode
hipError_t png_encode_dist(const uint8_t* img, int N, int H, int W, int C, int filter, const int* dist, int ndist, uint8_t* out,
                           int64_t* sizes, void* ws, hipStream_t s);

// png_decode.hip: N zlib streams (stream n = streams[offsets[n], offsets[n + 1]), device) -> uint8 images [N,H,W,C]: inflate (one wave per
// stream, png_inflate_core.h) into the workspace, then the PNG row filters undone.  status[n]: pnginf::Status.  See ch_png_decode.
size_t png_decode_workspace_bytes(int N, int H, int W, int C);
hipError_t png_decode(const uint8_t* streams, const int64_t* offsets, int N, int H, int W, int C, uint8_t* img, int32_t* status, void* ws,
                      hipStream_t s);

// jpeg_encode.hip: N uint8 images [N,H,W,C] (C = 1 or 3) -> N baseline-JPEG entropy-coded scans (libjpeg's integer arithmetic, the
// Annex K Huffman tables, byte-stuffed and padded).  subsampling: 0 = 4:4:4, 2 = 4:2:0 (ignored for C = 1).  See ch_jpeg_encode.
size_t jpeg_scan_bound(int H, int W, int C, int subsampling);
size_t jpeg_encode_workspace_bytes(int N, int H, int W, int C, int subsampling);
hipError_t jpeg_encode(const uint8_t* img, int N, int H, int W, int C, int quality, int subsampling, uint8_t* out, int64_t* sizes, void* ws,
                       hipStream_t s);

// jpeg_decode.hip: N baseline-JPEG entropy-coded scans (stream n = streams[offsets[n], offsets[n + 1]), its table block at tables +
// n * 2048; jpeg_entropy_core.h) -> uint8 images [N,H,W,C] (C = 1 or 3).  sampling: 0 = 4:4:4 (and grey), 1 = 4:2:2, 2 = 4:2:0.  rounds:
// launches of the state hand-over between chunks, 0 = the default.  status[n]: jpegent::Status.  restart: null, or per stream its restart
// interval in MCUs (device, [N]; 0 = none).  See ch_jpeg_decode and ch_jpeg_decode_rst.
int jpeg_decode_default_rounds();
size_t jpeg_decode_workspace_bytes(int N, int H, int W, int C, int sampling);
hipError_t jpeg_decode(const uint8_t* streams, const int64_t* offsets, const uint8_t* tables, const uint32_t* restart, int N, int H, int W, int C,
                       int sampling, int rounds, uint8_t* img, int32_t* status, void* ws, hipStream_t s);

}  // namespace chk
