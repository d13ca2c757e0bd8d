/*
 * ctrlhair_hip.h -- C ABI of libctrlhair_hip.so: the MI355X (gfx950) implementation of the CtrlHair
 * convolutional GAN *inference* forward path.
 *
 * The reference (XuyangGuo/CtrlHair) is pure Python on torch.nn; it has no FFI of its own.  Each entry
 * point below therefore replaces a Python call site of the reference (cited per function), and is what a
 * ctypes binding added to the reference would bind.  Plain pointers and sizes only;
 * no torch types.  All device pointers are HIP device memory owned by the caller; all work is enqueued on
 * the caller's stream; no entry point synchronises the device except ch_finalize()/ch_destroy().
 *
 * Error convention: int status, 0 = ok, non-zero = failure; message via ch_last_error().  No C++ exception
 * crosses the ABI.  A handle is bound to one device and is not thread-safe; different handles are independent.
 */
#ifndef CTRLHAIR_HIP_H
#define CTRLHAIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CH_ABI_VERSION 1

typedef struct ch_handle ch_handle;
typedef void* ch_stream_t;              /* hipStream_t */

enum ch_status { CH_OK = 0, CH_ERR_ARG = 1, CH_ERR_HIP = 2, CH_ERR_STATE = 3, CH_ERR_WEIGHTS = 4 };

/* which network a tensor belongs to (one handle can hold all of them) */
enum ch_model {
    CH_MODEL_SEAN = 0,         /* sean_codes/models/networks/generator.py: SPADEGenerator (+Zencoder) */
    CH_MODEL_SHAPE = 1,        /* shape_branch/model.py: Generator (hair/face MaskEncoder + MaskDecoder), cfg 054 */
    CH_MODEL_COLOR = 2,        /* color_texture_branch: EigenGenerator "gen.*", Discriminator "dis.*", rgb Predictor "rgb.*" */
    CH_MODEL_BISENET = 3       /* external_code/face_parsing/model.py: BiSeNet(19) */
};

enum ch_dtype { CH_F32 = 0, CH_I64 = 1 };

int  ch_abi_version(void);

/* Replaces model construction + .cuda(): sean_codes/models/networks/__init__.py:39-51 (create_network),
 * hair_editor.py:45-51.  Binds the handle to HIP device `device`. */
int  ch_create(int device, ch_handle** out);
void ch_destroy(ch_handle* h);
const char* ch_last_error(const ch_handle* h);

/* Replaces util/util.py:202-208 (load_network -> net.load_state_dict): hand over one state-dict entry under its
 * reference key name (e.g. "up_0.conv_0.weight_orig", "head_0.ace_0.fc_mu3.weight").  `host` is host memory,
 * copied before return.  Unknown names are kept and ignored at finalize (the reference state dict carries unused
 * buffers: Spade.param_free_norm.*, num_batches_tracked). */
int  ch_load_tensor(ch_handle* h, int model, const char* name, const void* host, int dtype,
                    const int64_t* shape, int ndim);

/* Options, set before ch_finalize.  "sean.f16x3" (default 0) selects the arithmetic of the SEAN generator's MFMA convs:
 *   0  f32 throughout on the f32 matrix cores (v_mfma_f32_16x16x4_f32 / 32x32x2_f32: every product and every sum an IEEE f32
 *      operation); with "sean.wino" >= 1 the 3x3 convs are evaluated as Winograd convolutions (ctrlhair_amd/csrc/conv_wino.h,
 *      conv_wino4.h: f32 operands and f32 accumulation, but TRANSFORMED operands -- U = G g G^T is computed in double and rounded
 *      once to f32, the input / output transforms are f32 adds / fmas -- so this is not a re-association of the direct sum and
 *      carries its own rounding error: F(2x2,3x3) <= ~4e-6 against the direct evaluation on the generator output, F(4x4,3x3)
 *      (the default for the ResBlock convs and the SPADE convs up to 64 pixels) <= ~3e-5; the contract tolerance is 1e-3),
 *      with 0 directly (conv_mfma.h: the reference conv2d's products and sums);
 *   1  f16 matrix cores with the 3-term split-operand scheme of ctrlhair_amd/csrc/conv_sh16.h: f32-class accuracy, f32
 *      accumulation, activations between ACE and conv stored as f16 hi/lo pairs;
 *   2  f16 matrix cores, single term: operands rounded to f16, f32 accumulation and f32 normalisation / modulation
 *      (the reduced-precision configuration of BASELINE.json configs[4]; tolerance 5e-2);
 *   3  bf16 matrix cores (v_mfma_f32_32x32x16_bf16), single term: operands rounded to bf16, f32 accumulation and f32
 *      normalisation / modulation -- configs[4] as written ("bf16 MFMA conv path"; tolerance 5e-2).
 * "sean.ahead" (default 8): run-ahead mode -- when a batch chunk holds at most `value` x 512x512 pixels, the kernels of the
 *   18 ACE layers that depend only on the label map and the style codes (label tables, fc_mu, style LUTs) run on an internal
 *   side stream into per-layer buffers, joined to `stream` by events (interactive latency: 3.3 -> 2.65 ms at 256x256; still
 *   1.6 % at 8 x 512x512).  Handles sized for larger chunks run only the style LUT builds (small GEMMs) ahead and keep the
 *   HBM-write-bound label-table kernels inline (1 % at 16 x 512x512; with the label tables ahead too: no gain).  0 = off.
 * "shape.f16x3" (default 1): the shape VAE's convs run on the same f16x3 split-operand kernels -- all encoder layers (k4,
 *   stride 2: space-to-depth staging), decoder layers 1-6 and the output convs; LayerNorm outputs and the one-hot / sin-cos
 *   inputs are bounded, so their scales are static; 0 = every conv on the exact-f32 kernels.
 * "bisenet.f16x3" (default 1): BiSeNet's convs on the f16x3 kernels; its f32 activations stay in the C4 layout and are split
 *   into f16 pairs while staged, with the scale derived from the maximum the producing kernel recorded; 0 = exact-f32 kernels.
 *   (The Zencoder follows "sean.f16x3".)
 * "aux.wino" (default 1): the exact-f32 kernels of the shape VAE and BiSeNet ("shape.f16x3" / "bisenet.f16x3" = 0, and the layers those
 *   options leave on them) run their 3x3 stride-1 convs as Winograd F(2x2,3x3) wherever the output fits the kernel's tiles; 0 = direct.
 * "sean.wino" (default 2; "sean.f16x3" = 0 only): 1 = the ResBlock 3x3 convs, the SPADE gamma/beta convs and the style convs as
 *   Winograd F(2x2,3x3) on the f32 matrix cores, the learned 1x1 shortcuts on the pointwise kernel of conv_pw.h; 2 = in addition the
 *   ResBlock convs from 32 pixels up as Winograd F(4x4,3x3) (conv_wino4.h: 36 instead of 64 products per 4 x 4 pixels); 0 = direct.
 * "sean.wino4_ace" (default 64; with "sean.wino" = 2): the SPADE / style convs of the levels up to this many pixels (multiples of 32)
 *   run as dense F(4x4,3x3) over every tile instead of F(2x2,3x3) over the boundary quads; 0 = never.
 *   Both F(4x4,3x3) choices are made per call: with fewer tasks of 32 x 32 pixels than a round of F(2x2,3x3) tasks would need CUs (single
 *   images, small batches of small images) the F(2x2,3x3) kernels run instead (wino4_pays, conv_wino4.h); "sean.wino4_force" = 1 (any
 *   time) switches that rule off.
 * "sean.edge" (default 1; before ch_finalize; exact-f32 Winograd path and the f16x3 / f16 / bf16 paths with pixel-level compaction): a boundary pixel whose 5 x 5 label neighbourhood is five uniform
 *   columns (or rows) A..A B..B -- one straight, axis-aligned piece of a region border -- takes gamma / beta from the row of its code
 *   (orientation, A, B, number of A columns: 2888 rows per ACE, built at ch_finalize in double) plus three column / row sums of the style
 *   LUT, in the interior pass, on the levels of 128 pixels and more; only corners, curved pieces and the image frame go through the
 *   boundary conv (csrc/ace_sparse.h).  Same real number, another association of the f32 sums (<= 1e-6 against "sean.edge" = 0;
 *   f16x3: <= 5e-6; on the single-term f16 / bf16 paths the table rows are exact f32 where the conv they replace is not).
 *   Costs 55 MB of tables at ngf = 64 (3040 rows per ACE on every path that builds them: the 152 rows of "sean.frame" are always there).  0 = every non-interior pixel through the conv.
 * "sean.frame" (default 1; before ch_finalize; effective only with "sean.edge" = 1 on the exact-f32 Winograd path, levels of 128 pixels and
 *   more): a pixel of the two outermost rings of a level whose 5 x 5 window reaches outside the image along exactly one axis, and whose
 *   labels inside the image all equal its own label A < 19, is served like a straight-edge pixel: both SPADE convs and the style convs
 *   zero-pad, so a tap outside adds nothing and a hidden position outside is zero (2 x 19 x 4 = 152 more rows per ACE behind the 2888:
 *   orientation, A, which border and distance).  The 2 x 2 pixels at each image corner stay with the boundary conv.  <= 1e-5 against
 *   "sean.frame" = 0.  The f16x3 / f16 / bf16 paths do not use it.  0 = frame pixels through the boundary conv.
 * "sean.convt_gemm" (default 1; before ch_finalize; exact-f32 path): the Zencoder's ConvTranspose2d(128, 256, k3, s2, p1, op1)
 *   (architecture.py:167-170) as four phase GEMMs over shifted views of its input -- 9 products per 2 x 2 outputs and channel pair -- with the
 *   InstanceNorm + lrelu that follows reading the phase planes; calls with fewer than 16384 input pixels and 0 = four Winograd F(2x2,3x3)
 *   phase convs (16 products).  Same sums in another order (<= 1e-6 on the style codes).
 * "sean.patch" (default 1; before ch_finalize): when a level is left with few boundary quads (at most 32 chunks of 64 per sample) their
 *   hidden-activation patches are written pre-gathered, in the conv kernel's stage layout, instead of being fetched piecewise from the
 *   planes (csrc/conv_wino.h WinoAceParams::patch); decided per level and call on the device; bit-identical.  0 = planes only.
 * "sean.int_groups" (default 0; any time; exact-f32 Winograd path, levels of 128 pixels and more): a block of the four-pixel interior pass
 *   (csrc/ace_sparse.hip, ace_interior_f32_tile4_kernel) sets up its 128 x 8 pixels once -- marks, noise, ownership, the slots of its
 *   straight-edge codes -- and then serves several groups of 32 channels.  0 = per launch, the largest divisor of the group count that
 *   leaves at least sixteen blocks per compute unit in the grid; n >= 1 = at most n groups per block (1 = one group per block, the
 *   decomposition before the group loop).  Bit-identical for every value.
 * "sean.int_onepass" (default 1; any time; same kernel): 1 = a block hashes its distinct straight-edge codes into 128 key slots and, where
 *   it holds more than 64 of them (label maps with many small regions: 16 x 16-block maps at the 128-pixel level), runs steps of 16
 *   channels over a table of 128 rows, so up to 128 codes are served in one round with whole-line stores; beyond 128, further rounds.
 *   0 = 64 key slots, steps of 32 channels, another round for every further 64 codes.  Bit-identical.
 * "sean.batch_invariant" (default 0; any time; exact-f32 path): by default several choices follow the number of tasks of a call, i.e. its
 *   batch size -- F(4x4,3x3) vs F(2x2,3x3) (wino4_pays), split-K of launches with few tasks, sample-pair tiles of the 16-pixel level, the
 *   GEMV / tiny-level routes of interactive batches -- so the same sample rendered alone and inside a batch differs by the rounding of two
 *   associations of the same f32 sums (measured <= 3e-5 at 512 x 512).  1 = every such choice is made as for a large batch: sample i
 *   alone == sample i in any batch of the same handle, bit for bit (tests/test_hip_sean_generator.py); costs latency on small calls
 *   (bench.py reports both).
 * "sean.wino4v" (default 1; before ch_finalize; with "sean.wino" = 2): F(4x4,3x3) layers with at least 512 GEMM rows at up to 64 x 64
 *   pixels -- the ResBlock convs of G_middle / up_0 and every SPADE / style conv that "sean.wino4_ace" selects -- and the Zencoder's
 *   256 -> 512 conv read their input pre-transformed (V = B^T d B, written once by an extra bandwidth-bound pass, csrc/conv_wino4v.h)
 *   instead of transforming it again in every row tile; same arithmetic in the same order: bit-identical results.  Costs a workspace
 *   of 9 bytes per input element of the largest such layer (604 MB at max_batch 16, 512 x 512).  0 = transform inside the conv kernel.
 * "sean.wino4_split" (default -1; before ch_finalize; with "sean.wino" = 2): the plain F(4x4,3x3) convs that transform their input inside
 *   the kernel (everything the V route of "sean.wino4v" does not take) on wino4_plain_split_kernel (csrc/conv_wino4_split.h): the two waves
 *   that share a group of tiles split the 36 Winograd positions instead of the 32 GEMM rows, so each does half of the input transform, and
 *   they exchange partial output transforms once per task; same operations on the same values in the same order: bit-identical results.
 *   0 = never, 1 = wherever the shape allows, -1 = per layer shape where it measured faster (wino4_split_pays, csrc/conv_wino4.h).  Costs a
 *   second weight image per such layer: 37 MB at ngf = 64 with -1 (the layers below 512 GEMM rows), 470 MB with 1 (every layer).
 * "sean.overlap" (default 0; before ch_finalize): number of CUs given to CU-masked side streams on which the interior passes and
 *   label-table kernels run beside the convs (with dynamic task claiming in the Winograd kernels).  Bit-identical results; measured
 *   SLOWER than the serial order at every setting on MI355X: kept as an option, not used.
 * "sean.lut_grouped" (default 1; exact-f32 path, calls with more than 64 (sample, label) columns): the style LUTs of all styled ACEs
 *   of a chunk come from ONE grouped GEMM launch at its start (csrc/conv_pw.h); 0 = one launch of the generic 1x1 kernel per ACE.
 * "sean.pw_wide" (default 1; any time; exact-f32 path): 1 = the 1x1 GEMM kernel (csrc/conv_pw.h) with wave tiles of 64 rows x 64 pixels
 *   (pw_conv_wide_kernel) for the learned shortcuts with at least 64 output channels and a multiple of 256 pixels per plane, for the
 *   Zencoder's phase GEMMs and for the grouped style-LUT launch of "sean.lut_grouped" (when every styled ACE has 18 C % 256 == 0);
 *   fc_mu reduces a wave's 32 partial sums through one transposed butterfly; the F(4x4,3x3) style images are packed by one thread per
 *   (GEMM row, label), their constant zero units written once per handle.  0 = the kernels of round 11.  Bit-identical results.
 * "sean.prologue" (default 1; before ch_finalize; exact-f32 Winograd path, handles beyond the run-ahead sizes of "sean.ahead"): what the ACEs
 *   of a chunk build from labels, codes and weights alone -- level geometry, hidden planes of the 32 / 64-pixel ACEs, gamma / beta tables,
 *   column / row sums and F(2x2) style images of the ACEs from 128 pixels -- comes from a few grouped launches at the start of the chunk,
 *   into per-ACE buffers (+456 MiB on a 16 x 512^2 handle at ngf = 64).  Bit-identical results.  Off by
 *   itself with "sean.f16x3", "sean.overlap" and while ch_profile_enable is on.  0 = every ACE launches its own kernels, inline.
 * "sean.label_memo" (default 1; before ch_finalize; handles with "sean.prologue" in effect): the label-only products of a chunk -- level
 *   label maps, classification, level geometry, hidden planes of the 32 / 64-pixel ACEs, pre-gathered patches of the ACEs from 128 pixels
 *   (one patch buffer per ACE) -- stay on the device; a call of one chunk compares its label maps with the handle's copy on the device and
 *   the launches that build those products return at once when nothing changed (same shapes, same options).  Bit-identical results.
 *   0 = no memo and none of its buffers.  ch_sean_label_memo_stats counts.
 * "sean.spade_memo" (default 1; before ch_finalize; in effect with "sean.label_memo" only): the SPADE conv of a styled 32 / 64-pixel ACE
 *   contracts 128 hidden channels, which depend on labels and weights alone, and then the one-hot planes with the style images of the
 *   sample.  1 = the second call in a row with the same label maps stores the Winograd-domain accumulators of every task after the hidden
 *   part (4.2 GiB on a 16 x 512^2 handle at ngf = 64), the following ones load them and run the style part only.  Bit-identical results:
 *   every accumulator receives the same operations in the same order.  0 = none of it.  ch_sean_spade_memo_stats counts.
 * "sean.code_memo" (default 1; before ch_finalize; handles with "sean.lut_grouped" in effect): the projected codes and the style LUTs of all
 *   styled ACEs stay on the device; a call of one chunk that takes the grouped launch compares its style codes, as integer words, with the
 *   handle's copy on the device (1.2 MiB at 16 samples), and the projection and the grouped GEMM return at once when nothing changed (same
 *   batch, same options).  Independent of "sean.label_memo"; off while ch_profile_enable is on.  Bit-identical results.  0 = no memo and
 *   none of its buffers.
 *   ch_sean_code_memo_stats counts.
 * "sean.hidden_wq" (default 1; any time): every Winograd ACE level (32 pixels and more) takes the SPADE hidden activations and the
 *   one-hot planes from one persistent kernel (csrc/sean_kernels.hip spade_hidden_wq).  1 = on the gather levels it writes only the
 *   64-byte pixel groups that a boundary quad's patch touches; 0 = the same kernel over every pixel (bit-identical results).  The dense
 *   F(4x4,3x3) levels ("sean.wino4_ace") read every pixel either way.  (The two-kernel route of round 4 -- label table + one-hot kernel --
 *   serves the levels below 32 pixels only.)
 * "sean.wino_gather" (default 1): the Winograd ACE kernel takes tasks of 64 consecutive boundary quads of a sample and fetches each
 *   quad's own 4 x 4 patch (csrc/conv_wino.h); 0 = tasks per tile of 32 x 16 / 32 x 32 pixels (bit-identical results).
 * "sean.wino_th": tile height 16 / 32 of the tile mode (0 = chosen per resolution level).
 * "sean.sparse" (default 1): the exact SPADE-interior reduction (csrc/ace_sparse.h).  May be switched off (and back on) after
 *   ch_finalize; a handle finalised with 0 has no classification buffers and rejects 1 afterwards (CH_ERR_STATE).
 * "sean.sparse_min", "sean.sparse_th", "sean.sh16_compact": tuning knobs of that reduction (before ch_finalize).
 * "sean.dbg": profiling switches.  The bits that skip work (wrong results) or select superseded kernel versions exist only in
 *   libraries built with -DCH_ABLATE (make -C ctrlhair_amd/csrc ABLATE=1); the default build rejects them (CH_ERR_ARG).  Every bit
 *   is listed, with its value and meaning, in ctrlhair_amd/csrc/dbg_bits.h.
 * "sean.dbg_sel" (default 16; any time): index of the ACE launch that "sean.dbg" bit 256 cycle-stamps. */
int  ch_set_option(ch_handle* h, const char* key, int value);

/* Fold + pack + upload the loaded tensors: spectral-norm sigma (torch spectral_norm eval semantics,
 * architecture.py:42-46), eval-BN running stats -> per-channel affine (sync_batchnorm/batchnorm.py:52-55),
 * sigmoid(blending) folded into the SPADE / style weights (normalization.py:177-181), one-hot convs -> label
 * LUTs, MFMA operand layouts.  Sizes the workspace arena for images up to max_size x max_size in chunks of
 * max_batch.  ngf is inferred from the tensors.  For CH_MODEL_SHAPE / CH_MODEL_COLOR max_size is ignored.
 * Synchronises the device. */
int  ch_finalize(ch_handle* h, int model, int max_batch, int max_size);

/* Floats of noise per sample at image side S: sum over the 18 ACE layers (execution order: ace_s, ace_0, ace_1
 * per block) of (S/res_div)^2 -- the planes normalization.py:111 draws as randn(B, W, H, 1). */
size_t ch_sean_noise_floats(const ch_handle* h, int S);

/* Replaces Pix2PixModel.forward(data, mode='UI_mode') -> SPADEGenerator.forward
 * (sean_codes/models/pix2pix_model.py:59-68,119-144; generator.py:72-109; architecture.py:69-96;
 * normalization.py:108-189), batched: every sample b gets the UI_mode treatment the reference gives sample 0.
 *   labels : device uint8  [B,S,S]       CelebAMask-HQ ids 0..18 (the one-hot of pix2pix_model.py:133-138 is
 *                                        never materialised)
 *   codes  : device float  [B,19,512]    per-region style codes (obj_dic[str(j)]['ACE'])
 *   noise  : device float  [B,noise_floats(S)] explicit noise planes n_k[b][w][h], or NULL to draw them on
 *            device from `seed` (counter-based generator; the reference draws torch.randn)
 *   out    : device float  [B,3,S,S]     image in [-1,1] (tanh)
 * S must be a multiple of 32 with S <= max_size.  Asynchronous on `stream`. */
int  ch_sean_generate(ch_handle* h, const uint8_t* labels, const float* codes, const float* noise, uint64_t seed,
                      float* out, int B, int S, ch_stream_t stream);

/* The noise planes ch_sean_generate(noise = NULL, seed) draws on device, written out: noise [B, noise_floats(S)] (device).
 * ch_sean_generate(..., noise = these planes, ...) reproduces the NULL call bit for bit; the planes are i.i.d. N(0,1) from a
 * counter-based generator (the reference draws torch.randn from an unseeded global generator, normalization.py:111). */
int  ch_sean_draw_noise(ch_handle* h, uint64_t seed, float* noise, int B, int S, ch_stream_t stream);

/* Replaces Pix2PixModel.forward(data, mode='style_code') -> Zencoder.forward
 * (pix2pix_model.py:69-72; architecture.py:177-207; callers hair_editor.py:149-157 get_code, :208-231):
 * conv stack (reflection-padded 3x3, two stride-2 convs, ConvTranspose2d, InstanceNorm + LeakyReLU, tanh) at
 * S/2 resolution, then per-region average pooling with the label map nearest-down-sampled to S/2.
 *   img    : device float [B,3,S,S] in [-1,1]        labels : device uint8 [B,S,S]
 *   codes  : device float [B,19,512] (rows of absent regions are 0)
 * Requires the Zencoder.* tensors to have been loaded before ch_finalize. */
int  ch_sean_encode(ch_handle* h, const float* img, const uint8_t* labels, float* codes, int B, int S,
                    ch_stream_t stream);
/* The same encoder in two calls, for callers that compute the label map while the convolutions run (the labels only enter
 * the region means, architecture.py:185-205): ch_sean_encode_features runs the convolutional part and keeps the feature map
 * in the handle's workspace; ch_sean_encode_regions reduces it to codes.  One chunk (B <= max_batch); the second call must
 * follow the first with the same B, S (else CH_ERR_HIP), with no other SEAN call on the handle in between, and be ordered
 * after it (same stream, or an event).  ch_sean_encode(img, labels, codes) == features(img); regions(labels, codes). */
int  ch_sean_encode_features(ch_handle* h, const float* img, int B, int S, ch_stream_t stream);
int  ch_sean_encode_regions(ch_handle* h, const uint8_t* labels, float* codes, int B, int S, ch_stream_t stream);

/* ---- colour / texture branch (three MLPs on 512-d hair style codes) -------------------------------------------
 * Tensor names: the reference state-dict keys prefixed "gen." (EigenGenerator, model_eigengan.py:34-84), "dis."
 * (Discriminator used as encoder, model.py:86-130) and "rgb." (Predictor p004, predictor_model.py:14-41).
 * ch_color_generate replaces feature_generator(data)['code'] (ui/backend.py:166-169, solver.py:78-83):
 *   noise [B,8], cond [B,5] = cat(noise_curliness[1], rgb_mean[3], pca_std[1]) (model_eigengan.py:66-74) -> code [B,512]
 * ch_color_encode replaces feature_encoder({'code'}) (ui/backend.py:103-105): raw net output [B,11]; columns
 *   0 = adv, 1..8 = noise, 9 = noise_curliness, 10 unused (model.py:112-127 slices them on the host).
 * ch_color_predict replaces feature_rgb_predictor({'code'}) (ui/backend.py:96): [B,4] = rgb_mean[3], pca_std[1]. */
int  ch_color_generate(ch_handle* h, const float* noise, const float* cond, float* code, int B, ch_stream_t stream);
int  ch_color_encode(ch_handle* h, const float* code, float* out11, int B, ch_stream_t stream);
int  ch_color_predict(ch_handle* h, const float* code, float* out4, int B, ch_stream_t stream);

/* ---- shape branch (256x256 only: the Linear sizes fix it, shape_branch/model.py:85-89,120-122) ---------------
 * ch_shape_encode replaces mask_label_to_one_hot + split_hair_face + forward_hair_encoder(testing=True) +
 *   forward_face_encoder (ui/backend.py:81-86; shape_util.py:6-26; model.py:96-108,164-173):
 *   labels uint8 [B,256,256] (255 = no class) -> hair_code [B,16] (VAE mean), face_code [B,1024]; either output
 *   may be NULL to skip that encoder.
 * ch_shape_decode replaces forward_decode_by_code / forward_hair_decoder / forward_face_decoder / forward_decoder
 *   + mask_one_hot_to_label (model.py:175-199; shape_util.py:17-20; ui/backend.py:87-90,304-315):
 *   any of hair_logit [B,1,256,256], face_logit [B,18,256,256], labels uint8 [B,256,256], probs [B,19,256,256]
 *   may be NULL; hair_code NULL = face decoder only (ui/backend.py:420).
 * ch_shape_combine replaces Generator.forward_decoder on caller-made logits (ui/backend.py:421-424). */
int  ch_shape_encode(ch_handle* h, const uint8_t* labels, float* hair_code, float* face_code, int B, ch_stream_t stream);
int  ch_shape_decode(ch_handle* h, const float* hair_code, const float* face_code, float* hair_logit, float* face_logit,
                     uint8_t* labels, float* probs, int B, ch_stream_t stream);
int  ch_shape_combine(ch_handle* h, const float* hair_logit, const float* face_logit, uint8_t* labels, float* probs,
                      int B, ch_stream_t stream);

/* ---- BiSeNet face parser ---------------------------------------------------------------------------------------
 * Replaces FaceParsing.parsing_img's network part + swap_parsing_label_to_celeba_mask
 * (my_parsing_util.py:37-54; model.py:241-254 output [0] only; resnet.py:71-80):
 *   img float [B,3,H,W], already ImageNet-normalised (my_parsing_util.py:25-28); H, W multiples of 32
 *   labels uint8 [B,H,W] in CelebAMask-HQ ids;  logits (optional) float [B,19,H,W] = bilinear(align_corners) logits
 * The reference runs this network on CPU (the .cuda() calls are commented out, :37,41). */
int  ch_bisenet_parse(ch_handle* h, const float* img, uint8_t* labels, float* logits, int B, int H, int W,
                      ch_stream_t stream);

/* ---- Blending after the generator (the step that follows the hot path when Backend(blending=True)) ------------------
 * ch_blend_mask replaces hair_editor.py:297-305: hair = (target_parsing == 13) | (face_parsing == 13); out = cv2.dilate of
 *   hair with the 13x13 MORPH_ELLIPSE element, except on the target's background (label 0) where the 5x5 element is used.
 *   target_parsing, face_parsing, out: uint8 [H,W] device pointers (CelebAMask-HQ ids in, 0/1 out).
 * ch_poisson_blend replaces poisson_blending.poisson_blending (poisson_blending.py:29-87): same linear system (5-point
 *   Laplacian incl. the reference's border rows, identity rows for interior pixels with mask == 0), same gamma-2.2 round
 *   trip and uint8 truncation, solved matrix-free by conjugate gradients (Chronopoulos-Gear form, f64) instead of three sparse direct solves.
 *   source, target, out: uint8 [H,W,3] (cv2 layout); mask uint8 [H,W], non-zero = keep the SOURCE gradients (solve), zero =
 *   keep the target pixel; H, W >= 3.  Stops when ||r|| <= rel_tol * ||r0|| per channel or after max_iters iterations
 *   (recommended 1e-7 / 4000); *iters (host pointer, optional) receives the iteration count, NEGATED (INT_MIN for zero
 *   iterations) when the solve stopped at max_iters without reaching rel_tol -- checked once more after the last update
 *   (the reference uses a direct solve: an unconverged image is not its output).  Output agrees with the
 *   reference to +-1 grey level (the floor() after the gamma power amplifies last-bit differences of pow() and of the
 *   solve wherever the result sits on an integer boundary, e.g. every kept target pixel).  Run-to-run deterministic.
 * ch_blend_mask_batch / ch_poisson_blend_batch: the same two steps for B images of one size in one call (what
 *   Backend.outputs() and EditPipeline.edit_blended() blend): target_parsing, face_parsing, mask, out of ch_blend_mask uint8
 *   [B,H,W]; source, target, out uint8 [B,H,W,3]; *iters a host array of B counts (optional), each with the sign convention
 *   above.  Every CG iteration is ONE pair of launches for all B images; each image keeps its own state and stops on its own
 *   criterion, so image i is bit-identical to the single-image call on the same inputs, iteration count included (the
 *   single-image calls are the B = 1 case).  1 <= B <= 65535.  The handle's blend workspace grows to B times the
 *   single-image one (~15 f64 planes per image: 31.7 MB per 512x512 image, 0.5 GB for B = 16 at 512x512) and is kept until
 *   ch_destroy; split larger batches on the caller's side (PoissonBlender.max_workspace_bytes). */
int  ch_blend_mask(ch_handle* h, const uint8_t* target_parsing, const uint8_t* face_parsing, uint8_t* out, int H, int W,
                   ch_stream_t stream);
int  ch_poisson_blend(ch_handle* h, const uint8_t* source, const uint8_t* target, const uint8_t* mask, uint8_t* out, int H,
                      int W, int with_gamma, int max_iters, double rel_tol, int* iters, ch_stream_t stream);
int  ch_blend_mask_batch(ch_handle* h, const uint8_t* target_parsing, const uint8_t* face_parsing, uint8_t* out, int B, int H,
                         int W, ch_stream_t stream);
int  ch_poisson_blend_batch(ch_handle* h, const uint8_t* source, const uint8_t* target, const uint8_t* mask, uint8_t* out, int B,
                            int H, int W, int with_gamma, int max_iters, double rel_tol, int* iters, ch_stream_t stream);

/* ---- Hair colour statistics (dataset labels, colour-slider table, HairEditor.get_hair_color) ------------------------------
 * ch_resize_linear_u8 replaces cv2.resize(img, (Wd, Hd)) (INTER_LINEAR) of uint8 images (hair_editor.py:239): OpenCV's
 *   fixed-point arithmetic (11-bit tap weights, >> 4, >> 16, + 2 >> 2), bit-exact.  src uint8 [B,Hs,Ws,C], dst uint8
 *   [B,Hd,Wd,C] device pointers; 1 <= C <= 4, all sizes >= 1, Hd <= 65535.
 * ch_hair_erode replaces script_get_rgb_hsv_label.py:52-56 / script_get_color_var_label.py:52-56 / hair_editor.py:238-241:
 *   mask = cv2.erode((cv2.resize(labels, (W, H), INTER_NEAREST) == label), MORPH_ELLIPSE (ksize, ksize)), cv2's default
 *   border (pixels outside the image never erode).  Nearest source row min((int)(y * ((double)Hl / H)), Hl - 1), columns
 *   likewise.  labels uint8 [B,Hl,Wl], mask uint8 0/1 [B,H,W] device pointers; ksize odd, 1 <= ksize <= 31.
 * ch_hair_color_stats replaces the statistics of script_get_rgb_hsv_label.py:58-63 and script_get_color_var_label.py:58-90
 *   (moments, variances, PCA) by the exact integer sums they are finished from on the host (ctrlhair_amd/colorstats.py).
 *   img uint8 [B,H,W,3] (RGB), mask uint8 [B,H,W] (non-zero = hair) device pointers; sums int64 [B,CH_COLOR_STATS] device
 *   pointer, overwritten.  Per image: [0] pixel count, [1..3] sum c, [4..6] sum c^2, [7..9] sum c^3, [10..12] sum c^4 per
 *   RGB channel, [13..15] sum c0*c1, c0*c2, c1*c2, [16..21] sum H, H^2, S, S^2, V, V^2 of cv2's 8-bit RGB2HSV (H in [0,180)).
 *   H * W <= 2^63 / 255^4 (no overflow for any content).  Order-independent integer sums: run-to-run deterministic. */
#define CH_COLOR_STATS 22
int  ch_resize_linear_u8(ch_handle* h, const uint8_t* src, uint8_t* dst, int B, int Hs, int Ws, int C, int Hd, int Wd,
                         ch_stream_t stream);
int  ch_hair_erode(ch_handle* h, const uint8_t* labels, int B, int Hl, int Wl, int label, int ksize, uint8_t* mask, int H, int W,
                   ch_stream_t stream);
int  ch_hair_color_stats(ch_handle* h, const uint8_t* img, const uint8_t* mask, int B, int H, int W, int64_t* sums,
                         ch_stream_t stream);

/* ---- Image ingest: N decoded images of ANY sizes -> the input tensor of a network, in one call ---------------------------------
 * The step between a decoder's uint8 [H,W,3] device tensors and float32 [N,3,P,P]: resize to P x P on 8-bit data, then
 * out[n][c][y][x] = lut[c][resized byte].  lut: device float [3][256], whatever normalisation the caller evaluated once over the 256
 * byte values (ctrlhair_amd/ingest.py: FaceParsing.normalise of a ramp image for the parse network, x / 127.5 - 1 for SEAN), so the
 * floats have the bits of the caller's own arithmetic and the kernels hold none of it.
 * ch_ingest_images, mode CH_INGEST_PIL_BILINEAR: Image.resize((P, P), Image.BILINEAR) of an 8-bit RGB image (ImagingResample).  Per
 *   axis, in double: scale = in / out, fs = max(scale, 1), support = fs; per output i: center = (i + 0.5) scale, first =
 *   max((int)(center - support + 0.5), 0), last = min((int)(center + support + 0.5), in), weights w_j = max(0, 1 - |(j + first -
 *   center + 0.5) / fs|) for j < last - first, divided by their sum taken in that order, k_j = (int)(w_j 2^22 + 0.5).  A pass is
 *   clip8(((1 << 21) + sum k_j p_j) >> 22) in int32; horizontal first into a uint8 intermediate, then vertical; a pass whose size
 *   does not change is skipped.  The tables are the caller's (ingest.pil_bilinear_coeffs), one per distinct (in, out) pair.
 * ch_ingest_images, mode CH_INGEST_CV2_LINEAR: cv2.resize(img, (P, P)) (INTER_LINEAR), the arithmetic of ch_resize_linear_u8: no tables.
 * ch_ingest_labels: N uint8 label maps [h_n,w_n] -> uint8 [N,S,S], nearest: source row min((int)(y * ((double)h / S)), h - 1),
 *   columns likewise (ch_hair_erode's mapping).
 * batch: HOST bytes (8-byte aligned, a multiple of 16 bytes; may be freed on return): N descriptors of CH_INGEST_DESC_BYTES bytes
 *   {uint64 device address of the pixels, int32 H, int32 W, int32 htab, int32 vtab, int64 reserved (the library's)}, then the tables.
 *   htab / vtab: offset of the horizontal / vertical pass's table in int32 units from the start of the batch (a multiple of 4), or -1
 *   where the pass is skipped -- always -1 for mode 1 and for labels, for mode 0 exactly when W == P / H == P.  A table is int32
 *   {in, out, ksize, layout, bounds [out][2] = (first, count), k}: layout 1 (horizontal) stores k as [ksize][out], layout 0 (vertical)
 *   as [out][ksize]; first >= 0, 1 <= count <= ksize, first + count <= in.  Images of one size share their tables.
 * 1 <= N <= 65535, sides 1..CH_INGEST_MAX_SIDE, 1 <= P, S <= CH_INGEST_MAX_OUT; out: device float [N,3,P,P], 16-byte aligned
 *   (labels: uint8 [N,S,S]).  Everything the batch says is checked on the host before the first launch: a refusal names the image.
 * workspace: caller-owned device buffer (256-byte aligned) of ch_ingest_workspace_bytes(batch, batch_bytes, N, P, mode) bytes (labels:
 *   mode CH_INGEST_LABELS; 0 = a batch the entry would refuse): the batch's device copy -- descriptors and tables go up in ONE copy
 *   -- and mode 0's uint8 intermediates [H_n,P,3].  Contents undefined.
 * One copy and at most two launches on `stream` whatever N is: no synchronisation, no allocation, integer accumulation only, no
 *   atomics, no waiting between workgroups; image n of a batch is bit-identical to an N = 1 call. */
#define CH_INGEST_PIL_BILINEAR 0
#define CH_INGEST_CV2_LINEAR 1
#define CH_INGEST_LABELS 2
#define CH_INGEST_DESC_BYTES 32
#define CH_INGEST_MAX_SIDE 32768
#define CH_INGEST_MAX_OUT 4096
size_t ch_ingest_workspace_bytes(const void* batch, size_t batch_bytes, int N, int P, int mode);
int  ch_ingest_images(ch_handle* h, const void* batch, size_t batch_bytes, int N, int P, int mode, const float* lut, float* out,
                      void* workspace, size_t workspace_bytes, ch_stream_t stream);
int  ch_ingest_labels(ch_handle* h, const void* batch, size_t batch_bytes, int N, int S, uint8_t* out, void* workspace,
                      size_t workspace_bytes, ch_stream_t stream);

/* ---- EXIF orientation: N decoded images of ANY sizes -> the upright images, in one launch -------------------------------------------
 * ch_orient_u8 turns uint8 images [H,W,C] (C = 1, 3 or 4) by their EXIF orientation (tag 0x0112) 1..8, as Pillow's
 * ImageOps.exif_transpose does.  With a = the stored image and t = a transposed ([W,H,C]), the upright image is
 *   1: a   2: a[:, ::-1]   3: a[::-1, ::-1]   4: a[::-1]   5: t   6: t[:, ::-1]   7: t[::-1, ::-1]   8: t[::-1]
 * so orientations 5..8 give [W,H,C].  A pure permutation of bytes: exact.
 * batch: HOST bytes (8-byte aligned; may be freed on return): N descriptors of CH_ORIENT_DESC_BYTES bytes {uint64 device address of
 *   the stored pixels, int64 byte offset of the upright pixels in dst, int32 H, int32 W, int32 C, int32 orientation}; H, W, C are the
 *   STORED image's.  1 <= N <= 65535, sides 1..CH_ORIENT_MAX_SIDE.  The destination offsets ascend and the images do not overlap;
 *   neither the offsets nor the source addresses need any alignment.
 * dst: ONE device buffer of dst_bytes bytes that receives every image at its offset.  Everything the batch says is checked on the
 *   host before the launch -- offsets and extents inside dst, C, orientation, H * W * C, no source inside dst -- and a refusal names
 *   the image; the extent of a source is the caller's word.
 * workspace: caller-owned device buffer (256-byte aligned) of ch_orient_workspace_bytes(batch, batch_bytes, N, dst_bytes) bytes (0 = a
 *   batch the entry would refuse): the descriptors' device copy.  Contents undefined.
 * One copy and one launch on `stream` whatever N is: no synchronisation, no allocation, no atomics, no waiting between workgroups;
 *   image n of a batch is bit-identical to an N = 1 call. */
#define CH_ORIENT_DESC_BYTES 32
#define CH_ORIENT_MAX_SIDE 32768
size_t ch_orient_workspace_bytes(const void* batch, size_t batch_bytes, int N, size_t dst_bytes);
int  ch_orient_u8(ch_handle* h, const void* batch, size_t batch_bytes, int N, uint8_t* dst, size_t dst_bytes, void* workspace,
                  size_t workspace_bytes, ch_stream_t stream);

/* ---- Direction search: contact sheets and per-render measurements (shape_branch/script_find_direction.py:55-76,
 *      color_texture_branch/script_find_direction.py:55-74, util/canvas_grid.py:15-31) ------------------------------------------
 * ch_sheet_compose replaces Canvas.process_draw_image for n sources at once: source s goes to cell (cells[2s], cells[2s+1]) =
 *   (row i, column j) of the sheet, whose top-left pixel is y = i * H, x = j * (W + margin) (canvas_grid.py:21,30-31).
 *   canvas uint8 [rows * H, cols * W + margin * (cols - 1), 3] device pointer; cells int32 [n,2] device pointer.  A source whose
 *   cell lies outside the grid is skipped.  The canvas is NOT cleared: pixels of untouched cells and of the margins keep their
 *   bytes (fill it once, e.g. with 255 as Canvas does).  Two sources in one cell of one call: either may win.
 *   kind 0: src float32 [n,3,Hs,Ws] in [-1,1] -> uint8 as the project's to_u8: x * 127.5 rounded to float32, + 127.5 rounded to
 *           float32 (never a fused multiply-add: it gives another byte for ~2 inputs per million), clamped to [0,255], truncated;
 *           NaN -> 0.
 *   kind 1: src uint8 [n,Hs,Ws,3], copied.
 *   kind 2: src uint8 label maps [n,Hs,Ws], coloured by lut uint8 [256,3] (device pointer; hostutil.mask_to_rgb's table of a
 *           draw type: labels 19..254 black, 255 white).  lut is read for kind 2 only.
 *   (Hs, Ws) != (H, W): nearest source pixel, row min((int)(y * ((double)Hs / H)), Hs - 1), columns likewise (cv2 INTER_NEAREST,
 *   as ch_hair_erode).  1 <= n <= 65535, all sizes >= 1, margin >= 0.
 * ch_sweep_stats measures N renders: img as kind 0 ([N,3,H,W] float32) or kind 1 ([N,H,W,3] uint8) above, labels uint8
 *   [N,lh,lw] nearest-mapped to H x W by the same rule, ref int32 [N] (device pointers): ref[n] is the render that render n is
 *   compared with, or < 0 for none; a ref[n] >= N is treated as none.  stats int64 [N,CH_SWEEP_STATS] device pointer,
 *   overwritten.  "Hair" = label 13.  Per render: [0] hair pixels, [1..4] sum x, sum y, sum x^2, sum y^2 over hair pixels (image
 *   coordinates), [5..8] y_min, y_max, x_min, x_max of hair (all -1 without hair), [9..11] sum R, G, B over hair (uint8 values,
 *   after the kind-0 conversion), [12] pixels whose label differs from render ref[n], [13] pixels that are hair in both,
 *   [14] sum |dR| + |dG| + |dB| over pixels that are hair in either, [15] pixels that are hair in either; [12..15] = 0 for
 *   ref[n] < 0.  1 <= N <= 65535, H, W <= 32768, H * W <= 2^30.  Integer sums, minima and maxima combined with integer atomics:
 *   independent of the order of the blocks, so run-to-run deterministic.
 * Both enqueue on `stream` without synchronising or allocating. */
#define CH_SWEEP_STATS 16
int  ch_sheet_compose(ch_handle* h, const void* src, int kind, int n, int Hs, int Ws, const int32_t* cells, const uint8_t* lut,
                      uint8_t* canvas, int rows, int cols, int H, int W, int margin, ch_stream_t stream);
int  ch_sweep_stats(ch_handle* h, const void* img, int kind, const uint8_t* labels, const int32_t* ref, int N, int H, int W, int lh,
                    int lw, int64_t* stats, ch_stream_t stream);

/* ---- PNG encoding on the device: contact sheets, label maps, crops and paste-backs leave as compressed bytes -----------------------
 * ch_png_encode turns N images img uint8 [N,H,W,C] (device pointer; C = 1 grey, 3 RGB, 4 RGBA) into N complete zlib streams
 * (RFC 1950) of their PNG-filtered bytes (RFC 2083 section 6: per row the filter type byte and the filtered row, H * (1 + W * C)
 * bytes): image n's stream starts at out + n * ch_png_zlib_bound(H, W, C) and is sizes[n] bytes long (out uint8, sizes int64 [N]:
 * device pointers).  The caller wraps a stream into signature / IHDR / IDAT / IEND; nothing else is needed for a PNG file.
 *   filter -1: per row the type 0..4 with the smallest sum of |int8(filtered byte)|, the lowest type on a tie, the row above row 0
 *              being zero (libpng's heuristic); filter 0..4: that type for every row.
 *   The filtered stream is cut into chunks of ch_png_chunk_bytes() bytes regardless of rows (the last may be short).  A chunk is
 *   one deflate block of literals and (length 3..258, distance 1) matches under a dynamic Huffman code of its own (lengths limited
 *   to 15 / 7 bits), followed by the empty stored block that realigns to a byte -- or one stored block where that is not smaller
 *   (5 + len bytes).  A run never reaches back across a chunk start.  After the last chunk: an empty final block and the Adler-32.
 *   sizes[n] <= ch_png_zlib_bound = 2 + sum over chunks (len + 10) + 2 + 4.
 *   Integer arithmetic only; atomics are integer add and or: the bytes of an image are the same in every call and in every batch
 *   (they do depend on ch_png_chunk_bytes()).  Pixels decode exactly; the bytes differ from zlib's for the same pixels.
 * workspace: caller-owned device buffer (16-byte aligned) of ch_png_encode_workspace_bytes(N, H, W, C) bytes (0 for arguments the
 * call would reject).  1 <= N <= 65535, 1 <= H, W <= 32768, H * W <= 2^30.  Enqueues three kernels on `stream` without synchronising
 * or allocating.
 * ch_png_encode_dist is the same call with matches at ndist (0..3) further distances dist[0..ndist) (a HOST array read at the call;
 * every value in 2..32767, pairwise distinct): a layout period the caller knows -- the byte pitch of a contact sheet's columns, a
 * tile period, a row stride.  ndist = 0 gives the bytes of ch_png_encode exactly.  With D = (1, dist[0], ...) in that order:
 *   eq_d[i] = (i >= d and x[i] == x[i - d]) over the chunk's bytes x; the maximal true intervals of eq_d are the match intervals of
 *   d.  Position i belongs to the distance whose interval containing i is longest, the earlier in D on a tie; if that interval is
 *   shorter than 3, i is a literal.  A class run -- a maximal run of positions of one distance, R long, from p -- is coded as
 *   floor(R / 258) matches (258, d) at p + 258 k and then the remainder, one match if it is >= 3, else literals.  No match reaches
 *   before its chunk.  Distance symbols and extra bits follow RFC 1951 3.2.5; the used distance symbols (at most 4) get a Huffman
 *   code of their own, one bit where only one is used.
 * The bound, the workspace, the chunk size and the determinism are those of ch_png_encode: the bytes are a pure function of the
 * chunk's bytes and the list. */
int    ch_png_chunk_bytes(void);
size_t ch_png_zlib_bound(int H, int W, int C);
size_t ch_png_encode_workspace_bytes(int N, int H, int W, int C);
int    ch_png_encode(ch_handle* h, const uint8_t* img, int N, int H, int W, int C, int filter, uint8_t* out, int64_t* sizes,
                     void* workspace, size_t workspace_bytes, ch_stream_t stream);
int    ch_png_encode_dist(ch_handle* h, const uint8_t* img, int N, int H, int W, int C, int filter, const int* dist, int ndist,
                          uint8_t* out, int64_t* sizes, void* workspace, size_t workspace_bytes, ch_stream_t stream);

/* ---- PNG decoding on the device: crops and label maps arrive as compressed bytes ------------------------------------------------------
 * ch_png_decode turns N zlib streams into N images img uint8 [N,H,W,C] (device pointer; C = 1 grey, 3 RGB, 4 RGBA; bit depth 8, not
 * interlaced).  Stream n is the bytes streams[offsets[n] .. offsets[n + 1]) (streams uint8, offsets int64 [N + 1]: device pointers): one
 * complete zlib stream (RFC 1950), the concatenated IDAT payloads of one PNG file.  It is inflated (RFC 1951: stored, fixed and dynamic
 * blocks) to H * (1 + W * C) bytes in the workspace, and the five row filters are undone (RFC 2083 section 6; Average is
 * floor((a + b) / 2), Paeth with the tie order a, b, c).  The container (signature, chunks, CRC-32) is the caller's: pngdec.parse_png.
 * status[n] (int32 [N], device): CH_PNG_DEC_OK, or
 *   BAD_HEADER    CM != 8, CINFO > 7, FCHECK fails, or FDICT is set
 *   BAD_BLOCK     BTYPE 3, or a stored block's LEN != ~NLEN
 *   BAD_CODE      HLIT > 286 or HDIST > 30; repeat code 16 without a predecessor or a repeat past HLIT + HDIST; an over-subscribed
 *                 code; an incomplete code other than one single code of length 1 or a distance code without any code; no
 *                 end-of-block code
 *   BAD_SYMBOL    length symbol 286 / 287, distance symbol 30 / 31, or bits that are no code of an incomplete code (a distance
 *                 symbol wanted from an empty distance code)
 *   BAD_DISTANCE  a distance beyond the bytes produced so far (or beyond 32768)
 *   INPUT_END     the stream ends inside a block or before the end of the Adler-32
 *   SIZE          the stream inflates to more or fewer than H * (1 + W * C) bytes
 *   ADLER         Adler-32 mismatch
 *   BAD_FILTER    a row's filter type byte is greater than 4
 * and the pixels of that image are unspecified.  What is accepted is what stock zlib's inflate accepts: CINFO is not enforced as a
 * window size, bytes behind the Adler-32 are ignored, an empty stored block may stand anywhere.
 * For every byte sequence: the work for image n reads no stream byte outside [offsets[n], offsets[n + 1]), writes nothing outside image
 * n's slice of img, of status and of the workspace, and terminates.
 * workspace: caller-owned device buffer (16-byte aligned) of ch_png_decode_workspace_bytes(N, H, W, C) bytes (0 for arguments the call
 * would reject).  1 <= N <= 65535, 1 <= H, W <= 32768, H * W <= 2^30.  Enqueues two kernels on `stream` without synchronising or
 * allocating.  Integer arithmetic only, no atomics: image n is the same in every batch and every call. */
#define CH_PNG_DEC_OK 0
#define CH_PNG_DEC_BAD_HEADER 1
#define CH_PNG_DEC_BAD_BLOCK 2
#define CH_PNG_DEC_BAD_CODE 3
#define CH_PNG_DEC_BAD_SYMBOL 4
#define CH_PNG_DEC_BAD_DISTANCE 5
#define CH_PNG_DEC_INPUT_END 6
#define CH_PNG_DEC_SIZE 7
#define CH_PNG_DEC_ADLER 8
#define CH_PNG_DEC_BAD_FILTER 9
size_t ch_png_decode_workspace_bytes(int N, int H, int W, int C);
int    ch_png_decode(ch_handle* h, const uint8_t* streams, const int64_t* offsets, int N, int H, int W, int C, uint8_t* img,
                     int32_t* status, void* workspace, size_t workspace_bytes, ch_stream_t stream);

/* ---- JPEG encoding on the device: crops and paste-backs of .jpg photos leave as compressed bytes -----------------------------------
 * ch_jpeg_encode turns N images img uint8 [N,H,W,C] (device pointer; C = 1 grey, 3 interleaved RGB; RGBA is refused) into N
 * entropy-coded scans of baseline JPEG (ITU-T T.81, sequential DCT, Huffman): the bytes between the SOS header and the EOI marker,
 * byte-stuffed and padded.  Image n's scan starts at out + n * ch_jpeg_scan_bound(H, W, C, subsampling) and is sizes[n] bytes long
 * (out uint8, sizes int64 [N]: device pointers).  The caller writes the markers around it (ctrlhair_amd.jpegenc.wrap_jpeg).
 *   quality      1..100, libjpeg's scaling of the Annex K quantisation tables
 *   subsampling  0: 4:4:4;  2: 4:2:0 (Pillow's numbering); ignored for C = 1
 *   No restart markers, no progressive mode, the Annex K.3 Huffman tables (libjpeg without optimize_coding).
 * The arithmetic is libjpeg's, all of it integer -- 16-bit fixed-point RGB -> YCbCr, 2x2 chroma averaging with the alternating bias,
 * its edge replication and dummy blocks, the slow-integer forward DCT and its quantiser -- so the scan is the one libjpeg and
 * libjpeg-turbo (Pillow) write for the same pixels and parameters, byte for byte, and is the same in every call and batch position.
 * ch_jpeg_scan_bound: a block codes into at most 20 + 63 * 26 = 1658 bits (a category-11 DC difference behind a 9-bit code, 63 AC terms
 *   of size 10 behind 16-bit codes); the last byte is padded; every byte may be 0xFF and then takes a 0x00 behind it:
 *   bound = 2 * ceil(blocks * 1658 / 8) + 2, with blocks = the blocks of the scan, dummy luma blocks of 4:2:0 included.
 * workspace: caller-owned device buffer (16-byte aligned) of ch_jpeg_encode_workspace_bytes(N, H, W, C, subsampling) bytes.
 * Limits: sides 1..32768, H * W <= 2^30, N <= 65535.  Both size functions return 0 for arguments the call would refuse. */
size_t ch_jpeg_scan_bound(int H, int W, int C, int subsampling);
size_t ch_jpeg_encode_workspace_bytes(int N, int H, int W, int C, int subsampling);
int    ch_jpeg_encode(ch_handle* h, const uint8_t* img, int N, int H, int W, int C, int quality, int subsampling, uint8_t* out,
                      int64_t* sizes, void* workspace, size_t workspace_bytes, ch_stream_t stream);

/* ---- JPEG decoding on the device: the photos and edits of the crop and paste-back jobs arrive as compressed bytes -------------------
 * ch_jpeg_decode turns N entropy-coded scans of baseline JPEG (SOF0: sequential DCT, Huffman, 8 bits, one scan holding all components,
 * no restart interval) into N images img uint8 [N,H,W,C] (device pointer; C = 1 grey, 3 RGB from YCbCr).  The images of one call share
 * H, W, C and sampling: 0 = 4:4:4 (required for C = 1), 1 = 4:2:2, 2 = 4:2:0 (Pillow's numbering; luma 1x1, 2x1, 2x2, chroma 1x1).
 * Stream n is the bytes streams[offsets[n] .. offsets[n + 1]) between the SOS header and the EOI marker, stuffed (streams uint8, offsets
 * int64 [N + 1]: device pointers).  tables (uint8, device): per image a block of CH_JPEG_DEC_TABLE_BYTES bytes: at 64 * c the 8-bit
 * quantiser of component c in natural (row-major) order; at 192 + 272 * (2 * c + k) the DC (k = 0) and AC (k = 1) Huffman table of
 * component c as BITS[16] and HUFFVAL[256] (any tables, not only Annex K).  The markers are the caller's: jpegdec.parse_jpeg.
 * The Huffman decode is parallel WITHIN a scan: subsequences of 128 bytes, one lane each, start from the guess "a block begins here",
 * hand their exit state to the next and repeat until nothing changes (Huffman streams re-synchronise); chunks of 64 subsequences hand
 * over between `rounds` kernel launches (0: the default, CH_JPEG_DEC_DEFAULT_ROUNDS; at most 64).  A stream whose chain of states is
 * not whole after them is NOT_SYNCED, never wrong pixels.  The arithmetic behind it is libjpeg's, all of it integer -- the
 * slow-integer inverse DCT, fancy upsampling (h2v1, h2v2; replication when the chroma plane is at most 2 samples wide), 16-bit
 * fixed-point YCbCr -> RGB -- so for status 0 the pixels are libjpeg's and libjpeg-turbo's (Pillow's), byte for byte.
 * status[n] (int32 [N], device): CH_JPEG_DEC_OK, or
 *   BAD_CODE      bits that are no code of the table in force, or a DC symbol above 15
 *   BAD_INDEX     a run that carries the coefficient index past 63
 *   INPUT_END     the stream ends before the last block (or is empty)
 *   BLOCKS        the stream holds more symbols than the image's blocks take
 *   NOT_SYNCED    see above: decode it elsewhere or call again with more rounds
 *   TOO_LONG      more than min(512 * blocks, 2^28 - 1) bytes: longer than any valid scan (64 symbols of 31 bits per block, all stuffed)
 *   MARKER        a 0xFF followed by a byte other than 0x00 inside the stream
 *   RESTART       ch_jpeg_decode_rst only: the restart markers are not where the interval puts them (see below)
 *   RANGE         a dequantised coefficient or a first-pass value beyond +-8191, or a sample before the range limit outside -512..511:
 *                 values no sane file holds, at which libjpeg's C code, its SIMD code and 32-bit arithmetic part ways
 * and the pixels of that image are unspecified.  For every byte sequence: the work for image n reads no stream byte outside
 * [offsets[n], offsets[n + 1]), writes nothing outside image n's slice of img, of status and of the workspace, and terminates.
 * workspace: caller-owned device buffer (16-byte aligned) of ch_jpeg_decode_workspace_bytes(N, H, W, C, sampling) bytes (0 for arguments
 * the call would reject).  1 <= N <= 65535, 1 <= H, W <= 32768, H * W <= 2^30.  Enqueues on `stream` without synchronising or
 * allocating.  No atomics between workgroups, no result read from the launch that writes it: image n is the same in every batch and
 * every call.
 *
 * ch_jpeg_decode_rst is ch_jpeg_decode for scans with restart intervals: restart (uint32 [N], device) holds per stream the Ri of its DRI
 * segment, MCUs per interval, 0 = none; the stream then keeps its RSTm markers (0xFF 0xD0..0xD7).  ch_jpeg_decode is the all-zero case,
 * with byte-identical results, and the workspace is the same (ch_jpeg_decode_workspace_bytes).  For stream n with Ri > 0:
 *   1. An RSTm is legal in one place only: directly after the block that completes MCU number k * Ri (k >= 1, not after the last MCU),
 *      behind at most 7 pad bits, which are discarded unread as libjpeg does, with m == (k - 1) mod 8.  After it the decoder is at the
 *      byte behind the marker, block 0 of an MCU, zigzag index 0.
 *   2. RESTART: a marker missing at such a boundary, a marker anywhere else, a wrong m, two markers back to back; whole extra bytes or a
 *      fill 0xFF before a marker where the decoder gets as far as the marker (bytes that are no codes end it earlier, with BAD_CODE or
 *      BAD_INDEX; a fill 0xFF that decodes is MARKER by rule 3).  The pixels are unspecified, as for every non-zero status.
 *   3. 0xFF followed by anything other than 0x00 or 0xD0..0xD7 stays MARKER.
 *   4. The DC predictors are 0 at the start of every interval.
 *   5. Ri at or above the image's MCU count expects no marker: the stream decodes as by ch_jpeg_decode (a marker in it is MARKER).
 *   6. Every guarantee above carries over word for word: for every byte sequence and every Ri the work for image n reads nothing outside
 *      its stream, writes nothing outside its slices and terminates; no atomics between workgroups; image n is the same in every batch
 *      and every call; a stream is NOT_SYNCED, never wrong pixels.
 * A lane of the entropy stage whose next symbol does not fit before a marker continues from the state behind it whatever state it
 * arrived in, so wrong guesses converge at the first marker; whether a jump was legal is judged on the true chain only, where the block
 * ordinals are known.  A lane cannot drop the padding by count as libjpeg does: padding that reads as a whole symbol (only with a
 * Huffman table that assigns the all-ones code, which T.81 forbids) is RESTART.  libjpeg's resynchronisation of damaged intervals is
 * not restated: those streams are RESTART, decode them elsewhere. */
#define CH_JPEG_DEC_OK 0
#define CH_JPEG_DEC_BAD_CODE 1
#define CH_JPEG_DEC_BAD_INDEX 2
#define CH_JPEG_DEC_INPUT_END 3
#define CH_JPEG_DEC_BLOCKS 4
#define CH_JPEG_DEC_NOT_SYNCED 5
#define CH_JPEG_DEC_TOO_LONG 6
#define CH_JPEG_DEC_MARKER 7
#define CH_JPEG_DEC_RANGE 8
#define CH_JPEG_DEC_RESTART 9
#define CH_JPEG_DEC_TABLE_BYTES 2048
#define CH_JPEG_DEC_DEFAULT_ROUNDS 8
size_t ch_jpeg_decode_workspace_bytes(int N, int H, int W, int C, int sampling);
int    ch_jpeg_decode(ch_handle* h, const uint8_t* streams, const int64_t* offsets, const uint8_t* tables, int N, int H, int W, int C,
                      int sampling, int rounds, uint8_t* img, int32_t* status, void* workspace, size_t workspace_bytes,
                      ch_stream_t stream);
int    ch_jpeg_decode_rst(ch_handle* h, const uint8_t* streams, const int64_t* offsets, const uint8_t* tables, const uint32_t* restart, int N,
                          int H, int W, int C, int sampling, int rounds, uint8_t* img, int32_t* status, void* workspace,
                          size_t workspace_bytes, ch_stream_t stream);

/* ---- Hair-shape transfer: the mask warp of wrap_codes/mask_adaptor.py:87-143 (hair_mask_transfer_wrap), batched -------------
 * For each of B pairs: the donor's hair mask (hair_labels == 13) is padded to the 672 x 672 canvas (80-px border, hair on an image
 * edge extended 10 px, mask_adaptor.py:119-131), the pair's triangle mesh is deformed as rigidly as possible (libigl's per-element
 * ARAP energy for 2-D triangles, cotangent weights, CH_WARP_OUTER_ITERS local/global iterations from U = V as my_arap.cpp:181-187;
 * the global step is a Jacobi-preconditioned conjugate-gradient solve, warm-started, run until ||r|| <= CH_WARP_REL_TOL * ||rhs|| or
 * CH_WARP_MAX_CG iterations), the deformed mesh is drawn with per-vertex colour V / 671 (mesh_core.cpp render_colors_core: float32
 * barycentrics in its operation order, first covering triangle in face order wins, uncovered = -1), the canvas edge is fixed
 * (triangle_wrap_hair.py:77-85), the padded mask is sampled as cv2.remap(INTER_LINEAR, constant border 0) does and truncated to
 * uint8, the border is cropped and naive_transfer composes: warped hair -> 13, the face's own hair -> 255, else face_labels.
 *   hair_labels, face_labels, labels_out: uint8 [B,512,512] (CelebAMask-HQ ids).
 *   Packed meshes: V float [sum n_v, 2] rest positions on the canvas (x, y); F int32 [sum n_f, 3] vertex indices LOCAL to the
 *   pair; b int32 [sum n_b] constrained vertices (local), bc float [sum n_b, 2] their targets.  desc: HOST array int32 [B,6] =
 *   {v_off, n_v, f_off, n_f, b_off, n_b} per pair (offsets in vertices / triangles / constraints); 3 <= n_v <= CH_WARP_MAX_V,
 *   1 <= n_f <= CH_WARP_MAX_F, checked here.  A mesh whose device-side indices are out of range is rendered undeformed.
 *   U_in (optional) float [sum n_v, 2]: deformed positions given by the caller -- the ARAP solve is skipped (b, bc may be null).
 *   uv_out (optional) float [B,672,672,2]: the UV image after the edge fix.  U_out (optional) float [sum n_v, 2].
 *   workspace: caller-owned device buffer of ch_mask_warp_workspace_bytes(B) bytes (256-byte aligned), contents undefined.
 *   The descriptors are copied to its head as kernel arguments (desc may be freed on return); the ARAP solve and the render are
 *   each ONE launch for all B pairs (one workgroup per pair / per 16x16 tile and pair).
 * Everything is enqueued on `stream`; no synchronisation, no allocation.  No atomics on floating-point data and fixed reduction
 * trees: pair i of a batch is bit-identical to a B = 1 call on the same inputs. */
#define CH_WARP_MAX_V 2048
#define CH_WARP_MAX_F 4096
#define CH_WARP_OUTER_ITERS 100
#define CH_WARP_MAX_CG 200
#define CH_WARP_REL_TOL 1e-6f
size_t ch_mask_warp_workspace_bytes(int B);
int  ch_mask_warp_batch(ch_handle* h, const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int32_t* F,
                        const int32_t* b, const float* bc, const int32_t* desc, const float* U_in, uint8_t* labels_out,
                        float* uv_out, float* U_out, void* workspace, size_t workspace_bytes, int B, ch_stream_t stream);
/* ch_mask_warp_batch_dev: the same call with desc in DEVICE memory (int32 [B,6]), so a mesh made on the device (ch_delaunay_batch)
 * never visits the host.  The descriptors are validated by the kernel that copies them to the workspace: offsets >= 0,
 * 3 <= n_v <= CH_WARP_MAX_V, 1 <= n_f <= CH_WARP_MAX_F, 0 <= n_b <= CH_WARP_MAX_V.  A pair that fails is rendered undeformed (the
 * identity map: UV = pixel / 671 before the edge fix), its U_out rows are not written; the other pairs are not affected.  With
 * equal descriptors the results are those of ch_mask_warp_batch, byte for byte. */
int  ch_mask_warp_batch_dev(ch_handle* h, const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int32_t* F,
                            const int32_t* b, const float* bc, const int32_t* desc, const float* U_in, uint8_t* labels_out,
                            float* uv_out, float* U_out, void* workspace, size_t workspace_bytes, int B, ch_stream_t stream);

/* ---- Meshing for the warp: exact Delaunay triangulation of B planar point sets in one launch ---------------------------------
 * V float [sum n_v, 2] device, packed; v_desc: HOST int32 [B,2] = {v_off, n_v} per set (copied as kernel arguments, may be freed on
 * return).  F int32 [B, CH_WARP_MAX_F, 3], n_f int32 [B], status int32 [B]: device.  One workgroup per set, points in LDS, one lane
 * per point: nearest neighbour, then a walk around the point that finds each triangle's apex by a scan of the set.
 * Exactness domain: every coordinate is a float32 in [0, 1024) that is a multiple of 2^-20 (what warping.build_points_batch makes),
 *   i.e. a 30-bit integer on that grid.  Orientation fits int64 and the incircle determinant 124 bits; both are evaluated in
 *   float64 first and again in integers (__int128) whenever the float64 value is within its error bound, so the result is exactly
 *   a Delaunay triangulation of the convex hull: no point strictly inside any circumcircle, every triangle of positive area (no
 *   zero-area triangles along collinear hull points), 2 n - 2 - h triangles for h points on the hull boundary.
 * Ties: k >= 4 points on one empty circle are fanned from the smallest index among them -- a rule of the co-circular set alone, so
 *   the result is a manifold triangulation.
 * Canonical form: rows counter-clockwise in (x, y), smallest index first, in lexicographic order, no duplicates, indices local.
 * status[i]: CH_DELAUNAY_OK, or BAD_COUNT (n_v outside 3..CH_WARP_MAX_V), OFF_GRID (a coordinate outside the domain, NaN included),
 *   DUPLICATE (two equal points), COLLINEAR (all points on one line), INTERNAL (inconsistency, never seen); then n_f[i] = 0 and
 *   F's rows of the set are not written.  Nothing outside the set's own slots is ever written.
 * workspace: ch_delaunay_workspace_bytes(B) bytes, 256-byte aligned: the descriptors, then per set two uint64 counters (incircle
 *   tests evaluated, and how many of them went to the integer evaluation) at offset ((8 B + 255) / 256) * 256.
 * Enqueued on `stream`, no synchronisation, no allocation, no waiting between workgroups, no floating-point atomics: set i of a
 * batch is bit-identical to a B = 1 call. */
#define CH_DELAUNAY_OK 0
#define CH_DELAUNAY_BAD_COUNT 1
#define CH_DELAUNAY_OFF_GRID 2
#define CH_DELAUNAY_DUPLICATE 3
#define CH_DELAUNAY_COLLINEAR 4
#define CH_DELAUNAY_INTERNAL 5
size_t ch_delaunay_workspace_bytes(int B);
int  ch_delaunay_batch(ch_handle* h, const float* V, const int32_t* v_desc, int32_t* F, int32_t* n_f, int32_t* status,
                       void* workspace, size_t workspace_bytes, int B, ch_stream_t stream);

/* ---- Face alignment: external_code/crop.py:20-107 (recreate_aligned_images) for one photo -------------------------------------
 * The geometry (oriented quad, shrink factor, crop box, pad widths, blur, Pillow's quad coefficients) is a host plan
 * (ctrlhair_amd/alignment.py align_plan); the pixel work is here, bit-exact against Pillow 8-bit / numpy / scipy:
 * ch_resample_lanczos_u8 replaces Image.resize((Wd, Hd), LANCZOS) of an 8-bit image: src uint8 [Hs,Ws,C], dst uint8 [Hd,Wd,C]
 *   device pointers, 1 <= C <= 4.  Coefficient tables are built on the host (libm sin, double), normalised and rounded to 22
 *   fractional bits; horizontal pass into a uint8 intermediate, then the vertical pass; a pass whose size does not change is skipped.
 * ch_quad_warp_resample_u8 replaces Image.transform((T, T), QUAD, quad, BILINEAR) followed by resize((S, S), LANCZOS) of an RGB
 *   image: coef = the 8 bilinear-quad coefficients Pillow derives from the corners (host doubles); src uint8 [Hs,Ws,3], dst uint8
 *   [S,S,3].  One workgroup evaluates one row of the T x T grid in float64 into LDS and filters it horizontally at once: only the
 *   [T,S,3] intermediate is written.  S == T writes the transform itself.  S <= T <= CH_ALIGN_MAX_TRANSFORM.
 * ch_align_pad_feather_u8 replaces crop.py:83-92: np.pad(reflect) to float32, scipy gaussian_filter with the caller's kernel
 *   (gauss_w: HOST doubles [2 * radius + 1], symmetric; reflect borders, axis 0 then 1, double accumulation in correlate1d's order,
 *   float32 between passes), the feather mask and both blends as numpy evaluates them, np.median by an exact radix select,
 *   rint / clip / uint8.  pads: HOST int32 {left, top, right, bottom}, all >= 1; src uint8 [Hs,Ws,3], dst uint8
 *   [Hs+top+bottom, Ws+left+right, 3].
 * ch_face_align runs a whole plan on one stream: optional Lanczos shrink, crop (an offset and a stride), optional padding branch,
 *   quad warp + reduction.  src uint8 [H,W,3], dst uint8 [S,S,3].  plan: HOST doubles [CH_ALIGN_PLAN_LEN] =
 *   {shrink, resized W, resized H (= W / shrink, H / shrink rounded half to even when shrink > 1, else W, H), crop x0, y0, x1, y1, pad flag, pad left, top, right, bottom, quad coefficients a0..a7,
 *    transform_size, output_size, 0, 0}; gauss_w / radius as above (ignored without the pad flag).
 * workspace: caller-owned device buffer (256-byte aligned) of at least the matching ..._workspace_bytes query, contents
 *   undefined.  Everything is enqueued on `stream`: no device synchronisation, no allocation; host arrays may be freed on return.
 *   All results are integer arithmetic or single IEEE operations in a fixed order: run-to-run deterministic. */
#define CH_ALIGN_PLAN_LEN 24
#define CH_ALIGN_MAX_TRANSFORM 16384
size_t ch_resample_lanczos_workspace_bytes(int Hs, int Ws, int C, int Hd, int Wd);
int  ch_resample_lanczos_u8(ch_handle* h, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst, int Hd, int Wd, void* workspace,
                            size_t workspace_bytes, ch_stream_t stream);
size_t ch_quad_warp_workspace_bytes(int T, int S);
int  ch_quad_warp_resample_u8(ch_handle* h, const uint8_t* src, int Hs, int Ws, const double* coef, int T, int S, uint8_t* dst,
                              void* workspace, size_t workspace_bytes, ch_stream_t stream);
size_t ch_align_pad_workspace_bytes(int Hs, int Ws, const int32_t* pads, int radius);
int  ch_align_pad_feather_u8(ch_handle* h, const uint8_t* src, int Hs, int Ws, const int32_t* pads, const double* gauss_w, int radius,
                             uint8_t* dst, void* workspace, size_t workspace_bytes, ch_stream_t stream);
size_t ch_face_align_workspace_bytes(int H, int W, const double* plan, int radius);
int  ch_face_align(ch_handle* h, const uint8_t* src, int H, int W, const double* plan, const double* gauss_w, int radius,
                   uint8_t* dst, void* workspace, size_t workspace_bytes, ch_stream_t stream);

/* ---- Paste-back: N edited crops of one alignment composited into the photo they came from ------------------------------------
 * The inverse geometry is a host plan (ctrlhair_amd/alignment.py unalign_plan / pack_unalign).  plan: HOST doubles
 *   [CH_UNALIGN_PLAN_LEN] = {A00, A01, A02, A10, A11, A12, bbox x0, y0, x1, y1, scale, output_size S, 0, 0, 0, 0}: A maps the photo
 *   pixel centre (X + 0.5, Y + 0.5, 1) to crop coordinates (x, y) (pixel i covers [i, i + 1)), evaluated in float64 as
 *   (A00 (X + 0.5) + A01 (Y + 0.5)) + A02 without fused multiply-adds; bbox = the quad's bounding box inside the photo, not empty;
 *   scale = s, crop pixels per photo pixel, 0 < s <= CH_UNALIGN_MAX_SCALE.
 * photo uint8 [H,W,3], edits uint8 [N,S,S,3], weight uint8 [S,S] or NULL, out uint8 [N,H,W,3] (must not overlap photo): device.
 * Inside bbox, per edit: alpha = clamp(min(x, S - x, y, S - y) / feather_px, 0, 1) (feather_px <= 0: 1 inside the quad, 0 outside),
 *   times weight / 255 sampled bilinearly at (x, y) (centres at i + 0.5, edges clamped) when weight is given; e = the edit resampled
 *   with Lanczos-3 at filter scale fs = max(1, s): taps |i + 0.5 - x| < 3 fs and likewise in y, weight L((i + 0.5 - x) / fs)
 *   L((j + 0.5 - y) / fs), taps outside [0, S) dropped and the rest renormalised; out = clamp(floor(alpha e + (1 - alpha) p + 0.5),
 *   0, 255) in float32.  alpha == 0 and everything outside bbox: the photo's bytes.
 * Two launches on `stream` (copy outside bbox, resample + composite inside) for all N; no workspace, no synchronisation, no
 *   atomics: image n of a batch is bit-identical to an N = 1 call. */
#define CH_UNALIGN_PLAN_LEN 16
#define CH_UNALIGN_MAX_SCALE 16
int  ch_face_unalign(ch_handle* h, const uint8_t* photo, int H, int W, const uint8_t* edits, int N, const uint8_t* weight,
                     const double* plan, double feather_px, uint8_t* out, ch_stream_t stream);

/* ---- Paste-back with an edge-aware matte: the weight map refined by a colour guided filter of the photo --------------------------
 * He, Sun, Tang, "Guided Image Filtering", colour guide: the weight is fitted locally as a linear function of the photo's RGB, so
 * the matte follows the photo's edges instead of the staircase of an up-sampled label map.  plan, photo, edits, out, feather_px,
 * the coordinates (x, y) and the Lanczos resample e are exactly those of ch_face_unalign.  weight uint8 [S,S] is required.
 * The domain D is the plan's bbox, bw x bh pixels.  1 <= radius <= CH_MATTE_MAX_RADIUS (at r = 64 the sum of I I over a window is at
 * most 255^2 129^2 ~ 1.08e9, which fits int32); eps > 0 and finite, in units of a guide scaled to [0, 1].  Per pixel (X, Y) of D:
 *   1. p8 = weight[clamp(floor(y))][clamp(floor(x))] when min(x, S - x, y, S - y) > 0, else 0 (nearest: an exact integer).
 *   2. Over the window [X - r, X + r] x [Y - r, Y + r] clipped to D, n pixels: the 13 integer sums of p, I_c (3), I_c p (3) and
 *      I_c I_d (6), I = the photo's bytes.  All exact.
 *   3. n sum(I_c p) - sum(I_c) sum(p) and n sum(I_c I_d) - sum(I_c) sum(I_d) as exact int64, converted to float64 and divided by
 *      n^2 255^2; (cov + eps Id) a = cov_Ip solved in float64 by LDL^T (Cholesky without square roots; the matrix is symmetric
 *      positive definite); b = sum(p) / (255 n) - a . sum(I) / (255 n).  a (3 values) and b are rounded to float32.
 *   4. q = mean_w(a) . I / 255 + mean_w(b) over the same clipped window, the sums accumulated in float64; m = clamp(q, 0, 1) as
 *      float32.
 *   5. alpha = m * ramp in float32, ramp = clamp(min(x, S - x, y, S - y) / feather_px, 0, 1) (feather_px <= 0: 1 inside the quad,
 *      0 outside): alpha is 0 outside the quad whatever the filter leaks.  out = clamp(floor(alpha e + (1 - alpha) p + 0.5), 0, 255)
 *      as in ch_face_unalign; alpha == 0 and everything outside D: the photo's bytes.
 * The matte is computed once and shared by all N edits; image n of a batch is bit-identical to an N = 1 call.
 * alpha_out: optional device float [bh,bw], receives alpha over D.
 * workspace: caller-owned device buffer (256-byte aligned) of ch_face_unalign_matte_workspace_bytes(H, W, plan, radius) bytes
 *   (0 = bad argument; 21 bytes per pixel of D), contents undefined.  Five launches on `stream`: no synchronisation, no
 *   allocation, no atomics, no waiting between workgroups; the cost does not grow with radius beyond halo and warm-up rows. */
#define CH_MATTE_MAX_RADIUS 64
size_t ch_face_unalign_matte_workspace_bytes(int H, int W, const double* plan, int radius);
int  ch_face_unalign_matte(ch_handle* h, const uint8_t* photo, int H, int W, const uint8_t* edits, int N, const uint8_t* weight,
                           const double* plan, double feather_px, int radius, double eps, uint8_t* out, float* alpha_out,
                           void* workspace, size_t workspace_bytes, ch_stream_t stream);

/* ---- Median style codes: sean_codes/get_mean_code.py for R segments (the 19 regions) in one call -----------------------------
 * For each segment the medoid is the row whose summed Euclidean distance to the segment's rows is smallest.  The reference builds
 * the n x n matrix from the Gram identity in float32; here the matrix is never stored and the arithmetic is fixed as follows:
 *   d_ij^2 = sum_k (x_ik - x_jk)^2 in float32, the difference formed before squaring (fused multiply-add allowed, summed in
 *            ascending k; no Gram identity anywhere), d_ij = sqrtf(d_ij^2), so d_ii = 0 exactly;
 *   S_i    = sum_j d_ij in float64;  index = the FIRST i attaining min S_i (numpy argmin);
 *   mean   = float64 column sums / n, rounded once to float32.
 * codes: device float [total, dim], the rows of segment r are seg_offsets[r] .. seg_offsets[r+1]-1 (16-byte aligned; dim a multiple
 *   of 4, 4 <= dim <= CH_MEDOID_MAX_DIM).  seg_offsets: HOST int64 [R+1], ascending from 0; 1 <= R <= CH_MEDOID_MAX_SEGMENTS; a
 *   segment has at most CH_MEDOID_MAX_ROWS rows.
 * n_split: each 128-row tile walks its 128-column tiles in ascending order; the column range is cut into n_split contiguous parts
 *   (clamped to the number of tiles) run by different workgroups, whose float64 partial sums are added in ascending order.
 *   0 = auto, a function of the segment's row count alone.
 * index: device int32 [R], row within the segment, -1 for an empty segment.  sums (optional): device double [total].
 * mean: device float [R, dim], zeros for an empty segment.
 * workspace: caller-owned device buffer (256-byte aligned) of ch_style_medoid_workspace_bytes(seg_offsets, R, dim, n_split) bytes
 *   (0 = bad argument), contents undefined.  Everything is enqueued on `stream`: no synchronisation, no allocation; seg_offsets
 *   may be freed on return.  No floating-point atomics and fixed reduction trees: two runs are bit-identical, and a segment's
 *   sums have the same bits whether it is run alone or among others (same n_split). */
#define CH_MEDOID_MAX_DIM 65536
#define CH_MEDOID_MAX_SEGMENTS 65535
#define CH_MEDOID_MAX_ROWS (1 << 30)
size_t ch_style_medoid_workspace_bytes(const int64_t* seg_offsets, int R, int dim, int n_split);
int  ch_style_medoid(ch_handle* h, const float* codes, const int64_t* seg_offsets, int R, int dim, int n_split, int32_t* index,
                     double* sums, float* mean, void* workspace, size_t workspace_bytes, ch_stream_t stream);

/* Test hook: after the next ch_sean_generate calls, the activation produced at stage `name` ("fc", "<block>",
 * "<block>.ace_0" = tensor before leaky_relu, "<block>.conv_0", "<block>.shortcut") is also copied
 * (device-to-device, same stream) to `dev_ptr` (caller-sized: [B,C,r,r] floats).  dev_ptr NULL removes the tap. */
int  ch_sean_set_tap(ch_handle* h, const char* name, float* dev_ptr);

/* Diagnostic hook of the f16x3 / f16 paths (ctrlhair_amd/csrc/sh16.h): data-dependent activations are stored as f16 hi/lo
 * pairs with a power-of-two scale; each producer records the maximum of |value * 8| over its tensor and rewrites the
 * tensor with a corrected scale when that maximum left the window [0.5, 65504].  Copies to host_out[0..n) the maxima
 * recorded by the last ch_sean_generate batch chunk: entry 2i = output of ACE layer i (execution order), 2i+1 = its style
 * projections; 0 = not written.  Synchronises the device (not for the hot path). */
int  ch_sean_scale_report(ch_handle* h, float* host_out, int n);

/* Label memo (option "sean.label_memo"), a query: calls << 32 | hits -- how many chunks of ch_sean_generate went through the memo's decision so
 * far (`calls`) and how many of them found the label maps of the chunk before (`hits`); 0 on a handle without the memo; -1 without a
 * finalised SEAN model or when the read fails (ch_last_error).  Synchronises the device (tests, tools). */
long long ch_sean_label_memo_stats(ch_handle* h);
/* SPADE memo (option "sean.spade_memo"), the same kind of query: stores << 32 | loads -- how many of those chunks stored the accumulators of
 * the styled F(4x4)-route ACEs and how many ran from the stored ones; 0 on a handle without it. */
long long ch_sean_spade_memo_stats(ch_handle* h);
/* Code memo (option "sean.code_memo"), the same kind of query: calls << 32 | hits -- how many chunks went through the code memo's decision
 * and how many of them found the style codes of the chunk before; 0 on a handle without it. */
long long ch_sean_code_memo_stats(ch_handle* h);

/* Profiling hook (tools/ only): copies the first `bytes` of the generator's split-K scratch to host memory; with option
 * "sean.dbg" bit 256 the wave-specialised conv kernel leaves per-tile cycle stamps there.  Synchronises the device. */
int  ch_sean_debug_read(ch_handle* h, void* host_out, size_t bytes);

/* Roofline helper: the matrix-core issue rate this device sustains on an MFMA-only loop with non-trivial operands (no memory
 * traffic; ~ms_target ms; synchronises the device).  kind 0 = v_mfma_f32_32x32x2_f32, 1 = v_mfma_f32_32x32x16_f16.  Reported by
 * bench.py next to the spec peak (the spec figure assumes the 2.4 GHz boost clock). */
int  ch_mfma_peak(ch_handle* h, int kind, int ms_target, double* tflops);

/* Kernel-level timing hook for bench.py / roofline: when enabled, ch_sean_generate brackets every MFMA conv launch
 * with hipEvents on `stream`.  ch_profile_read synchronises those events and returns, for launches of `kind`
 * (0 = plain conv, 1 = SPADE conv with fused ACE epilogue, 2 = style-LUT GEMM, 3 = interior pass of a sparse ACE, <0 = all), their count, summed
 * duration (ms) and summed algorithmic flops / bytes.  A read with kind < 0 also clears the records. */
int  ch_profile_enable(ch_handle* h, int on);
int  ch_profile_read(ch_handle* h, int kind, int* launches, double* total_ms, double* flops, double* bytes);
/* As ch_profile_read; additionally `flops_executed`: the FLOPs the matrix cores actually ran.  They differ from `flops`
 * (the dense evaluation of every layer) for ACE launches served by the exact SPADE-interior reduction (option "sean.sparse",
 * ctrlhair_amd/csrc/ace_sparse.h): gamma/beta of SPADE.forward (/root/reference/sean_codes/models/networks/
 * normalization.py:249-257) depend on the 5x5 label neighbourhood only, so pixels whose neighbourhood is uniform take
 * per-label constants and only the compacted boundary pixels go through the conv. */
int  ch_profile_read_ex(ch_handle* h, int kind, int* launches, double* total_ms, double* flops, double* flops_executed,
                        double* bytes);

#ifdef __cplusplus
}
#endif
#endif
