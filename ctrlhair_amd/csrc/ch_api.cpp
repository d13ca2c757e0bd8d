// ch_api.cpp -- the C ABI of libctrlhair_hip.so (see include/ctrlhair_hip.h for the contract).
#include "../../include/ctrlhair_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>

#include "aux_models.h"
#include "sean_model.h"
#include "kernels.h"
#include "ingest_batch.h"
#include "orient_batch.h"
#include "jpeg_entropy_core.h"
#include "png_inflate_core.h"

struct ch_handle {
    int device = 0;
    std::string err;
    chk::TensorStore tensors[4];
    chk::SeanModel sean;
    bool sean_ready = false;
    chk::ShapeModel shape;
    chk::ColorModel color;
    chk::BiSeNetModel bisenet;
    void* blend_ws = nullptr;        // Poisson CG workspace, grown on demand
    size_t blend_ws_bytes = 0;
    chk::AlignCache align_cache;     // host Lanczos tables of the face alignment, built on first use
};

namespace {
int fail(ch_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}
// Every entry point runs with the handle's device current and restores the caller's device on return (a process may own
// handles on several GPUs, or keep torch's current device elsewhere).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
// The tail of every entry point that launches: f() runs with the handle's device current; its hipError_t becomes CH_OK, or CH_ERR_HIP with
// `prefix` ("ch_name: ") and HIP's text as the message.
template <class F>
int launch(ch_handle* h, const char* prefix, F&& f) {
    DeviceGuard guard(h->device);
    const hipError_t e = f();
    return e == hipSuccess ? CH_OK : fail(h, CH_ERR_HIP, std::string(prefix) + hipGetErrorString(e));
}
// The same for the model calls, whose f() returns "" or what went wrong: CH_ERR_STATE for a model that is not finalized, else CH_ERR_HIP
// (an exception included), with `name` in front of the message.
template <class F>
int model_call(ch_handle* h, const char* name, F&& f) {
    if (!h) return CH_ERR_ARG;
    DeviceGuard guard(h->device);
    try {
        const std::string e = f();
        if (!e.empty()) return fail(h, e.find("not finalized") != std::string::npos ? CH_ERR_STATE : CH_ERR_HIP, std::string(name) + ": " + e);
    } catch (const std::exception& ex) {
        return fail(h, CH_ERR_HIP, std::string(name) + ": " + ex.what());
    }
    return CH_OK;
}
// CH_OK, or CH_ERR_ARG for a workspace of `have` bytes where the size query `query_name` (with its argument list, if the message shows one)
// asks for `need`
int workspace_short(ch_handle* h, const char* prefix, size_t have, size_t need, const char* query_name) {
    return have >= need ? CH_OK : fail(h, CH_ERR_ARG, std::string(prefix) + "workspace smaller than " + query_name);
}
hipStream_t hs(ch_stream_t stream) { return static_cast<hipStream_t>(stream); }
}  // namespace

// ---- face alignment (face_align.hip) ---------------------------------------------------------------------------------------------
namespace {
constexpr int ALIGN_MAX_DIM = 32768;         // photo sides; keeps every byte offset and pixel count far inside int / size_t
bool align_dims_ok(int H, int W) { return H >= 1 && W >= 1 && H <= ALIGN_MAX_DIM && W <= ALIGN_MAX_DIM; }
bool pads_ok(const int32_t* p, int radius) {
    return p && p[0] >= 1 && p[1] >= 1 && p[2] >= 1 && p[3] >= 1 && p[0] <= ALIGN_MAX_DIM && p[1] <= ALIGN_MAX_DIM && p[2] <= ALIGN_MAX_DIM &&
           p[3] <= ALIGN_MAX_DIM && radius >= 0 && radius <= ALIGN_MAX_DIM;
}
// plan doubles -> AlignPlan; empty string when consistent with an H x W photo
std::string parse_plan(const double* d, int H, int W, chk::AlignPlan& p) {
    for (int i = 0; i < CH_ALIGN_PLAN_LEN; ++i)
        if (!std::isfinite(d[i])) return "plan[" + std::to_string(i) + "] is not finite";
    for (int i = 0; i < 12; ++i)
        if (d[i] != std::floor(d[i]) || std::fabs(d[i]) > 1e9) return "plan[" + std::to_string(i) + "] is not an integer";
    if (d[20] != std::floor(d[20]) || d[21] != std::floor(d[21]) || std::fabs(d[20]) > 1e9 || std::fabs(d[21]) > 1e9)
        return "transform_size / output_size is not an integer";
    p.shrink = (int)d[0], p.rw = (int)d[1], p.rh = (int)d[2];
    p.cx0 = (int)d[3], p.cy0 = (int)d[4], p.cx1 = (int)d[5], p.cy1 = (int)d[6];
    p.do_pad = d[7] != 0.0, p.pl = (int)d[8], p.pt = (int)d[9], p.pr = (int)d[10], p.pb = (int)d[11];
    for (int i = 0; i < 8; ++i) p.q[i] = d[12 + i];
    p.T = (int)d[20], p.S = (int)d[21];
    if (p.shrink < 0) return "negative shrink";
    if (p.shrink > 1) {
        if (!align_dims_ok(p.rh, p.rw)) return "resized size out of range";
        if (p.rw != (int)std::nearbyint((double)W / p.shrink) || p.rh != (int)std::nearbyint((double)H / p.shrink))
            return "resized size is not the photo's divided by the shrink factor (rounded half to even)";
    } else if (p.rw != W || p.rh != H) {
        return "resized size differs from the photo's without a shrink";
    }
    if (p.cx0 < 0 || p.cy0 < 0 || p.cx1 > p.rw || p.cy1 > p.rh || p.cx0 >= p.cx1 || p.cy0 >= p.cy1) return "crop box outside the (resized) photo";
    if (p.do_pad) {
        const int32_t pads[4] = {p.pl, p.pt, p.pr, p.pb};
        if (!pads_ok(pads, 0)) return "pad widths must be in [1, 32768]";
        if ((p.cy1 - p.cy0) + p.pt + p.pb > ALIGN_MAX_DIM || (p.cx1 - p.cx0) + p.pl + p.pr > ALIGN_MAX_DIM) return "padded size out of range";
    }
    if (p.S < 1 || p.T < p.S || p.T > CH_ALIGN_MAX_TRANSFORM) return "need 1 <= output_size <= transform_size <= " + std::to_string(CH_ALIGN_MAX_TRANSFORM);
    return "";
}
// the checks both paste-back entries share; "" or what is wrong with the arguments
std::string parse_unalign(const uint8_t* photo, int H, int W, const uint8_t* edits, int N, const double* plan, double feather_px,
                          const uint8_t* out, chk::UnalignPlan& p) {
    if (!photo || !edits || !plan || !out || !align_dims_ok(H, W) || N < 1 || N > 65535 || !std::isfinite(feather_px))
        return "bad argument (null pointer, photo side outside [1, 32768], N outside [1, 65535])";
    for (int i = 0; i < CH_UNALIGN_PLAN_LEN; ++i)
        if (!std::isfinite(plan[i])) return "plan[" + std::to_string(i) + "] is not finite";
    for (int i = 6; i < 12; ++i)
        if (i != 10 && (plan[i] != std::floor(plan[i]) || std::fabs(plan[i]) > 1e9)) return "plan[" + std::to_string(i) + "] is not an integer";
    for (int i = 0; i < 6; ++i) p.A[i] = plan[i];
    p.x0 = (int)plan[6], p.y0 = (int)plan[7], p.x1 = (int)plan[8], p.y1 = (int)plan[9];
    p.scale = plan[10], p.S = (int)plan[11];
    if (p.x0 < 0 || p.y0 < 0 || p.x1 > W || p.y1 > H || p.x0 >= p.x1 || p.y0 >= p.y1) return "bbox empty or outside the photo";
    if (!(p.scale > 0.0) || p.scale > CH_UNALIGN_MAX_SCALE) return "scale outside (0, " + std::to_string(CH_UNALIGN_MAX_SCALE) + "]";
    if (p.S < 1 || p.S > CH_ALIGN_MAX_TRANSFORM) return "output_size outside [1, " + std::to_string(CH_ALIGN_MAX_TRANSFORM) + "]";
    const size_t bytes = (size_t)H * W * 3;
    if (out < photo + bytes && photo < out + bytes * (size_t)N) return "out overlaps photo";
    return "";
}
}  // namespace

extern "C" {

int ch_abi_version(void) { return CH_ABI_VERSION; }

int ch_create(int device, ch_handle** out) {
    if (!out) return CH_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return CH_ERR_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return CH_ERR_HIP;
    ch_handle* h = new (std::nothrow) ch_handle();
    if (!h) return CH_ERR_HIP;
    h->device = device;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        // kernels are built for gfx950 only; refuse instead of failing at the first launch
        h->err = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 (MI355X) only";
        *out = h;
        return CH_ERR_HIP;
    }
    *out = h;
    return CH_OK;
}

void ch_destroy(ch_handle* h) {
    if (!h) return;
    {
        DeviceGuard g(h->device);
        (void)hipDeviceSynchronize();
        h->sean.destroy();
        h->shape.destroy();
        h->color.destroy();
        h->bisenet.destroy();
        if (h->blend_ws) (void)hipFree(h->blend_ws);
        h->blend_ws = nullptr;
    }
    delete h;
}

const char* ch_last_error(const ch_handle* h) { return h ? h->err.c_str() : "null handle"; }

int ch_load_tensor(ch_handle* h, int model, const char* name, const void* host, int dtype, const int64_t* shape,
                   int ndim) {
    if (!h || !name || !host || ndim < 0 || ndim > 8 || (ndim > 0 && !shape)) return fail(h, CH_ERR_ARG, "bad argument");
    if (model < 0 || model > CH_MODEL_BISENET) return fail(h, CH_ERR_ARG, "unknown model id");
    if (dtype != CH_F32 && dtype != CH_I64) return fail(h, CH_ERR_ARG, "unsupported dtype");
    try {
        chk::HostTensor t;
        t.dtype = dtype;
        size_t n = 1;
        for (int i = 0; i < ndim; ++i) {
            if (shape[i] < 0) return fail(h, CH_ERR_ARG, "negative dimension");
            t.shape.push_back(shape[i]);
            n *= (size_t)shape[i];
        }
        const size_t bytes = n * (dtype == CH_F32 ? 4 : 8);
        t.data.assign(static_cast<const char*>(host), static_cast<const char*>(host) + bytes);
        h->tensors[model][name] = std::move(t);
    } catch (const std::exception& e) {
        return fail(h, CH_ERR_WEIGHTS, std::string("ch_load_tensor: ") + e.what());
    }
    return CH_OK;
}

int ch_finalize(ch_handle* h, int model, int max_batch, int max_size) {
    if (!h) return CH_ERR_ARG;
    if (model < 0 || model > CH_MODEL_BISENET) return fail(h, CH_ERR_ARG, "unknown model id");
    DeviceGuard guard(h->device);
    if (model != CH_MODEL_SEAN) {
        try {
            std::string e;
            if (model == CH_MODEL_SHAPE) { h->shape.destroy(); e = h->shape.build(h->tensors[model], max_batch); if (!e.empty()) h->shape.destroy(); }
            if (model == CH_MODEL_COLOR) { h->color.destroy(); e = h->color.build(h->tensors[model], max_batch); if (!e.empty()) h->color.destroy(); }
            if (model == CH_MODEL_BISENET) { h->bisenet.destroy(); e = h->bisenet.build(h->tensors[model], max_batch, max_size); if (!e.empty()) h->bisenet.destroy(); }
            if (!e.empty()) return fail(h, CH_ERR_WEIGHTS, "ch_finalize: " + e);
            h->tensors[model].clear();
        } catch (const std::exception& e) {
            return fail(h, CH_ERR_WEIGHTS, std::string("ch_finalize: ") + e.what());
        }
        return CH_OK;
    }
    try {
        h->sean.destroy();
        h->sean_ready = false;
        std::string e = h->sean.build(h->tensors[model], max_batch, max_size);
        if (!e.empty()) {
            h->sean.destroy();
            return fail(h, CH_ERR_WEIGHTS, "ch_finalize: " + e);
        }
        h->tensors[model].clear();   // host copies no longer needed
        h->sean_ready = true;
    } catch (const std::exception& e) {
        return fail(h, CH_ERR_WEIGHTS, std::string("ch_finalize: ") + e.what());
    }
    return CH_OK;
}

size_t ch_sean_noise_floats(const ch_handle* h, int S) {
    if (!h || !h->sean_ready || S <= 0) return 0;
    return h->sean.noise_floats(S);
}

// what every ch_sean_* call checks before it runs: CH_OK, or the status to return (with the handle's message set)
static int sean_precheck(ch_handle* h, const char* name, bool args_ok, const char* what = "bad argument") {
    if (!h) return CH_ERR_ARG;
    if (!h->sean_ready) return fail(h, CH_ERR_STATE, std::string(name) + ": SEAN weights not finalized");
    return args_ok ? CH_OK : fail(h, CH_ERR_ARG, std::string(name) + ": " + what);
}

int ch_sean_generate(ch_handle* h, const uint8_t* labels, const float* codes, const float* noise, uint64_t seed,
                     float* out, int B, int S, ch_stream_t stream) {
    if (int rc = sean_precheck(h, "ch_sean_generate", labels && codes && out, "null pointer")) return rc;
    return model_call(h, "ch_sean_generate", [&] { return h->sean.generate(labels, codes, noise, seed, out, B, S, hs(stream)); });
}
int ch_sean_draw_noise(ch_handle* h, uint64_t seed, float* noise, int B, int S, ch_stream_t stream) {
    if (int rc = sean_precheck(h, "ch_sean_draw_noise", noise && B >= 1)) return rc;
    return model_call(h, "ch_sean_draw_noise", [&] { return h->sean.draw_noise(seed, noise, B, S, hs(stream)); });
}
int ch_sean_encode(ch_handle* h, const float* img, const uint8_t* labels, float* codes, int B, int S,
                   ch_stream_t stream) {
    if (int rc = sean_precheck(h, "ch_sean_encode", img && labels && codes && B >= 1)) return rc;
    return model_call(h, "ch_sean_encode", [&] { return h->sean.encode(img, labels, codes, B, S, hs(stream)); });
}
int ch_sean_encode_features(ch_handle* h, const float* img, int B, int S, ch_stream_t stream) {
    if (int rc = sean_precheck(h, "ch_sean_encode_features", img && B >= 1)) return rc;
    return model_call(h, "ch_sean_encode_features", [&] { return h->sean.encode(img, nullptr, nullptr, B, S, hs(stream), 1); });
}
int ch_sean_encode_regions(ch_handle* h, const uint8_t* labels, float* codes, int B, int S, ch_stream_t stream) {
    if (int rc = sean_precheck(h, "ch_sean_encode_regions", labels && codes && B >= 1)) return rc;
    return model_call(h, "ch_sean_encode_regions", [&] { return h->sean.encode(nullptr, labels, codes, B, S, hs(stream), 2); });
}

int ch_color_generate(ch_handle* h, const float* noise, const float* cond, float* code, int B, ch_stream_t stream) {
    if (h && (!noise || !cond || !code || B < 1)) return fail(h, CH_ERR_ARG, "ch_color_generate: bad argument");
    return model_call(h, "ch_color_generate", [&] { return h->color.generate(noise, cond, code, B, hs(stream)); });
}
int ch_color_encode(ch_handle* h, const float* code, float* out11, int B, ch_stream_t stream) {
    if (h && (!code || !out11 || B < 1)) return fail(h, CH_ERR_ARG, "ch_color_encode: bad argument");
    return model_call(h, "ch_color_encode", [&] { return h->color.encode(code, out11, B, hs(stream)); });
}
int ch_color_predict(ch_handle* h, const float* code, float* out4, int B, ch_stream_t stream) {
    if (h && (!code || !out4 || B < 1)) return fail(h, CH_ERR_ARG, "ch_color_predict: bad argument");
    return model_call(h, "ch_color_predict", [&] { return h->color.predict(code, out4, B, hs(stream)); });
}
int ch_shape_encode(ch_handle* h, const uint8_t* labels, float* hair_code, float* face_code, int B, ch_stream_t stream) {
    if (h && (!labels || (!hair_code && !face_code) || B < 1)) return fail(h, CH_ERR_ARG, "ch_shape_encode: bad argument");
    return model_call(h, "ch_shape_encode", [&] { return h->shape.encode(labels, hair_code, face_code, B, hs(stream)); });
}
int ch_shape_decode(ch_handle* h, const float* hair_code, const float* face_code, float* hair_logit, float* face_logit,
                    uint8_t* labels, float* probs, int B, ch_stream_t stream) {
    if (h && (!face_code || B < 1 || ((labels || probs || hair_logit) && !hair_code)))
        return fail(h, CH_ERR_ARG, "ch_shape_decode: bad argument");
    return model_call(h, "ch_shape_decode", [&] { return h->shape.decode(hair_code, face_code, hair_logit, face_logit, labels, probs, B, hs(stream)); });
}
int ch_shape_combine(ch_handle* h, const float* hair_logit, const float* face_logit, uint8_t* labels, float* probs, int B,
                     ch_stream_t stream) {
    if (h && (!hair_logit || !face_logit || !labels || B < 1)) return fail(h, CH_ERR_ARG, "ch_shape_combine: bad argument");
    return model_call(h, "ch_shape_combine", [&] { return h->shape.combine(hair_logit, face_logit, labels, probs, B, hs(stream)); });
}
int ch_bisenet_parse(ch_handle* h, const float* img, uint8_t* labels, float* logits, int B, int H, int W,
                     ch_stream_t stream) {
    if (h && (!img || !labels || B < 1)) return fail(h, CH_ERR_ARG, "ch_bisenet_parse: bad argument");
    return model_call(h, "ch_bisenet_parse", [&] { return h->bisenet.parse(img, labels, logits, B, H, W, hs(stream)); });
}

int ch_blend_mask_batch(ch_handle* h, const uint8_t* target_parsing, const uint8_t* face_parsing, uint8_t* out, int B, int H, int W,
                        ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!target_parsing || !face_parsing || !out || B < 1 || B > 65535 || H < 1 || W < 1)
        return fail(h, CH_ERR_ARG, "ch_blend_mask: bad argument");
    return launch(h, "ch_blend_mask: ", [&] { return chk::blend_mask_batch(target_parsing, face_parsing, out, B, H, W, hs(stream)); });
}

int ch_blend_mask(ch_handle* h, const uint8_t* target_parsing, const uint8_t* face_parsing, uint8_t* out, int H, int W,
                  ch_stream_t stream) {
    return ch_blend_mask_batch(h, target_parsing, face_parsing, out, 1, H, W, stream);
}

int ch_poisson_blend_batch(ch_handle* h, const uint8_t* source, const uint8_t* target, const uint8_t* mask, uint8_t* out, int B, int H,
                           int W, int with_gamma, int max_iters, double rel_tol, int* iters, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!source || !target || !mask || !out || B < 1 || B > 65535 || H < 3 || W < 3 || max_iters < 0 || !(rel_tol >= 0.0))
        return fail(h, CH_ERR_ARG, "ch_poisson_blend: bad argument (B >= 1; images need H, W >= 3)");
    DeviceGuard guard(h->device);
    const size_t need = (size_t)B * chk::poisson_workspace_bytes(H, W);
    if (need > h->blend_ws_bytes) {
        if (h->blend_ws) (void)hipFree(h->blend_ws);
        h->blend_ws = nullptr;
        h->blend_ws_bytes = 0;
        if (hipMalloc(&h->blend_ws, need) != hipSuccess) return fail(h, CH_ERR_HIP, "ch_poisson_blend: workspace allocation failed");
        h->blend_ws_bytes = need;
    }
    return launch(h, "ch_poisson_blend: ",
                  [&] { return chk::poisson_blend_batch(source, target, mask, out, B, H, W, with_gamma, max_iters, rel_tol, h->blend_ws, iters, hs(stream)); });
}

int ch_poisson_blend(ch_handle* h, const uint8_t* source, const uint8_t* target, const uint8_t* mask, uint8_t* out, int H, int W,
                     int with_gamma, int max_iters, double rel_tol, int* iters, ch_stream_t stream) {
    return ch_poisson_blend_batch(h, source, target, mask, out, 1, H, W, with_gamma, max_iters, rel_tol, iters, stream);
}

size_t ch_mask_warp_workspace_bytes(int B) { return chk::mask_warp_workspace_bytes(B); }

namespace {
// the checks ch_mask_warp_batch and ch_mask_warp_batch_dev share; `fn` names the entry point in the messages
int mask_warp_precheck(const char* fn, ch_handle* h, const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int32_t* F,
                       const int32_t* b, const float* bc, const int32_t* desc, const float* U_in, const uint8_t* labels_out, const void* workspace,
                       size_t workspace_bytes, int B) {
    if (!h) return CH_ERR_ARG;
    const std::string f = std::string(fn) + ": ";
    if (!hair_labels || !face_labels || !V || !F || !desc || !labels_out || !workspace || B < 1 || B > 65535 || (!U_in && (!b || !bc)))
        return fail(h, CH_ERR_ARG, f + "bad argument");
    return workspace_short(h, f.c_str(), workspace_bytes, chk::mask_warp_workspace_bytes(B), "ch_mask_warp_workspace_bytes(B)");
}
}  // namespace

int ch_mask_warp_batch(ch_handle* h, const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int32_t* F,
                       const int32_t* b, const float* bc, const int32_t* desc, const float* U_in, uint8_t* labels_out, float* uv_out,
                       float* U_out, void* workspace, size_t workspace_bytes, int B, ch_stream_t stream) {
    if (int rc = mask_warp_precheck("ch_mask_warp_batch", h, hair_labels, face_labels, V, F, b, bc, desc, U_in, labels_out, workspace,
                                    workspace_bytes, B))
        return rc;
    for (int i = 0; i < B; ++i) {
        const int32_t* d = desc + 6 * i;
        if (d[0] < 0 || d[2] < 0 || d[4] < 0 || d[5] < 0)
            return fail(h, CH_ERR_ARG, "ch_mask_warp_batch: negative offset or count in desc[" + std::to_string(i) + "]");
        if (d[1] < 3 || d[1] > chk::WARP_MAX_V || d[3] < 1 || d[3] > chk::WARP_MAX_F)
            return fail(h, CH_ERR_ARG, "ch_mask_warp_batch: mesh " + std::to_string(i) + " has " + std::to_string(d[1]) + " vertices / " +
                                           std::to_string(d[3]) + " triangles; supported: 3.." + std::to_string(chk::WARP_MAX_V) +
                                           " vertices, 1.." + std::to_string(chk::WARP_MAX_F) + " triangles");
    }
    return launch(h, "ch_mask_warp_batch: ", [&] {
        return chk::mask_warp_batch(hair_labels, face_labels, V, F, b, bc, desc, U_in, labels_out, uv_out, U_out, workspace, B,
                                    CH_WARP_OUTER_ITERS, CH_WARP_MAX_CG, CH_WARP_REL_TOL, hs(stream));
    });
}

int ch_mask_warp_batch_dev(ch_handle* h, const uint8_t* hair_labels, const uint8_t* face_labels, const float* V, const int32_t* F,
                           const int32_t* b, const float* bc, const int32_t* desc, const float* U_in, uint8_t* labels_out, float* uv_out,
                           float* U_out, void* workspace, size_t workspace_bytes, int B, ch_stream_t stream) {
    if (int rc = mask_warp_precheck("ch_mask_warp_batch_dev", h, hair_labels, face_labels, V, F, b, bc, desc, U_in, labels_out, workspace,
                                    workspace_bytes, B))
        return rc;
    return launch(h, "ch_mask_warp_batch_dev: ", [&] {
        return chk::mask_warp_batch_dev(hair_labels, face_labels, V, F, b, bc, desc, U_in, labels_out, uv_out, U_out, workspace, B,
                                        CH_WARP_OUTER_ITERS, CH_WARP_MAX_CG, CH_WARP_REL_TOL, hs(stream));
    });
}

size_t ch_delaunay_workspace_bytes(int B) { return chk::delaunay_workspace_bytes(B); }

int ch_delaunay_batch(ch_handle* h, const float* V, const int32_t* v_desc, int32_t* F, int32_t* n_f, int32_t* status, void* workspace,
                      size_t workspace_bytes, int B, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!V || !v_desc || !F || !n_f || !status || !workspace || B < 1 || B > 65535)
        return fail(h, CH_ERR_ARG, "ch_delaunay_batch: bad argument");
    if (int rc = workspace_short(h, "ch_delaunay_batch: ", workspace_bytes, chk::delaunay_workspace_bytes(B), "ch_delaunay_workspace_bytes(B)"))
        return rc;
    for (int i = 0; i < B; ++i)
        if (v_desc[2 * i] < 0) return fail(h, CH_ERR_ARG, "ch_delaunay_batch: negative offset in v_desc[" + std::to_string(i) + "]");
    static_assert(CH_DELAUNAY_OK == chk::DELAUNAY_OK && CH_DELAUNAY_BAD_COUNT == chk::DELAUNAY_BAD_COUNT &&
                      CH_DELAUNAY_OFF_GRID == chk::DELAUNAY_OFF_GRID && CH_DELAUNAY_DUPLICATE == chk::DELAUNAY_DUPLICATE &&
                      CH_DELAUNAY_COLLINEAR == chk::DELAUNAY_COLLINEAR && CH_DELAUNAY_INTERNAL == chk::DELAUNAY_INTERNAL,
                  "status codes of the header and of delaunay.hip");
    return launch(h, "ch_delaunay_batch: ", [&] { return chk::delaunay_batch(V, v_desc, F, n_f, status, workspace, B, hs(stream)); });
}

size_t ch_resample_lanczos_workspace_bytes(int Hs, int Ws, int C, int Hd, int Wd) {
    if (!align_dims_ok(Hs, Ws) || !align_dims_ok(Hd, Wd) || C < 1 || C > 4) return 0;
    return chk::lanczos_workspace_bytes(Hs, Ws, C, Hd, Wd);
}

int ch_resample_lanczos_u8(ch_handle* h, const uint8_t* src, int Hs, int Ws, int C, uint8_t* dst, int Hd, int Wd, void* workspace,
                           size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!src || !dst || !workspace || !align_dims_ok(Hs, Ws) || !align_dims_ok(Hd, Wd) || C < 1 || C > 4)
        return fail(h, CH_ERR_ARG, "ch_resample_lanczos_u8: bad argument");
    const size_t need = chk::lanczos_workspace_bytes(Hs, Ws, C, Hd, Wd);
    if (int rc = workspace_short(h, "ch_resample_lanczos_u8: ", workspace_bytes, need, "ch_resample_lanczos_workspace_bytes")) return rc;
    return launch(h, "ch_resample_lanczos_u8: ", [&] {
        return chk::lanczos_resample_u8(h->align_cache, src, (long long)Ws * C, Hs, Ws, C, dst, Hd, Wd, workspace, hs(stream));
    });
}

size_t ch_quad_warp_workspace_bytes(int T, int S) {
    if (S < 1 || T < S || T > CH_ALIGN_MAX_TRANSFORM) return 0;
    return chk::quad_warp_workspace_bytes(T, S);
}

int ch_quad_warp_resample_u8(ch_handle* h, const uint8_t* src, int Hs, int Ws, const double* coef, int T, int S, uint8_t* dst, void* workspace,
                             size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!src || !dst || !coef || !align_dims_ok(Hs, Ws) || S < 1 || T < S || T > CH_ALIGN_MAX_TRANSFORM || (!workspace && S != T))
        return fail(h, CH_ERR_ARG, "ch_quad_warp_resample_u8: bad argument");
    for (int i = 0; i < 8; ++i)
        if (!std::isfinite(coef[i])) return fail(h, CH_ERR_ARG, "ch_quad_warp_resample_u8: quad coefficient is not finite");
    const size_t need = chk::quad_warp_workspace_bytes(T, S);
    if (int rc = workspace_short(h, "ch_quad_warp_resample_u8: ", workspace_bytes, need, "ch_quad_warp_workspace_bytes(T, S)")) return rc;
    return launch(h, "ch_quad_warp_resample_u8: ", [&] {
        return chk::quad_warp_resample_u8(h->align_cache, src, (long long)Ws * 3, Hs, Ws, coef, T, S, dst, workspace, hs(stream));
    });
}

size_t ch_align_pad_workspace_bytes(int Hs, int Ws, const int32_t* pads, int radius) {
    if (!align_dims_ok(Hs, Ws) || !pads_ok(pads, radius)) return 0;
    const int Hp = Hs + pads[1] + pads[3], Wp = Ws + pads[0] + pads[2];
    if (!align_dims_ok(Hp, Wp)) return 0;
    return chk::align_pad_workspace_bytes(Hp, Wp, radius);
}

int ch_align_pad_feather_u8(ch_handle* h, const uint8_t* src, int Hs, int Ws, const int32_t* pads, const double* gauss_w, int radius,
                            uint8_t* dst, void* workspace, size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!src || !dst || !gauss_w || !workspace || !align_dims_ok(Hs, Ws) || !pads_ok(pads, radius))
        return fail(h, CH_ERR_ARG, "ch_align_pad_feather_u8: bad argument (pads must be >= 1)");
    const size_t need = ch_align_pad_workspace_bytes(Hs, Ws, pads, radius);
    if (need == 0) return fail(h, CH_ERR_ARG, "ch_align_pad_feather_u8: padded size out of range");
    if (int rc = workspace_short(h, "ch_align_pad_feather_u8: ", workspace_bytes, need, "ch_align_pad_workspace_bytes")) return rc;
    return launch(h, "ch_align_pad_feather_u8: ", [&] {
        return chk::align_pad_feather_u8(src, (long long)Ws * 3, Hs, Ws, pads, gauss_w, radius, dst, workspace, hs(stream));
    });
}

size_t ch_face_align_workspace_bytes(int H, int W, const double* plan, int radius) {
    chk::AlignPlan p;
    if (!plan || !align_dims_ok(H, W) || radius < 0 || radius > ALIGN_MAX_DIM || !parse_plan(plan, H, W, p).empty()) return 0;
    return chk::face_align_workspace_bytes(H, W, p, radius) + 256;
}

int ch_face_align(ch_handle* h, const uint8_t* src, int H, int W, const double* plan, const double* gauss_w, int radius, uint8_t* dst,
                  void* workspace, size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!src || !dst || !plan || !workspace || !align_dims_ok(H, W) || radius < 0 || radius > ALIGN_MAX_DIM)
        return fail(h, CH_ERR_ARG, "ch_face_align: bad argument");
    chk::AlignPlan p;
    const std::string why = parse_plan(plan, H, W, p);
    if (!why.empty()) return fail(h, CH_ERR_ARG, "ch_face_align: " + why);
    if (p.do_pad && !gauss_w) return fail(h, CH_ERR_ARG, "ch_face_align: the plan pads but gauss_w is null");
    const size_t need = chk::face_align_workspace_bytes(H, W, p, radius) + 256;
    if (int rc = workspace_short(h, "ch_face_align: ", workspace_bytes, need, "ch_face_align_workspace_bytes")) return rc;
    return launch(h, "ch_face_align: ", [&] { return chk::face_align(h->align_cache, src, H, W, p, gauss_w, radius, dst, workspace, hs(stream)); });
}

// ---- paste-back (face_unalign.hip, face_matte.hip) ------------------------------------------------------------------------------------
int ch_face_unalign(ch_handle* h, const uint8_t* photo, int H, int W, const uint8_t* edits, int N, const uint8_t* weight, const double* plan,
                    double feather_px, uint8_t* out, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    chk::UnalignPlan p;
    const std::string why = parse_unalign(photo, H, W, edits, N, plan, feather_px, out, p);
    if (!why.empty()) return fail(h, CH_ERR_ARG, "ch_face_unalign: " + why);
    return launch(h, "ch_face_unalign: ", [&] { return chk::face_unalign(photo, edits, weight, p, H, W, N, feather_px, out, hs(stream)); });
}

size_t ch_face_unalign_matte_workspace_bytes(int H, int W, const double* plan, int radius) {
    if (!plan || !align_dims_ok(H, W) || radius < 1 || radius > CH_MATTE_MAX_RADIUS) return 0;
    for (int i = 6; i < 10; ++i)
        if (!std::isfinite(plan[i]) || plan[i] != std::floor(plan[i]) || std::fabs(plan[i]) > 1e9) return 0;
    const int x0 = (int)plan[6], y0 = (int)plan[7], x1 = (int)plan[8], y1 = (int)plan[9];
    if (x0 < 0 || y0 < 0 || x1 > W || y1 > H || x0 >= x1 || y0 >= y1) return 0;
    return chk::face_matte_workspace_bytes(x1 - x0, y1 - y0);
}

int ch_face_unalign_matte(ch_handle* h, const uint8_t* photo, int H, int W, const uint8_t* edits, int N, const uint8_t* weight, const double* plan,
                          double feather_px, int radius, double eps, uint8_t* out, float* alpha_out, void* workspace, size_t workspace_bytes,
                          ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    chk::UnalignPlan p;
    const std::string why = parse_unalign(photo, H, W, edits, N, plan, feather_px, out, p);
    if (!why.empty()) return fail(h, CH_ERR_ARG, "ch_face_unalign_matte: " + why);
    if (!weight) return fail(h, CH_ERR_ARG, "ch_face_unalign_matte: weight is null (the matte refines a weight map)");
    if (radius < 1 || radius > CH_MATTE_MAX_RADIUS)
        return fail(h, CH_ERR_ARG, "ch_face_unalign_matte: radius outside [1, " + std::to_string(CH_MATTE_MAX_RADIUS) + "]");
    if (!(eps > 0.0) || !std::isfinite(eps)) return fail(h, CH_ERR_ARG, "ch_face_unalign_matte: eps must be positive and finite");
    if (!workspace || reinterpret_cast<uintptr_t>(workspace) % 256 != 0)
        return fail(h, CH_ERR_ARG, "ch_face_unalign_matte: workspace is null or not 256-byte aligned");
    const size_t need = chk::face_matte_workspace_bytes(p.x1 - p.x0, p.y1 - p.y0);
    if (int rc = workspace_short(h, "ch_face_unalign_matte: ", workspace_bytes, need, "ch_face_unalign_matte_workspace_bytes")) return rc;
    if (reinterpret_cast<uintptr_t>(alpha_out) % 4 != 0) return fail(h, CH_ERR_ARG, "ch_face_unalign_matte: alpha_out is not 4-byte aligned");
    return launch(h, "ch_face_unalign_matte: ",
                  [&] { return chk::face_unalign_matte(photo, edits, weight, p, H, W, N, feather_px, radius, eps, out, alpha_out, workspace, hs(stream)); });
}

// ---- median style codes (style_medoid.hip) ---------------------------------------------------------------------------------------
namespace {
bool medoid_args_ok(const int64_t* off, int R, int dim, int n_split) {
    if (!off || R < 1 || R > CH_MEDOID_MAX_SEGMENTS || dim < 4 || dim > CH_MEDOID_MAX_DIM || dim % 4 != 0 || n_split < 0 || off[0] != 0)
        return false;
    for (int r = 0; r < R; ++r)
        if (off[r + 1] < off[r] || off[r + 1] - off[r] > CH_MEDOID_MAX_ROWS) return false;
    return true;
}
}  // namespace

size_t ch_style_medoid_workspace_bytes(const int64_t* seg_offsets, int R, int dim, int n_split) {
    if (!medoid_args_ok(seg_offsets, R, dim, n_split)) return 0;
    return chk::style_medoid_workspace_bytes(seg_offsets, R, n_split);
}

int ch_style_medoid(ch_handle* h, const float* codes, const int64_t* seg_offsets, int R, int dim, int n_split, int32_t* index, double* sums,
                    float* mean, void* workspace, size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!medoid_args_ok(seg_offsets, R, dim, n_split))
        return fail(h, CH_ERR_ARG, "ch_style_medoid: bad argument (dim a multiple of 4, seg_offsets ascending from 0, n_split >= 0)");
    if (!index || !mean || !workspace || (!codes && seg_offsets[R] > 0) || (reinterpret_cast<uintptr_t>(codes) & 15))
        return fail(h, CH_ERR_ARG, "ch_style_medoid: null output or workspace, or codes not 16-byte aligned");
    const size_t need = chk::style_medoid_workspace_bytes(seg_offsets, R, n_split);
    if (int rc = workspace_short(h, "ch_style_medoid: ", workspace_bytes, need, "ch_style_medoid_workspace_bytes")) return rc;
    return launch(h, "ch_style_medoid: ", [&] { return chk::style_medoid(codes, seg_offsets, R, dim, n_split, index, sums, mean, workspace, hs(stream)); });
}

int ch_resize_linear_u8(ch_handle* h, const uint8_t* src, uint8_t* dst, int B, int Hs, int Ws, int C, int Hd, int Wd,
                        ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!src || !dst || B < 1 || B > 65535 || Hs < 1 || Ws < 1 || C < 1 || C > 4 || Hd < 1 || Hd > 65535 || Wd < 1)
        return fail(h, CH_ERR_ARG, "ch_resize_linear_u8: bad argument");
    return launch(h, "ch_resize_linear_u8: ", [&] { return chk::resize_linear_u8(src, dst, B, Hs, Ws, C, Hd, Wd, hs(stream)); });
}

// ---- image ingest (ingest.hip) ------------------------------------------------------------------------------------------------------
size_t ch_ingest_workspace_bytes(const void* batch, size_t batch_bytes, int N, int P, int mode) {
    size_t need = 0;
    return chk::ingest_check(batch, batch_bytes, N, P, mode, need).empty() ? need : 0;
}

namespace {
static_assert(CH_INGEST_PIL_BILINEAR == chk::INGEST_PIL && CH_INGEST_CV2_LINEAR == chk::INGEST_CV2 && CH_INGEST_LABELS == chk::INGEST_LABELS &&
                  CH_INGEST_DESC_BYTES == sizeof(chk::IngestImage) && CH_INGEST_MAX_SIDE == chk::INGEST_MAX_SIDE &&
                  CH_INGEST_MAX_OUT == chk::INGEST_MAX_OUT,
              "ingest constants of the header and of kernels.h");
// the checks both ingest entries share behind their null-pointer test: the batch, then the workspace
int ingest_refuse(ch_handle* h, const char* prefix, const void* batch, size_t batch_bytes, int N, int P, int mode, const void* workspace,
                  size_t workspace_bytes) {
    size_t need = 0;
    const std::string why = chk::ingest_check(batch, batch_bytes, N, P, mode, need);
    if (!why.empty()) return fail(h, CH_ERR_ARG, std::string(prefix) + why);
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return fail(h, CH_ERR_ARG, std::string(prefix) + "workspace is not 256-byte aligned");
    return workspace_short(h, prefix, workspace_bytes, need, "ch_ingest_workspace_bytes");
}
}  // namespace

int ch_ingest_images(ch_handle* h, const void* batch, size_t batch_bytes, int N, int P, int mode, const float* lut, float* out, void* workspace,
                     size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!batch || !lut || !out || !workspace) return fail(h, CH_ERR_ARG, "ch_ingest_images: null pointer");
    if (mode != CH_INGEST_PIL_BILINEAR && mode != CH_INGEST_CV2_LINEAR) return fail(h, CH_ERR_ARG, "ch_ingest_images: mode is not 0 or 1");
    if (reinterpret_cast<uintptr_t>(lut) % 4 != 0 || reinterpret_cast<uintptr_t>(out) % 16 != 0)
        return fail(h, CH_ERR_ARG, "ch_ingest_images: lut is not 4-byte aligned or out is not 16-byte aligned");
    if (int rc = ingest_refuse(h, "ch_ingest_images: ", batch, batch_bytes, N, P, mode, workspace, workspace_bytes)) return rc;
    return launch(h, "ch_ingest_images: ", [&] { return chk::ingest_images(batch, batch_bytes, N, P, mode, lut, out, workspace, hs(stream)); });
}

int ch_ingest_labels(ch_handle* h, const void* batch, size_t batch_bytes, int N, int S, uint8_t* out, void* workspace, size_t workspace_bytes,
                     ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!batch || !out || !workspace) return fail(h, CH_ERR_ARG, "ch_ingest_labels: null pointer");
    if (int rc = ingest_refuse(h, "ch_ingest_labels: ", batch, batch_bytes, N, S, CH_INGEST_LABELS, workspace, workspace_bytes)) return rc;
    return launch(h, "ch_ingest_labels: ", [&] { return chk::ingest_labels(batch, batch_bytes, N, S, out, workspace, hs(stream)); });
}

// ---- EXIF orientation (orient.hip) ----------------------------------------------------------------------------------------------------
static_assert(CH_ORIENT_DESC_BYTES == sizeof(chk::OrientImage) && CH_ORIENT_MAX_SIDE == chk::ORIENT_MAX_SIDE,
              "orient constants of the header and of orient_batch.h");

size_t ch_orient_workspace_bytes(const void* batch, size_t batch_bytes, int N, size_t dst_bytes) {
    size_t need = 0;
    return chk::orient_check(batch, batch_bytes, N, 0, dst_bytes, need).empty() ? need : 0;
}

int ch_orient_u8(ch_handle* h, const void* batch, size_t batch_bytes, int N, uint8_t* dst, size_t dst_bytes, void* workspace,
                 size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!batch || !dst || !workspace) return fail(h, CH_ERR_ARG, "ch_orient_u8: null pointer");
    size_t need = 0;
    const std::string why = chk::orient_check(batch, batch_bytes, N, reinterpret_cast<uintptr_t>(dst), dst_bytes, need);
    if (!why.empty()) return fail(h, CH_ERR_ARG, "ch_orient_u8: " + why);
    if (reinterpret_cast<uintptr_t>(workspace) % 256 != 0) return fail(h, CH_ERR_ARG, "ch_orient_u8: workspace is not 256-byte aligned");
    if (int rc = workspace_short(h, "ch_orient_u8: ", workspace_bytes, need, "ch_orient_workspace_bytes")) return rc;
    return launch(h, "ch_orient_u8: ", [&] { return chk::orient_u8(batch, batch_bytes, N, dst, workspace, hs(stream)); });
}

int ch_hair_erode(ch_handle* h, const uint8_t* labels, int B, int Hl, int Wl, int label, int ksize, uint8_t* mask, int H, int W,
                  ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!labels || !mask || B < 1 || B > 65535 || Hl < 1 || Wl < 1 || H < 1 || W < 1 || (H + 15) / 16 > 65535 || label < 0 || label > 255)
        return fail(h, CH_ERR_ARG, "ch_hair_erode: bad argument");
    if (ksize < 1 || ksize > 2 * chk::HAIR_ERODE_MAX_R + 1 || ksize % 2 == 0)
        return fail(h, CH_ERR_ARG, "ch_hair_erode: ksize must be odd and in [1, 31]");
    // cv2.getStructuringElement(MORPH_ELLIPSE, (ksize, ksize)): row dy spans dx = cvRound(c * sqrt((r^2 - dy^2) / r^2)), c = r
    chk::HairErodeRows rows{};
    const int r = ksize / 2;
    rows.r = r;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    for (int dy = -r; dy <= r; ++dy)
        rows.hw[dy + r] = (int)std::nearbyint(r * std::sqrt(((double)r * r - (double)dy * dy) * inv_r2));
    return launch(h, "ch_hair_erode: ", [&] { return chk::hair_erode(labels, B, Hl, Wl, label, rows, mask, H, W, hs(stream)); });
}

int ch_hair_color_stats(ch_handle* h, const uint8_t* img, const uint8_t* mask, int B, int H, int W, int64_t* sums, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!img || !mask || !sums || B < 1 || B > 65535 || H < 1 || W < 1) return fail(h, CH_ERR_ARG, "ch_hair_color_stats: bad argument");
    if ((int64_t)H * W > INT64_MAX / (255LL * 255 * 255 * 255))
        return fail(h, CH_ERR_ARG, "ch_hair_color_stats: H * W too large for exact int64 sums of c^4");
    return launch(h, "ch_hair_color_stats: ", [&] { return chk::hair_color_stats(img, mask, B, H, W, sums, hs(stream)); });
}

int ch_sheet_compose(ch_handle* h, const void* src, int kind, int n, int Hs, int Ws, const int32_t* cells, const uint8_t* lut, uint8_t* canvas,
                     int rows, int cols, int H, int W, int margin, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!src || !cells || !canvas || kind < 0 || kind > 2 || (kind == 2 && !lut))
        return fail(h, CH_ERR_ARG, "ch_sheet_compose: null pointer or unknown source kind");
    if (n < 1 || n > 65535) return fail(h, CH_ERR_ARG, "ch_sheet_compose: n outside 1..65535");
    if (Hs < 1 || Ws < 1 || rows < 1 || cols < 1 || H < 1 || W < 1 || margin < 0)
        return fail(h, CH_ERR_ARG, "ch_sheet_compose: sizes must be positive (margin >= 0)");
    if ((int64_t)rows * H > INT32_MAX || (int64_t)cols * ((int64_t)W + margin) * 3 > INT32_MAX || (int64_t)Hs * Ws > INT32_MAX)
        return fail(h, CH_ERR_ARG, "ch_sheet_compose: sheet or source too large");
    return launch(h, "ch_sheet_compose: ",
                  [&] { return chk::sheet_compose(src, kind, n, Hs, Ws, cells, lut, canvas, rows, cols, H, W, margin, hs(stream)); });
}

int ch_sweep_stats(ch_handle* h, const void* img, int kind, const uint8_t* labels, const int32_t* ref, int N, int H, int W, int lh, int lw,
                   int64_t* stats, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    if (!img || !labels || !ref || !stats || kind < 0 || kind > 1)
        return fail(h, CH_ERR_ARG, "ch_sweep_stats: null pointer or unknown image kind");
    if (N < 1 || N > 65535) return fail(h, CH_ERR_ARG, "ch_sweep_stats: N outside 1..65535");
    if (H < 1 || W < 1 || lh < 1 || lw < 1) return fail(h, CH_ERR_ARG, "ch_sweep_stats: sizes must be positive");
    if (H > 32768 || W > 32768 || (int64_t)H * W > (1 << 30) || (int64_t)lh * lw > (1 << 30))
        return fail(h, CH_ERR_ARG, "ch_sweep_stats: image or label map too large (sides <= 32768, H * W <= 2^30)");
    return launch(h, "ch_sweep_stats: ", [&] { return chk::sweep_stats(img, kind, labels, ref, N, H, W, lh, lw, stats, hs(stream)); });
}

// ---- PNG encoding (png_encode.hip) -----------------------------------------------------------------------------------------------
namespace {
bool png_dims_ok(int H, int W, int C) {
    return (C == 1 || C == 3 || C == 4) && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && (int64_t)H * W <= (1 << 30);
}
}  // namespace

int ch_png_chunk_bytes(void) { return chk::PNG_CHUNK; }

size_t ch_png_zlib_bound(int H, int W, int C) { return png_dims_ok(H, W, C) ? chk::png_zlib_bound(H, W, C) : 0; }

size_t ch_png_encode_workspace_bytes(int N, int H, int W, int C) {
    return (N >= 1 && N <= 65535 && png_dims_ok(H, W, C)) ? chk::png_encode_workspace_bytes(N, H, W, C) : 0;
}

namespace {
// ch_png_encode and ch_png_encode_dist: `fn` names the entry point in the messages
int png_encode_checked(const char* fn, ch_handle* h, const uint8_t* img, int N, int H, int W, int C, int filter, const int* dist, int ndist,
                       uint8_t* out, int64_t* sizes, void* workspace, size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    const std::string f = std::string(fn) + ": ";
    if (!img || !out || !sizes || !workspace) return fail(h, CH_ERR_ARG, f + "null pointer");
    if (C != 1 && C != 3 && C != 4) return fail(h, CH_ERR_ARG, f + "C must be 1, 3 or 4");
    if (filter < -1 || filter > 4) return fail(h, CH_ERR_ARG, f + "filter must be -1 (adaptive) or 0..4");
    if (N < 1 || N > 65535) return fail(h, CH_ERR_ARG, f + "N outside 1..65535");
    if (!png_dims_ok(H, W, C)) return fail(h, CH_ERR_ARG, f + "image too small or too large (sides 1..32768, H * W <= 2^30)");
    if (ndist < 0 || ndist > 3) return fail(h, CH_ERR_ARG, f + "ndist outside 0..3");
    if (ndist > 0 && !dist) return fail(h, CH_ERR_ARG, f + "dist is null with ndist > 0");
    for (int k = 0; k < ndist; ++k) {
        if (dist[k] < 2 || dist[k] > 32767) return fail(h, CH_ERR_ARG, f + "distance outside 2..32767 (distance 1 is always present)");
        for (int j = 0; j < k; ++j)
            if (dist[j] == dist[k]) return fail(h, CH_ERR_ARG, f + "duplicate distance");
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(h, CH_ERR_ARG, f + "workspace not 16-byte aligned");
    if (int rc = workspace_short(h, f.c_str(), workspace_bytes, chk::png_encode_workspace_bytes(N, H, W, C), "ch_png_encode_workspace_bytes"))
        return rc;
    return launch(h, f.c_str(), [&] { return chk::png_encode_dist(img, N, H, W, C, filter, dist, ndist, out, sizes, workspace, hs(stream)); });
}
}  // namespace

int ch_png_encode(ch_handle* h, const uint8_t* img, int N, int H, int W, int C, int filter, uint8_t* out, int64_t* sizes, void* workspace,
                  size_t workspace_bytes, ch_stream_t stream) {
    return png_encode_checked("ch_png_encode", h, img, N, H, W, C, filter, nullptr, 0, out, sizes, workspace, workspace_bytes, stream);
}

int ch_png_encode_dist(ch_handle* h, const uint8_t* img, int N, int H, int W, int C, int filter, const int* dist, int ndist, uint8_t* out,
                       int64_t* sizes, void* workspace, size_t workspace_bytes, ch_stream_t stream) {
    return png_encode_checked("ch_png_encode_dist", h, img, N, H, W, C, filter, dist, ndist, out, sizes, workspace, workspace_bytes, stream);
}

// ---- PNG decoding (png_decode.hip, png_inflate_core.h) ---------------------------------------------------------------------------------
size_t ch_png_decode_workspace_bytes(int N, int H, int W, int C) {
    return (N >= 1 && N <= 65535 && png_dims_ok(H, W, C)) ? chk::png_decode_workspace_bytes(N, H, W, C) : 0;
}

int ch_png_decode(ch_handle* h, const uint8_t* streams, const int64_t* offsets, int N, int H, int W, int C, uint8_t* img, int32_t* status,
                  void* workspace, size_t workspace_bytes, ch_stream_t stream) {
    namespace pi = chk::pnginf;
    static_assert(CH_PNG_DEC_OK == pi::OK && CH_PNG_DEC_BAD_HEADER == pi::BAD_HEADER && CH_PNG_DEC_BAD_BLOCK == pi::BAD_BLOCK &&
                      CH_PNG_DEC_BAD_CODE == pi::BAD_CODE && CH_PNG_DEC_BAD_SYMBOL == pi::BAD_SYMBOL &&
                      CH_PNG_DEC_BAD_DISTANCE == pi::BAD_DISTANCE && CH_PNG_DEC_INPUT_END == pi::INPUT_END && CH_PNG_DEC_SIZE == pi::SIZE &&
                      CH_PNG_DEC_ADLER == pi::ADLER && CH_PNG_DEC_BAD_FILTER == pi::BAD_FILTER,
                  "status codes of the header and of png_inflate_core.h");
    if (!h) return CH_ERR_ARG;
    const std::string f = "ch_png_decode: ";
    if (!streams || !offsets || !img || !status || !workspace) return fail(h, CH_ERR_ARG, f + "null pointer");
    if (N < 1 || N > 65535) return fail(h, CH_ERR_ARG, f + "N outside 1..65535");
    if (!png_dims_ok(H, W, C)) return fail(h, CH_ERR_ARG, f + "C must be 1, 3 or 4, sides 1..32768, H * W <= 2^30");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(h, CH_ERR_ARG, f + "workspace not 16-byte aligned");
    if (int rc = workspace_short(h, f.c_str(), workspace_bytes, chk::png_decode_workspace_bytes(N, H, W, C), "ch_png_decode_workspace_bytes"))
        return rc;
    return launch(h, f.c_str(), [&] { return chk::png_decode(streams, offsets, N, H, W, C, img, status, workspace, hs(stream)); });
}

// ---- JPEG encoding (jpeg_encode.hip) ---------------------------------------------------------------------------------------------------
namespace {
bool jpeg_dims_ok(int H, int W, int C, int subsampling) {
    return (C == 1 || C == 3) && (subsampling == 0 || subsampling == 2) && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 &&
           (int64_t)H * W <= (1 << 30);
}
}  // namespace

size_t ch_jpeg_scan_bound(int H, int W, int C, int subsampling) {
    return jpeg_dims_ok(H, W, C, subsampling) ? chk::jpeg_scan_bound(H, W, C, subsampling) : 0;
}

size_t ch_jpeg_encode_workspace_bytes(int N, int H, int W, int C, int subsampling) {
    return (N >= 1 && N <= 65535 && jpeg_dims_ok(H, W, C, subsampling)) ? chk::jpeg_encode_workspace_bytes(N, H, W, C, subsampling) : 0;
}

int ch_jpeg_encode(ch_handle* h, const uint8_t* img, int N, int H, int W, int C, int quality, int subsampling, uint8_t* out, int64_t* sizes,
                   void* workspace, size_t workspace_bytes, ch_stream_t stream) {
    if (!h) return CH_ERR_ARG;
    const std::string f = "ch_jpeg_encode: ";
    if (!img || !out || !sizes || !workspace) return fail(h, CH_ERR_ARG, f + "null pointer");
    if (C != 1 && C != 3) return fail(h, CH_ERR_ARG, f + "C must be 1 (grey) or 3 (RGB)");
    if (quality < 1 || quality > 100) return fail(h, CH_ERR_ARG, f + "quality outside 1..100");
    if (subsampling != 0 && subsampling != 2) return fail(h, CH_ERR_ARG, f + "subsampling must be 0 (4:4:4) or 2 (4:2:0)");
    if (N < 1 || N > 65535) return fail(h, CH_ERR_ARG, f + "N outside 1..65535");
    if (!jpeg_dims_ok(H, W, C, subsampling)) return fail(h, CH_ERR_ARG, f + "image too small or too large (sides 1..32768, H * W <= 2^30)");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(h, CH_ERR_ARG, f + "workspace not 16-byte aligned");
    const size_t need = chk::jpeg_encode_workspace_bytes(N, H, W, C, subsampling);
    if (int rc = workspace_short(h, f.c_str(), workspace_bytes, need, "ch_jpeg_encode_workspace_bytes")) return rc;
    return launch(h, f.c_str(), [&] { return chk::jpeg_encode(img, N, H, W, C, quality, subsampling, out, sizes, workspace, hs(stream)); });
}

// ---- JPEG decoding (jpeg_decode.hip, jpeg_entropy_core.h) -------------------------------------------------------------------------------
namespace {
bool jpeg_dec_dims_ok(int H, int W, int C, int sampling) {
    return (C == 1 || C == 3) && sampling >= 0 && sampling <= (C == 3 ? 2 : 0) && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 &&
           (int64_t)H * W <= (1 << 30);
}
}  // namespace

size_t ch_jpeg_decode_workspace_bytes(int N, int H, int W, int C, int sampling) {
    return (N >= 1 && N <= 65535 && jpeg_dec_dims_ok(H, W, C, sampling)) ? chk::jpeg_decode_workspace_bytes(N, H, W, C, sampling) : 0;
}

namespace {
// ch_jpeg_decode (restart == nullptr) and ch_jpeg_decode_rst: one body, the entry's name in the messages
int jpeg_decode_entry(const char* entry, ch_handle* h, const uint8_t* streams, const int64_t* offsets, const uint8_t* tables, const uint32_t* restart,
                      int N, int H, int W, int C, int sampling, int rounds, uint8_t* img, int32_t* status, void* workspace, size_t workspace_bytes,
                      ch_stream_t stream) {
    namespace je = chk::jpegent;
    static_assert(CH_JPEG_DEC_OK == je::OK && CH_JPEG_DEC_BAD_CODE == je::BAD_CODE && CH_JPEG_DEC_BAD_INDEX == je::BAD_INDEX &&
                      CH_JPEG_DEC_INPUT_END == je::INPUT_END && CH_JPEG_DEC_BLOCKS == je::BLOCKS && CH_JPEG_DEC_NOT_SYNCED == je::NOT_SYNCED &&
                      CH_JPEG_DEC_TOO_LONG == je::TOO_LONG && CH_JPEG_DEC_MARKER == je::MARKER && CH_JPEG_DEC_RANGE == je::RANGE &&
                      CH_JPEG_DEC_RESTART == je::RESTART &&
                      CH_JPEG_DEC_TABLE_BYTES == je::TABLE_BYTES && CH_JPEG_DEC_DEFAULT_ROUNDS == je::DEFAULT_ROUNDS,
                  "constants of the header and of jpeg_entropy_core.h");
    if (!h) return CH_ERR_ARG;
    const std::string f = std::string(entry) + ": ";
    if (!streams || !offsets || !tables || !img || !status || !workspace) return fail(h, CH_ERR_ARG, f + "null pointer");
    if (N < 1 || N > 65535) return fail(h, CH_ERR_ARG, f + "N outside 1..65535");
    if (C != 1 && C != 3) return fail(h, CH_ERR_ARG, f + "C must be 1 (grey) or 3 (YCbCr -> RGB)");
    if (sampling < 0 || sampling > (C == 3 ? 2 : 0))
        return fail(h, CH_ERR_ARG, f + "sampling must be 0 (4:4:4), 1 (4:2:2) or 2 (4:2:0), and 0 for C = 1");
    if (rounds < 0 || rounds > je::MAX_ROUNDS) return fail(h, CH_ERR_ARG, f + "rounds outside 0..64");
    if (!jpeg_dec_dims_ok(H, W, C, sampling)) return fail(h, CH_ERR_ARG, f + "image too small or too large (sides 1..32768, H * W <= 2^30)");
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(h, CH_ERR_ARG, f + "workspace not 16-byte aligned");
    const size_t need = chk::jpeg_decode_workspace_bytes(N, H, W, C, sampling);
    if (int rc = workspace_short(h, f.c_str(), workspace_bytes, need, "ch_jpeg_decode_workspace_bytes")) return rc;
    return launch(h, f.c_str(), [&] {
        return chk::jpeg_decode(streams, offsets, tables, restart, N, H, W, C, sampling, rounds, img, status, workspace, hs(stream));
    });
}
}  // namespace

int ch_jpeg_decode(ch_handle* h, const uint8_t* streams, const int64_t* offsets, const uint8_t* tables, int N, int H, int W, int C, int sampling,
                   int rounds, uint8_t* img, int32_t* status, void* workspace, size_t workspace_bytes, ch_stream_t stream) {
    return jpeg_decode_entry("ch_jpeg_decode", h, streams, offsets, tables, nullptr, N, H, W, C, sampling, rounds, img, status, workspace,
                             workspace_bytes, stream);
}

int ch_jpeg_decode_rst(ch_handle* h, const uint8_t* streams, const int64_t* offsets, const uint8_t* tables, const uint32_t* restart, int N, int H,
                       int W, int C, int sampling, int rounds, uint8_t* img, int32_t* status, void* workspace, size_t workspace_bytes,
                       ch_stream_t stream) {
    if (h && !restart) return fail(h, CH_ERR_ARG, "ch_jpeg_decode_rst: null pointer");
    return jpeg_decode_entry("ch_jpeg_decode_rst", h, streams, offsets, tables, restart, N, H, W, C, sampling, rounds, img, status, workspace,
                             workspace_bytes, stream);
}

int ch_sean_set_tap(ch_handle* h, const char* name, float* dev_ptr) {
    if (!h || !name) return CH_ERR_ARG;
    if (dev_ptr) h->sean.taps[name] = dev_ptr;
    else h->sean.taps.erase(name);
    return CH_OK;
}

int ch_sean_scale_report(ch_handle* h, float* host_out, int n) {
    if (!h || !host_out || n < 0) return CH_ERR_ARG;
    if (!h->sean_ready || !h->sean.amax_slots) return fail(h, CH_ERR_STATE, "ch_sean_scale_report: SEAN weights not finalized");
    DeviceGuard guard(h->device);
    unsigned raw[64];
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(raw, h->sean.amax_slots, sizeof raw, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, CH_ERR_HIP, "ch_sean_scale_report: device read failed");
    for (int i = 0; i < n; ++i) {
        float v = 0.f;
        if (i < 64) std::memcpy(&v, &raw[i], 4);
        host_out[i] = v;
    }
    return CH_OK;
}

// a query, like ch_sean_noise_floats: the value is the result, -1 says that there is none (ch_last_error says why)
long long ch_sean_label_memo_stats(ch_handle* h) {
    if (!h) return -1;
    if (!h->sean_ready) {
        fail(h, CH_ERR_STATE, "ch_sean_label_memo_stats: SEAN weights not finalized");
        return -1;
    }
    DeviceGuard guard(h->device);
    int calls = 0, hits = 0;
    const std::string e = h->sean.label_memo_stats(&calls, &hits);
    if (!e.empty()) {
        fail(h, CH_ERR_HIP, "ch_sean_label_memo_stats: " + e);
        return -1;
    }
    return (long long)calls << 32 | (long long)(unsigned)hits;
}
long long ch_sean_spade_memo_stats(ch_handle* h) {
    if (!h) return -1;
    if (!h->sean_ready) {
        fail(h, CH_ERR_STATE, "ch_sean_spade_memo_stats: SEAN weights not finalized");
        return -1;
    }
    DeviceGuard guard(h->device);
    int stores = 0, loads = 0;
    const std::string e = h->sean.spade_memo_stats(&stores, &loads);
    if (!e.empty()) {
        fail(h, CH_ERR_HIP, "ch_sean_spade_memo_stats: " + e);
        return -1;
    }
    return (long long)stores << 32 | (long long)(unsigned)loads;
}
long long ch_sean_code_memo_stats(ch_handle* h) {
    if (!h) return -1;
    if (!h->sean_ready) {
        fail(h, CH_ERR_STATE, "ch_sean_code_memo_stats: SEAN weights not finalized");
        return -1;
    }
    DeviceGuard guard(h->device);
    int calls = 0, hits = 0;
    const std::string e = h->sean.code_memo_stats(&calls, &hits);
    if (!e.empty()) {
        fail(h, CH_ERR_HIP, "ch_sean_code_memo_stats: " + e);
        return -1;
    }
    return (long long)calls << 32 | (long long)(unsigned)hits;
}

int ch_sean_debug_read(ch_handle* h, void* host_out, size_t bytes) {
    if (!h || !host_out) return CH_ERR_ARG;
    if (!h->sean_ready || !h->sean.splitk_ws) return fail(h, CH_ERR_STATE, "ch_sean_debug_read: SEAN weights not finalized");
    DeviceGuard guard(h->device);
    if ((long long)bytes > h->sean.splitk_cap * 4) return fail(h, CH_ERR_ARG, "ch_sean_debug_read: too many bytes");
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host_out, h->sean.splitk_ws, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return fail(h, CH_ERR_HIP, "ch_sean_debug_read: device read failed");
    return CH_OK;
}

}  // extern "C"

namespace {
// ch_set_option: one row per key.  `frozen_by`: the model whose ch_finalize freezes the key (NEVER: live at any time).  The value
// goes through `map` (BOOL: value != 0; CLAMP: into [lo, hi]; RAW) into `set`; a `guard`, where a key has one, may refuse it first.
enum OptFreeze { NEVER, BY_SEAN, BY_SHAPE, BY_BISENET };
enum OptMap { BOOL, CLAMP, RAW };
struct OptRow {
    const char* key;
    OptFreeze frozen_by;
    OptMap map;
    int lo, hi;                          // CLAMP only
    void (*set)(ch_handle*, int);
    int (*guard)(ch_handle*, int);       // CH_OK, or the status to return
};
constexpr int MAXI = 0x7fffffff;
#define OPT_FIELD(field) [](ch_handle* h, int v) { h->field = v; }, nullptr
#define SEAN_FIELD(field) OPT_FIELD(sean.opt.field)

int guard_sparse(ch_handle* h, int value) {
    // after ch_finalize the reduction can be switched OFF (and back on); a handle finalised without it has no classification
    // buffers, and turning it on would silently do nothing
    if (h->sean_ready && value != 0 && !h->sean.gtab)
        return fail(h, CH_ERR_STATE, "ch_set_option(sean.sparse = 1): the handle was finalised with sean.sparse = 0 (no buffers); set it before ch_finalize");
    return CH_OK;
}
int guard_dbg(ch_handle* h, int value) {
#ifndef CH_ABLATE
    if (value & CH_ABLATE_DBG_MASK)
        return fail(h, CH_ERR_ARG, "ch_set_option(sean.dbg): timing-ablation / superseded-kernel bits need a library built with -DCH_ABLATE "
                                   "(make -C ctrlhair_amd/csrc ABLATE=1)");
#endif
    return CH_OK;
}

const OptRow OPTION_TABLE[] = {
    // 0 exact f32 | 1 f16x3 split operands (f32-class) | 2 single-term f16 operands | 3 single-term bf16 operands
    {"sean.f16x3", BY_SEAN, RAW, 0, 0, [](ch_handle* h, int v) { h->sean.opt.use_sh16 = v != 0; h->sean.opt.terms = v == 2 ? 1 : (v == 3 ? 2 : 3); }, nullptr},
    {"shape.f16x3", BY_SHAPE, BOOL, 0, 0, OPT_FIELD(shape.use_sh16)},
    {"shape.overlap", BY_SHAPE, BOOL, 0, 0, OPT_FIELD(shape.overlap)},       // 1 = the hair encoder / decoder on a side stream beside the face one (default), 0 = one after the other
    {"shape.enc_lut", BY_SHAPE, BOOL, 0, 0, OPT_FIELD(shape.enc_l0_lut)},    // exact-f32 shape encoders: 1 = layer 0 as a label table (default), 0 = through the conv kernel
    {"bisenet.f16x3", BY_BISENET, BOOL, 0, 0, OPT_FIELD(bisenet.use_sh16)},
    // exact-f32 kernels of the shape VAE / BiSeNet: 3x3 stride-1 convs as Winograd F(2x2,3x3) (default 1)
    {"aux.wino", NEVER, BOOL, 0, 0, [](ch_handle* h, int v) { h->shape.wino = h->bisenet.wino = v; }, nullptr},
    // run-ahead mode up to `value` images of 512x512 per chunk (0 = off)
    {"sean.ahead", BY_SEAN, RAW, 0, 0, [](ch_handle* h, int v) { h->sean.opt.ahead_pixels = (long long)v * 512 * 512; }, nullptr},
    // exact-f32 path: 3x3 convs as Winograd on the f32 matrix cores (conv_wino.h): 1 = F(2x2,3x3); 2 = + the ResBlock convs as F(4x4,3x3) (default)
    {"sean.wino", BY_SEAN, CLAMP, 0, 2, SEAN_FIELD(wino)},
    {"sean.lut_grouped", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(lut_grouped)},      // exact-f32 path: 1 = the style LUTs of a chunk from one grouped GEMM launch (default)
    // exact-f32 Winograd path, handles beyond the run-ahead sizes: 1 = the label / code-only products of the ACEs from grouped launches at the start
    // of a chunk (default; off by itself with sean.f16x3, sean.overlap or while profiling is enabled), 0 = every ACE launches its own, inline
    {"sean.prologue", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(prologue)},
    // handles with the ACE prologue: 1 = the label-only products of a chunk stay on the device and their launches return at once while the calls
    // bring the same label maps (default; sean_model.h memo_state), 0 = no memo: every call rebuilds them
    {"sean.label_memo", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(label_memo)},
    // with the label memo, styled ACEs on the F(4x4) V route: 1 = the accumulators after the hidden k-steps are kept and a call with the same label
    // maps runs the style k-steps only (default; sean_model.h memo_acc), 0 = launch for launch as without it
    {"sean.spade_memo", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(spade_memo)},
    // handles with the grouped style-LUT launch: 1 = the projections and the style LUTs stay on the device and their two launches return at once
    // while the calls bring the same style codes (default; sean_model.h code_state), 0 = no memo: every call rebuilds them
    {"sean.code_memo", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(code_memo)},
    {"sean.overlap", BY_SEAN, CLAMP, 0, MAXI, SEAN_FIELD(overlap)},        // CUs of the side streams of the overlap mode (sean_model.h), 0 = off
    {"sean.wino4_force", NEVER, BOOL, 0, 0, SEAN_FIELD(wino4_force)},        // 1 = F(4x4,3x3) wherever the shape allows, even with fewer tasks than CUs (tests / measurements)
    {"sean.patch", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(patch)},                  // 1 = pre-gathered hidden-activation patches for levels with few boundary quads (default), 0 = planes only
    {"sean.convt_gemm", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(convt_gemm)},        // exact-f32 Zencoder: 1 = the ConvTranspose as four phase GEMMs over shifted views (default), 0 = four Winograd phase convs
    {"sean.edge", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(edge)},                    // 1 = straight-edge pixels from per-code table rows in the interior pass (default), 0 = through the boundary conv
    {"sean.frame", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(frame)},                  // with sean.edge, exact-f32 Winograd path: 1 = frame pixels with a uniform in-image window from table rows too (default), 0 = boundary conv
    {"sean.int_groups", NEVER, CLAMP, 0, MAXI, SEAN_FIELD(int_groups)},      // channel groups per block of the four-pixel interior pass: 0 = chosen per launch (default), n >= 1 = at most n
    {"sean.int_onepass", NEVER, BOOL, 0, 0, SEAN_FIELD(int_onepass)},        // four-pixel interior pass: 1 = 128 code slots per block, one round up to 128 codes (default), 0 = 64 slots and rounds
    // exact-f32 path: 1 = 64-row wave tiles of the 1x1 GEMM kernel, transposed fc_mu reduction, one-thread-per-(row, label) style pack (default), 0 = round 11's kernels
    {"sean.pw_wide", NEVER, BOOL, 0, 0, SEAN_FIELD(pw_wide)},
    {"sean.batch_invariant", NEVER, BOOL, 0, 0, SEAN_FIELD(batch_inv)},      // exact-f32 path: 1 = kernel choices independent of the batch size of a call (default 0)
    {"sean.wino4v", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(wino4v)},                // 1 = pre-transformed-input route of the F(4x4,3x3) layers with many GEMM rows (conv_wino4v.h; default), 0 = off
    // plain F(4x4,3x3) convs on the position-split kernel (conv_wino4_split.h): 0 = never, 1 = wherever supported, < 0 = per shape (default)
    {"sean.wino4_split", BY_SEAN, CLAMP, -1, 1, SEAN_FIELD(wino4_split)},
    {"sean.wino4_ace", BY_SEAN, CLAMP, 0, MAXI, SEAN_FIELD(wino4_ace_max_r)},    // largest level (pixels) whose SPADE convs run as F(4x4,3x3) over every tile; 0 = none
    {"sean.hidden_wq", NEVER, BOOL, 0, 0, SEAN_FIELD(hidden_wq)},            // Winograd ACE path: 1 = hidden activations + one-hot planes from spade_hidden_wq (default)
    {"sean.wino_gather", BY_SEAN, BOOL, 0, 0, SEAN_FIELD(wino_gather)},      // 1 = gather mode of the Winograd ACE kernel (default), 0 = tile mode
    {"sean.wino_th", BY_SEAN, RAW, 0, 0, SEAN_FIELD(wino_th)},               // tile height 16 / 32 of the Winograd ACE kernel (0 = chosen per level)
    // exact SPADE-interior reduction (ace_sparse.h); buffers are sized at ch_finalize
    {"sean.sparse", NEVER, BOOL, 0, 0, [](ch_handle* h, int v) { h->sean.opt.sparse = v; }, guard_sparse},
    {"sean.sh16_compact", BY_SEAN, CLAMP, 0, 2, SEAN_FIELD(sh16_compact)},   // f16x3 path: pixel-level compaction (1) or tile skipping only (0); 2: without pair entries (A/B)
    {"sean.sparse_th", BY_SEAN, RAW, 0, 0, SEAN_FIELD(sparse_th)},           // tile height of the compaction: 8 / 16, 0 = chosen per layer
    {"sean.sparse_min", BY_SEAN, RAW, 0, 0, SEAN_FIELD(sparse_min_r)},       // smallest ACE resolution served by the sparse path
    {"sean.dbg_sel", NEVER, RAW, 0, 0, SEAN_FIELD(dbg_sel)},                 // index of the ACE launch that sean.dbg bit 256 cycle-stamps
    {"sean.dbg", NEVER, RAW, 0, 0, [](ch_handle* h, int v) { h->sean.opt.dbg = v; }, guard_dbg},      // profiling switches (dbg_bits.h)
};
#undef SEAN_FIELD
#undef OPT_FIELD
}  // namespace

extern "C" {

int ch_set_option(ch_handle* h, const char* key, int value) {
    if (!h || !key) return CH_ERR_ARG;
    for (const OptRow& r : OPTION_TABLE) {
        if (std::strcmp(key, r.key) != 0) continue;
        const bool frozen = r.frozen_by == BY_SEAN ? h->sean_ready : r.frozen_by == BY_SHAPE ? h->shape.ready : r.frozen_by == BY_BISENET && h->bisenet.ready;
        if (frozen) return fail(h, CH_ERR_STATE, std::string("ch_set_option(") + key + ") must precede ch_finalize");
        if (int rc = r.guard ? r.guard(h, value) : CH_OK) return rc;
        r.set(h, r.map == BOOL ? value != 0 : (r.map == CLAMP ? std::max(r.lo, std::min(r.hi, value)) : value));
        ++h->sean.memo_epoch;      // (label memo: what an earlier call left on the device was built under other options)
        return CH_OK;
    }
    return fail(h, CH_ERR_ARG, std::string("unknown option '") + key + "'");
}

int ch_mfma_peak(ch_handle* h, int kind, int ms_target, double* tflops) {
    if (!h || !tflops || kind < 0 || kind > 1 || ms_target < 1 || ms_target > 2000) return fail(h, CH_ERR_ARG, "ch_mfma_peak: bad argument");
    return launch(h, "ch_mfma_peak: ", [&] { return chk::mfma_peak(kind, ms_target, tflops, nullptr); });
}

int ch_profile_enable(ch_handle* h, int on) {
    if (!h) return CH_ERR_ARG;
    h->sean.prof_on = on != 0;
    return CH_OK;
}

int ch_profile_read(ch_handle* h, int kind, int* launches, double* total_ms, double* flops, double* bytes) {
    return ch_profile_read_ex(h, kind, launches, total_ms, flops, nullptr, bytes);
}

int ch_profile_read_ex(ch_handle* h, int kind, int* launches, double* total_ms, double* flops, double* flops_executed,
                       double* bytes) {
    if (!h) return CH_ERR_ARG;
    DeviceGuard guard(h->device);
    int n = 0;
    double ms = 0, fl = 0, fx = 0, by = 0;
    for (auto& r : h->sean.prof) {
        if (hipEventSynchronize(r.e1) != hipSuccess) return fail(h, CH_ERR_HIP, "hipEventSynchronize failed");
        if (kind < 0 || r.kind == kind) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) return fail(h, CH_ERR_HIP, "hipEventElapsedTime failed");
            ms += t;
            fl += r.flops;
            if (r.sp_stat) {        // sparse ACE launch: the matrix cores ran over the compacted boundary sub-tiles only
                int st[4] = {0, 0, 0, 0};
                if (hipMemcpy(st, r.sp_stat, sizeof st, hipMemcpyDeviceToHost) != hipSuccess)
                    return fail(h, CH_ERR_HIP, "ch_profile_read: work-list statistics read failed");
                fx += (double)st[3] * r.sp_flops_unit;
                by += r.sp_bytes_fixed + r.sp_bytes_px * (r.kind == 3 ? r.sp_npix - (double)st[1] : (double)st[1]);
            } else {
                fx += r.flops_exec >= 0.0 ? r.flops_exec : r.flops;
                by += r.bytes;
            }
            ++n;
        }
    }
    if (flops_executed) *flops_executed = fx;
    if (kind < 0) {      // records are consumed only by a read with kind < 0 (read specific kinds first)
        for (auto& r : h->sean.prof) {
            h->sean.ev_pool.push_back(r.e0);
            h->sean.ev_pool.push_back(r.e1);
        }
        h->sean.prof.clear();
        h->sean.prof_stats_used = 0;
    }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    if (flops) *flops = fl;
    if (bytes) *bytes = by;
    return CH_OK;
}

}  // extern "C"
