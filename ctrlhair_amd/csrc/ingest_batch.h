// ingest_batch.h -- the batch of ch_ingest_images / ch_ingest_labels (include/ctrlhair_hip.h) and its check.  Host code without any HIP
// in it: ch_api.cpp runs ingest_check on every batch before ingest.hip launches anything, and tools/ingest_check_host.cpp runs the same
// function on the CPU under sanitizers over batches that lie.  Whatever passes here holds for the kernels: every table lies inside
// the batch, is the one of its image's size, and every tap range [first, first + count) lies inside the image.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace chk {

constexpr int INGEST_MAX_SIDE = 32768;        // source sides
constexpr int INGEST_MAX_OUT = 4096;          // P and S
enum { INGEST_PIL = 0, INGEST_CV2 = 1, INGEST_LABELS = 2 };      // == CH_INGEST_*
struct IngestImage {                          // one descriptor, 32 bytes
    uint64_t src;                             // device address of the pixels, [H][W][3] (labels: [H][W])
    int32_t H, W;
    int32_t htab, vtab;                       // int32 offset of the pass's table in the batch; -1: the pass is skipped
    int64_t inter;                            // the library's: byte offset of the image's [H][P][3] intermediate behind the batch's copy
};
static_assert(sizeof(IngestImage) == 32, "descriptor layout");

inline size_t ingest_up256(size_t v) { return (v + 255) & ~(size_t)255; }

// "" or what is wrong with the table at int32 offset `at` of the batch (`words` int32 long): {in, out, ksize, layout} | bounds [out][2] |
// k [out * ksize]
inline std::string ingest_check_table(const int32_t* b32, size_t words, int32_t at, int in, int out, int layout) {
    if (at < 0 || (at & 3) || (size_t)at + 4 > words) return "table offset outside the batch or not a multiple of 4";
    const int32_t* t = b32 + at;
    if (t[0] != in || t[1] != out || t[3] != layout) return "table is not the one of this image's (in, out) pair and pass";
    const int ksize = t[2];
    if (ksize < 1 || ksize > 2 * INGEST_MAX_SIDE + 1) return "table ksize out of range";
    if ((size_t)at + 4 + (size_t)out * 2 + (size_t)out * (size_t)ksize > words) return "table runs past the end of the batch";
    for (int i = 0; i < out; ++i) {
        const int first = t[4 + 2 * i], count = t[4 + 2 * i + 1];
        if (first < 0 || count < 1 || count > ksize || first > in - count) return "table taps outside the image";
    }
    return "";
}

// "" and the workspace bytes of the call (the batch's device copy, then mode 0's intermediates), or what is wrong with the batch
inline std::string ingest_check(const void* batch, size_t batch_bytes, int N, int P, int mode, size_t& ws_bytes) {
    ws_bytes = 0;
    if (!batch) return "null batch";
    if (N < 1 || N > 65535) return "N outside [1, 65535]";
    if (P < 1 || P > INGEST_MAX_OUT) return "output side outside [1, " + std::to_string(INGEST_MAX_OUT) + "]";
    if (mode != INGEST_PIL && mode != INGEST_CV2 && mode != INGEST_LABELS) return "mode is not 0 or 1";
    if (reinterpret_cast<uintptr_t>(batch) % 8 != 0 || batch_bytes % 16 != 0 || batch_bytes < sizeof(IngestImage) * (size_t)N)
        return "batch not 8-byte aligned, not a multiple of 16 bytes, or shorter than N descriptors";
    const IngestImage* d = static_cast<const IngestImage*>(batch);
    const int32_t* b32 = static_cast<const int32_t*>(batch);
    const size_t words = batch_bytes / 4;
    size_t inter = 0;
    for (int n = 0; n < N; ++n) {
        const std::string at = "image " + std::to_string(n) + ": ";
        if (!d[n].src) return at + "null address";
        if (d[n].H < 1 || d[n].W < 1 || d[n].H > INGEST_MAX_SIDE || d[n].W > INGEST_MAX_SIDE)
            return at + "side outside [1, " + std::to_string(INGEST_MAX_SIDE) + "]";
        const bool need_h = mode == INGEST_PIL && d[n].W != P, need_v = mode == INGEST_PIL && d[n].H != P;
        if (need_h != (d[n].htab >= 0) || need_v != (d[n].vtab >= 0))
            return at + "a table where the pass is skipped, or none where it runs (a pass runs in mode 0 when the size changes)";
        if (need_h) {
            const std::string why = ingest_check_table(b32, words, d[n].htab, d[n].W, P, 1);
            if (!why.empty()) return at + "horizontal " + why;
            inter += ingest_up256((size_t)d[n].H * P * 3);
        }
        if (need_v) {
            const std::string why = ingest_check_table(b32, words, d[n].vtab, d[n].H, P, 0);
            if (!why.empty()) return at + "vertical " + why;
        }
    }
    ws_bytes = ingest_up256(batch_bytes) + inter;
    return "";
}

}  // namespace chk
