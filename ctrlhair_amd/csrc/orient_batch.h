// orient_batch.h -- the batch of ch_orient_u8 (include/ctrlhair_hip.h) and its check.  Host code without any HIP in it: ch_api.cpp runs
// orient_check on every batch before orient.hip launches anything, and tools/orient_check_host.cpp runs the same function on the CPU
// under sanitizers over batches that lie.  Whatever passes here holds for the kernel: every image's H * W * C bytes lie inside the
// destination buffer at its offset, no two images share a destination byte, and no source range touches the destination buffer.
// The sources are addressed by pointer, as in ingest_batch.h: their extents are the caller's word, only null and aliasing are refused.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace chk {

constexpr int ORIENT_MAX_SIDE = 32768;
constexpr int ORIENT_TILE = 64;               // pixels per side of the tile one workgroup turns
struct OrientImage {                          // one descriptor, 32 bytes
    uint64_t src;                             // device address of the stored pixels, [H][W][C]
    int64_t dst;                              // byte offset of the upright pixels in the destination buffer: [H][W][C], orientations 5..8 [W][H][C]
    int32_t H, W, C;                          // of the STORED image; C is 1, 3 or 4
    int32_t orient;                           // EXIF orientation 1..8 (1: a copy)
};
static_assert(sizeof(OrientImage) == 32, "descriptor layout");

inline size_t orient_up256(size_t v) { return (v + 255) & ~(size_t)255; }

// tiles (= workgroups) of one image
inline unsigned orient_tiles(int H, int W) {
    return (unsigned)((H + ORIENT_TILE - 1) / ORIENT_TILE) * (unsigned)((W + ORIENT_TILE - 1) / ORIENT_TILE);
}

// "" and the workspace bytes of the call (the descriptors' device copy), or what is wrong with the batch.  dst_addr: the destination
// buffer's device address, 0 when it is not known yet (the size query): the aliasing test is then left to the entry itself.
inline std::string orient_check(const void* batch, size_t batch_bytes, int N, uint64_t dst_addr, size_t dst_bytes, size_t& ws_bytes) {
    ws_bytes = 0;
    if (!batch) return "null batch";
    if (N < 1 || N > 65535) return "N outside [1, 65535]";
    if (reinterpret_cast<uintptr_t>(batch) % 8 != 0 || batch_bytes != sizeof(OrientImage) * (size_t)N)
        return "batch not 8-byte aligned, or not N descriptors long";
    if (dst_addr && dst_addr + dst_bytes < dst_addr) return "destination buffer wraps around the address space";
    const OrientImage* d = static_cast<const OrientImage*>(batch);
    uint64_t end = 0;                         // first free destination byte: the images lie in the buffer in ascending order
    for (int n = 0; n < N; ++n) {
        const std::string at = "image " + std::to_string(n) + ": ";
        if (!d[n].src) return at + "null address";
        if (d[n].H < 1 || d[n].W < 1 || d[n].H > ORIENT_MAX_SIDE || d[n].W > ORIENT_MAX_SIDE)
            return at + "side outside [1, " + std::to_string(ORIENT_MAX_SIDE) + "]";
        if (d[n].C != 1 && d[n].C != 3 && d[n].C != 4) return at + "C is not 1, 3 or 4";
        if (d[n].orient < 1 || d[n].orient > 8) return at + "orientation outside [1, 8]";
        uint64_t bytes = 0;                   // 2^15 * 2^15 * 4 fits, but the check does not lean on the limits above
        if (__builtin_mul_overflow((uint64_t)d[n].H, (uint64_t)d[n].W, &bytes) || __builtin_mul_overflow(bytes, (uint64_t)d[n].C, &bytes))
            return at + "H * W * C overflows";
        if (d[n].dst < 0 || (uint64_t)d[n].dst > dst_bytes || bytes > dst_bytes - (uint64_t)d[n].dst)
            return at + "destination offset or extent outside the destination buffer";
        if ((uint64_t)d[n].dst < end) return at + "destination overlaps the image before it (offsets must ascend)";
        end = (uint64_t)d[n].dst + bytes;
        if (d[n].src + bytes < d[n].src) return at + "source wraps around the address space";
        if (dst_addr && d[n].src < dst_addr + dst_bytes && dst_addr < d[n].src + bytes) return at + "source lies inside the destination buffer";
    }
    ws_bytes = orient_up256(batch_bytes);
    return "";
}

}  // namespace chk
