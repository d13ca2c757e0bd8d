// linear_tap.h -- one axis of cv2.resize(INTER_LINEAR) on uint8 data, shared by color_stats.hip (ch_resize_linear_u8) and ingest.hip
// (ch_ingest_images, mode 1).  Device only.
#pragma once
#include <hip/hip_runtime.h>

namespace chk {

// One axis of hostutil._linear_taps: f = (i + 0.5) * (n_in / n_out) - 0.5 in double (no contraction: the host rounds the
// product and the difference separately), floor, fraction rounded to f32, zero fraction at clamped taps, 11-bit weights
// rint(f * 2048) and rint((1 - f) * 2048) in f32.
__device__ __forceinline__ void linear_tap(int i, int n_out, int n_in, int& i0, int& i1, int& w0, int& w1) {
#pragma clang fp contract(off)
    const double scale = (double)n_in / (double)n_out;
    const double fd = ((double)i + 0.5) * scale - 0.5;
    const double fl = floor(fd);
    int k = (int)fl;
    float f = (float)(fd - fl);
    if (k < 0 || k >= n_in - 1) f = 0.f;
    k = k < 0 ? 0 : (k > n_in - 1 ? n_in - 1 : k);
    i0 = k;
    i1 = k + 1 < n_in - 1 ? k + 1 : n_in - 1;
    w1 = (int)rintf(f * 2048.f);
    w0 = (int)rintf((1.f - f) * 2048.f);
}

}  // namespace chk
