// face_unalign.hip -- paste N edited FFHQ-aligned crops back into the photo they were aligned from (the inverse of face_align.hip's
// geometry; the reference stops at the crop, so there is no upstream arithmetic to restate: DESIGN.md, "Paste-back").
//
// Per photo pixel (X, Y) of the quad's bounding box and per edit n:
//   (x, y) = A (X + 0.5, Y + 0.5, 1)                    crop coordinates, float64, left to right, no fused multiply-add
//   alpha  = clamp(min(x, S - x, y, S - y) / feather, 0, 1) [* bilinear(weight)(x, y) / 255]
//   e      = Lanczos-3 resample of the edit at (x, y) with filter scale fs = max(1, s): taps |i + 0.5 - x| < 3 fs, those outside
//            [0, S) dropped and the rest renormalised (Pillow's border rule); float32
//   out    = clamp(floor(alpha e + (1 - alpha) p + 0.5), 0, 255)
// The tap weights differ from pixel to pixel (the map is rotated) but are separable inside one pixel: each thread keeps its x weights
// in its own LDS column (tap-major, so a wave reads 64 consecutive floats: no bank conflict), evaluates one y weight per tap row and
// accumulates weighted row sums.  No barrier, no atomics, one workgroup per 32 x 8 tile and edit.
// Everything outside the bounding box is copied from the photo by copy_outside_kernel, 16 bytes per thread where the sizes allow.
// The geometry, the resample and the copy are shared with face_matte.hip: face_unalign_dev.h.
#include "face_unalign_dev.h"

namespace chk {
namespace {

using namespace unalign;

__device__ __forceinline__ float weight_bilinear(const uint8_t* __restrict__ w, int S, float x, float y) {
    const float u = x - 0.5f, v = y - 0.5f;
    const float fu = floorf(u), fv = floorf(v);
    const float du = u - fu, dv = v - fv;
    const int i0 = min(max((int)fu, 0), S - 1), i1 = min(max((int)fu + 1, 0), S - 1);
    const int j0 = min(max((int)fv, 0), S - 1), j1 = min(max((int)fv + 1, 0), S - 1);
    const float a = (float)w[(size_t)j0 * S + i0], b = (float)w[(size_t)j0 * S + i1];
    const float c = (float)w[(size_t)j1 * S + i0], d = (float)w[(size_t)j1 * S + i1];
    const float top = a + (b - a) * du, bot = c + (d - c) * du;
    return (top + (bot - top) * dv) * (1.0f / 255.0f);
}

__global__ __launch_bounds__(BLK) void face_unalign_kernel(const uint8_t* __restrict__ photo, const uint8_t* __restrict__ edits,
                                                           const uint8_t* __restrict__ weight, UnalignGeom g, uint8_t* __restrict__ out) {
    extern __shared__ float wx_lds[];                 // [nt][BLK]
    const int tid = threadIdx.y * TW + threadIdx.x;
    const int X = g.x0 + blockIdx.x * TW + threadIdx.x, Y = g.y0 + blockIdx.y * TH + threadIdx.y;
    if (X >= g.x1 || Y >= g.y1) return;
    const int n = blockIdx.z;
    const size_t pix = ((size_t)Y * g.W + X) * 3;
    const uint8_t* p = photo + pix;
    uint8_t* o = out + (size_t)n * g.H * g.W * 3 + pix;
    const uint8_t p0 = p[0], p1 = p[1], p2 = p[2];

    double x, y;
    crop_xy(g, X, Y, x, y);
    float alpha = border_ramp(g, x, y);
    if (alpha > 0.0f && weight) alpha *= weight_bilinear(weight, g.S, (float)x, (float)y);
    if (!(alpha > 0.0f)) {                            // outside the quad, or weight 0: the photo, untouched
        o[0] = p0, o[1] = p1, o[2] = p2;
        return;
    }
    resample_composite(g, edits, n, x, y, alpha, p0, p1, p2, o, wx_lds, tid);
}

}  // namespace

hipError_t face_unalign(const uint8_t* photo, const uint8_t* edits, const uint8_t* weight, const UnalignPlan& p, int H, int W, int N,
                        double feather_px, uint8_t* out, hipStream_t s) {
    const UnalignGeom g = make_geom(p, H, W, N, feather_px);
    copy_outside(photo, out, g, s);
    return launch_composite(face_unalign_kernel, photo, edits, weight, g, out, s);
}

}  // namespace chk
