// dbg_bits.h -- every bit of option "sean.dbg" (SeanOptions::dbg, ConvParams::dbg) that the code reads.  Profiling and A/B switches only;
// 0 is the product.  The values are part of what tests, tools and bench.py --dbg pass as integers: a name may be added, a value never moves.
// Free bits: 16, 512, 1024, 32768, 262144, 524288, 8388608, and 536870912 upwards.
#pragma once

namespace chk {

enum Dbg : int {
    // ---- timing ablations: WRONG RESULTS, CH_ABLATE builds only ----
    DBG_SKIP_STAGING = 1,                 // conv_sh16 kernels: stage no chunk after the first (ws2: no patch loads after the first step)
    DBG_SKIP_MFMA = 2,                    // conv_sh16_kernel: skip the MFMA loop
    DBG_SKIP_EPILOGUE = 4,                // conv_sh16 kernels: skip the epilogue
    DBG_SKIP_FIRST_STAGE = 8,             // conv_sh16_kernel: do not stage the first chunk either
    DBG_NO_LUT_GATHER = 4194304,          // ACE epilogue: no style-LUT gathers
    // ---- route switches of the default build ----
    DBG_NO_FUSE_1X1 = 32,                 // f16x3 ResBlock: do not fuse the 1x1 shortcut conv into the 3x3 conv
    DBG_WS_FORCE = 64,                    // force the wave-specialised persistent conv kernel wherever it is eligible
    DBG_WS_OFF = 128,                     // never take the wave-specialised persistent conv kernel
    DBG_STAMP = 256,                      // cycle stamps of ACE launch "sean.dbg_sel" into the split-K workspace (tools/ws_timeline.py)
    DBG_NO_SIDE_STREAM = 4096,            // no run-ahead of the label- / code-only work on the side stream
    DBG_NO_LUT_AHEAD = 8192,              // no run-ahead of the style LUTs alone
    DBG_ZENC_ZEROINS = 16384,             // style encoder's ConvTranspose (f16 paths): 3x3 conv over the zero-inserted view, the earlier form
    DBG_F32_NEED_MAP = 131072,            // exact-f32 sparse route: the label-table kernel writes only the pixels the conv reads
    DBG_ONEHOT_NO_COMPACT = 33554432,     // f16 paths: need-masked label-table launches never take the compacting kernel
    DBG_NO_WORK_QUADS = 67108864,         // f16 paths: no task list of four row tiles per entry (decided at ch_finalize)
    DBG_INTERIOR_FILL128 = 134217728,     // exact-f32 tile4 interior pass: the earlier block fill rule (128 interior pixels) instead of whole lines
    DBG_INTERIOR_NO_SINGLE = 268435456,   // f16 / bf16 interior pass: not the single-term kernel
    // ---- superseded kernel versions kept for A/B measurements: CH_ABLATE builds only ----
    DBG_WS2 = 2048,                       // conv_sh16_ws2_kernel (conv_sh16_ws2.h) for the 128-channel ACE convs
    DBG_INTERIOR_VEC4 = 65536,            // exact-f32 interior pass, first version: four pixels per thread
    DBG_INTERIOR_SECTORS = 1048576,       // exact-f32 interior pass, first version: one pixel per thread, whole 32-byte sectors
    DBG_INTERIOR_ROWS = 2097152,          // interior pass: the row-shaped kernels of the first version (blocks of 256 consecutive pixels)
    DBG_INTERIOR_TILE4 = 16777216,        // exact-f32 sparse route: the four-pixels-per-thread tile kernel from 128 px on
};

}  // namespace chk

// the bits that need a library built with -DCH_ABLATE (make ABLATE=1): ch_set_option rejects them otherwise
constexpr int CH_ABLATE_DBG_MASK = chk::DBG_SKIP_STAGING | chk::DBG_SKIP_MFMA | chk::DBG_SKIP_EPILOGUE | chk::DBG_SKIP_FIRST_STAGE | chk::DBG_NO_LUT_GATHER |
                                   chk::DBG_WS2 | chk::DBG_INTERIOR_VEC4 | chk::DBG_INTERIOR_SECTORS | chk::DBG_INTERIOR_ROWS | chk::DBG_INTERIOR_TILE4;
static_assert(CH_ABLATE_DBG_MASK == 24184847, "sean.dbg values are part of the interface: tests, tools and bench.py pass them as integers");
