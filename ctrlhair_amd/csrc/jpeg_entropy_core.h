// jpeg_entropy_core.h -- every address decision of the JPEG decoder's entropy stage (ch_jpeg_decode, jpeg_decode.hip), compilable for the
// host: tools/jpeg_entropy_host.cpp runs the same subsequence / round scheme serially under AddressSanitizer and
// UndefinedBehaviorSanitizer.  Here: the bit reader with unstuffing, the Huffman tables, the symbol step, the state that one subsequence
// hands to the next, and where a coefficient goes.
//
// A scan is cut into subsequences of SUBSEQ bytes, one lane each; LANES of them are a chunk, one workgroup, which keeps its CHUNK bytes
// plus MARGIN in LDS (a Window).  A decoder state is (bit position in the stuffed bytes, block index within the MCU, zigzag index).  The
// position never rests on a stuffing byte (a 0x00 behind a data 0xFF): the reader skips it when it steps over it.  Lane 0 of a stream
// knows its state; every other lane starts from guess(): "a block begins at my first byte".  run_subseq() decodes from an entry state up
// to the first symbol that starts at or beyond the subsequence's end and returns the exit state and the blocks completed.  A lane that
// meets an invalid code or a coefficient index past 63 exits with pos = INVALID and the reason in bz: an error only if it survives as
// the true state (chain_break()).
//
// Restart intervals (a stream with Ri > 0 MCUs per interval; the RST instantiations below).  Data bits end at an RSTm marker (0xFF 0xD0..D7).
// A state whose next symbol does not fit into the bits before a marker continues from the state every decoder has behind that marker,
// whatever state it was: (the byte after it, block 0, zigzag 0, FRESH).  So wrong guesses converge at the first marker.  Whether a jump
// was legal -- it follows the block that completes MCU k * Ri, fewer than 8 bits (the padding, dropped unread as libjpeg drops it) lay
// before the marker, its number is (k - 1) mod 8 -- and whether a symbol was read where a marker was due is judged where the absolute
// block ordinals are known and only on the true chain (RstAudit, the write pass).  A lane does not know its ordinals, so it cannot drop
// the padding by count as libjpeg does: padding that reads as a whole symbol -- possible only with a Huffman table that assigns the
// all-ones code, which T.81 forbids -- is a symbol read where a marker was due, RESTART.  FRESH marks "no symbol since the marker": two
// markers back to back are two jumps, the second from a FRESH state.  With Ri == 0 none of this is compiled into the path taken.
//
// Bounds: a Window reads as zero outside its bytes, whatever index is asked; every step consumes at least one bit, so a subsequence
// takes at most 8 * SUBSEQ + 40 steps (and the loop counts them); a coefficient is stored only into a block below the image's block
// count.  Nothing here depends on the data being a valid stream.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JE_HD __host__ __device__ inline
#else
#define JE_HD inline
#endif

namespace chk {
namespace jpegent {

constexpr int SUBSEQ = 128;                // bytes per lane
constexpr int LANES = 64;                  // lanes per chunk (one wavefront)
constexpr int CHUNK = SUBSEQ * LANES;      // bytes per workgroup
constexpr int MARGIN = 16;                 // a step reads at most 10 bytes from the byte its position is in
constexpr int DEFAULT_ROUNDS = 8;          // launches of the hand-over between chunks when the caller passes 0
constexpr int MAX_ROUNDS = 64;
constexpr uint32_t MAX_STREAM = 1u << 28;  // bytes: bit positions are 32-bit
constexpr uint32_t INVALID = 0xFFFFFFFFu;
constexpr int FAST_BITS = 9;

// the per-image table block of ch_jpeg_decode: quantisers of the components in natural order, then per component its DC and its AC table
// as BITS[16] HUFFVAL[256]
constexpr int TABLE_BYTES = 2048, TABLE_QUANT = 0, TABLE_HUFF = 192, TABLE_HUFF_STRIDE = 272;

constexpr uint32_t FRESH = 1u << 16;       // in State::bz: directly behind a restart marker

enum Status { OK = 0, BAD_CODE = 1, BAD_INDEX = 2, INPUT_END = 3, BLOCKS = 4, NOT_SYNCED = 5, TOO_LONG = 6, MARKER = 7, RANGE = 8, RESTART = 9 };

struct State {
    uint32_t pos;                          // bit position in the stuffed bytes, or INVALID
    uint32_t bz;                           // block index within the MCU << 8 | zigzag index (0: the DC comes next), FRESH; INVALID: the Status
};
JE_HD bool same(State a, State b) { return a.pos == b.pos && a.bz == b.bz; }

struct SubState {                          // what one subsequence keeps between launches
    State entry, exit;
    uint32_t count;                        // blocks completed
};

struct Geometry {
    int bpm;                               // blocks per MCU: 1, 3, 4 or 6
    int luma;                              // of them luma: 1, 1, 2 or 4
    uint32_t nblocks;                      // of the whole scan
};
// MCUs per restart interval as the decoder uses it: 0 (no markers expected) when the interval holds the whole scan
JE_HD uint32_t effective_restart(const Geometry& g, uint32_t ri) { return ri < g.nblocks / (uint32_t)g.bpm ? ri : 0u; }
JE_HD int comp_of(const Geometry& g, uint32_t b) { return b < (uint32_t)g.luma ? 0 : (int)b - g.luma + 1; }

// sampling: 0 = 4:4:4 (and grey), 1 = 4:2:2, 2 = 4:2:0
JE_HD Geometry geometry(int H, int W, int C, int sampling) {
    const int hs = (C == 3 && sampling) ? 2 : 1, vs = (C == 3 && sampling == 2) ? 2 : 1;
    const uint32_t mw = (uint32_t)(W + 8 * hs - 1) / (8 * hs), mh = (uint32_t)(H + 8 * vs - 1) / (8 * vs);
    Geometry g;
    g.luma = hs * vs;
    g.bpm = C == 1 ? 1 : hs * vs + 2;
    g.nblocks = mw * mh * (uint32_t)g.bpm;
    return g;
}

struct Window {                            // bytes [base, base + len) of a stream at p; everything else reads as zero
    const uint8_t* p;
    uint32_t base, len;
};
JE_HD uint32_t byte_at(const Window& w, uint32_t i) {
    const uint32_t k = i - w.base;
    return k < w.len ? w.p[k] : 0u;
}

struct Huff {
    uint16_t fast[1 << FAST_BITS];         // length << 8 | symbol for codes of up to FAST_BITS bits, else 0
    int32_t maxcode[17];                   // [l]: the largest code of length l, -1 if there is none
    int32_t valoff[17];                    // [l]: index of the first symbol of length l minus its code
    uint8_t vals[256];
};

// Annex C from BITS; at most 256 symbols are counted whatever BITS says
JE_HD void build_codes(Huff& h, const uint8_t* bits) {
    int32_t code = 0, k = 0;
    h.maxcode[0] = -1;
    h.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        int32_t n = bits[l - 1];
        if (n > 256 - k) n = 256 - k;
        h.valoff[l] = k - code;
        k += n;
        code += n;
        h.maxcode[l] = n ? code - 1 : -1;
        code <<= 1;
    }
}

// the code at the top of the 16-bit window w among lengths lo..hi: length << 8 | symbol, or 0
JE_HD uint32_t slow_lookup(const Huff& h, uint32_t w, int lo, int hi) {
    for (int l = lo; l <= hi; ++l) {
        const int32_t c = (int32_t)(w >> (16 - l));
        if (c <= h.maxcode[l]) {
            const int32_t i = c + h.valoff[l];
            return (i >= 0 && i < 256) ? ((uint32_t)l << 8 | h.vals[i]) : 0u;      // outside only for BITS that are no prefix code
        }
    }
    return 0u;
}
JE_HD uint16_t fast_entry(const Huff& h, uint32_t e) { return (uint16_t)slow_lookup(h, e << (16 - FAST_BITS), 1, FAST_BITS); }
JE_HD uint32_t lookup(const Huff& h, uint32_t w) {
    const uint32_t f = h.fast[w >> (16 - FAST_BITS)];
    return f ? f : slow_lookup(h, w, FAST_BITS + 1, 16);
}

// natural index of zigzag position k
constexpr uint8_t NATURAL_OF[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
JE_HD int natural_of(int k) { return NATURAL_OF[k & 63]; }

struct NoSink {
    JE_HD void put(uint32_t, int, int) const {}
};
struct CoefSink {                          // coef: int16 [nblocks][64], natural order
    int16_t* coef;
    uint32_t nblocks;
    JE_HD void put(uint32_t blk, int natural, int v) const {
        if (blk < nblocks) coef[(uint64_t)blk * 64 + (uint32_t)(natural & 63)] = (int16_t)v;
    }
};

JE_HD State invalid(int why) { return State{INVALID, (uint32_t)why}; }
JE_HD bool is_rst(uint32_t byte) { return (byte & 0xF8u) == 0xD0u; }

// The jumps over restart markers on the true chain, judged against the absolute block ordinals (see the top).  rib: blocks per interval.
struct NoAudit {
    JE_HD bool due(State, uint32_t) const { return false; }
    JE_HD void stepped(bool) {}
    JE_HD void jumped(bool, uint32_t, uint32_t) {}
};
struct RstAudit {
    uint32_t rib, nblocks;
    bool bad;
    // a marker is due before the next symbol: the state is at the start of the MCU that begins an interval, and not behind a marker already
    JE_HD bool due(State s, uint32_t blk) const { return s.bz == 0 && blk > 0 && blk < nblocks && blk % rib == 0; }
    JE_HD void stepped(bool was_due) { bad |= was_due; }
    JE_HD void jumped(bool was_due, uint32_t info, uint32_t blk) { bad |= !was_due || (info & 8u) || (info & 7u) != ((blk / rib - 1) & 7u); }
};

// "a block begins at the first byte of subsequence i", not on a stuffing byte
JE_HD State guess(uint32_t i, uint32_t byte_before, uint32_t first_byte) {
    const uint32_t at = i * (uint32_t)SUBSEQ + ((i && byte_before == 0xFF && first_byte == 0) ? 1u : 0u);
    return State{at * 8, 0};
}
// the same in a stream with restart markers: a subsequence that begins on a marker's second byte begins behind the marker
JE_HD State guess_rst(uint32_t i, uint32_t byte_before, uint32_t first_byte) {
    if (i && byte_before == 0xFF && is_rst(first_byte)) return State{(i * (uint32_t)SUBSEQ + 1u) * 8, FRESH};
    return guess(i, byte_before, first_byte);
}

enum StepResult { STEPPED = 0, INPUT_ENDS = 1, DEAD = 2, JUMPED = 3 };

// One symbol from state s.  tables: the 6 Huff of the image (component * 2 + (AC ? 1 : 0)).  stream_len: bytes of the whole stream.
// blk: ordinal of the block s is in; advanced when the block completes.  INPUT_ENDS: the symbol is not whole before the stream ends (s
// unchanged); DEAD: s is set to invalid(reason).  RST: JUMPED: s is the state behind the restart marker that ended the data bits; info:
// the marker's number | 8 when the jump left 8 bits or more unread or came from a state that is not the start of an MCU (or is FRESH).
template <bool RST, class Sink>
JE_HD int step(const Huff* tables, const Geometry& g, const Window& w, uint32_t stream_len, State& s, uint32_t& blk, const Sink& sink,
               uint32_t& info) {
    const uint32_t b0 = s.pos >> 3, o = s.pos & 7;
    uint32_t mark = 8, mnum = 0, mend = 0;                                     // RST: the first marker's 0xFF is data byte `mark` (8: none)
    // 5 data bytes from b0 (40 bits); bit k of skipped: a stuffing byte lies between data bytes k - 1 and k
    uint32_t i = b0, prev = byte_at(w, i), skipped = 0, have = i < stream_len ? 1u : 0u;
    uint64_t v = prev;
    for (int k = 1; k <= 4; ++k) {
        ++i;
        uint32_t x = byte_at(w, i);
        if (prev == 0xFF && x == 0) {
            ++i;
            x = byte_at(w, i);
            skipped |= 1u << k;
        } else if (RST && prev == 0xFF && is_rst(x) && mark == 8) {
            mark = (uint32_t)k - 1, mnum = x & 7u, mend = i + 1;
        }
        have += i < stream_len ? 1u : 0u;
        v = v << 8 | x;
        prev = x;
    }
    if (RST) {
        if (mark == 8 && prev == 0xFF) {
            const uint32_t x = byte_at(w, i + 1);
            if (is_rst(x)) mark = 4, mnum = x & 7u, mend = i + 2;
        }
        if (mark < have) have = mark;
    }
    const uint32_t avail = have * 8 > o ? have * 8 - o : 0;                    // data bits from s.pos to the end of the data, up to 40 - o
    // RST: the jump a symbol that does not fit before a marker turns into; in order only from the start of an MCU over pad bits
    const State behind{mend * 8, FRESH};
    const uint32_t jump = mnum | ((avail >= 8 || s.bz != 0) ? 8u : 0u);
    const uint64_t top = v << (24 + o);                                        // the bits from s.pos at the top of 64
    const uint32_t bidx = (s.bz >> 8) & 255u, zz = s.bz & 255u;
    const int comp = comp_of(g, bidx);
    const uint32_t f = lookup(tables[comp * 2 + (zz ? 1 : 0)], (uint32_t)(top >> 48));
    if (!f) {
        if (avail < 16) {
            if (RST && mark < 8) {
                info = jump, s = behind;
                return JUMPED;
            }
            return INPUT_ENDS;
        }
        s = invalid(BAD_CODE);
        return DEAD;
    }
    const uint32_t len = f >> 8, sym = f & 255u;
    const uint32_t size = zz ? (sym & 15u) : sym;
    if (size > 15) {                                                           // a DC symbol that is no category
        s = invalid(BAD_CODE);
        return DEAD;
    }
    const uint32_t n = len + size;                                             // <= 31 <= 40 - o
    if (n > avail) {
        if (RST && mark < 8) {
            info = jump, s = behind;
            return JUMPED;
        }
        return INPUT_ENDS;
    }
    int val = 0;
    if (size) {
        const uint32_t raw = (uint32_t)((top << len) >> (64 - size));
        val = raw < (1u << (size - 1)) ? (int)raw - (int)(1u << size) + 1 : (int)raw;
    }
    uint32_t nzz;
    bool complete = false;
    if (!zz) {
        sink.put(blk, 0, val);
        nzz = 1;
    } else if (!size) {
        if ((sym >> 4) == 15) {
            nzz = zz + 16;
            if (nzz > 63) {
                s = invalid(BAD_INDEX);
                return DEAD;
            }
        } else {
            nzz = 0;
            complete = true;
        }
    } else {
        const uint32_t at = zz + (sym >> 4);
        if (at > 63) {
            s = invalid(BAD_INDEX);
            return DEAD;
        }
        sink.put(blk, natural_of((int)at), val);
        nzz = at + 1;
        if (nzz == 64) {
            nzz = 0;
            complete = true;
        }
    }
    uint32_t nb = bidx;
    if (complete) {
        ++blk;
        nb = bidx + 1 == (uint32_t)g.bpm ? 0 : bidx + 1;
    }
    const uint32_t k = (o + n) >> 3;                                           // <= 4: the data byte the new position is in
    const uint32_t mask = (2u << k) - 1;
    s.pos = (b0 + k + (uint32_t)__builtin_popcount(skipped & mask)) * 8 + ((o + n) & 7);
    s.bz = nb << 8 | nzz;
    return STEPPED;
}

// Subsequence [.., end_byte) from `entry`: every symbol (and every jump over a restart marker) that starts before end_byte.  first_blk:
// ordinal of the block `entry` is in.  RST: the stream has restart markers; audit: RstAudit where first_blk is the true ordinal, else NoAudit.
template <bool RST, class Sink, class Audit>
JE_HD void run_subseq(const Huff* tables, const Geometry& g, const Window& w, uint32_t stream_len, uint32_t end_byte, State entry,
                      uint32_t first_blk, const Sink& sink, Audit& audit, State& exit, uint32_t& count) {
    State s = entry;
    uint32_t blk = first_blk;
    if (s.pos != INVALID) {
        for (int steps = 0; steps < 8 * SUBSEQ + 40 && (s.pos >> 3) < end_byte; ++steps) {
            const bool due = audit.due(s, blk);
            uint32_t info = 0;
            const int r = step<RST>(tables, g, w, stream_len, s, blk, sink, info);
            if (r == STEPPED) audit.stepped(due);
            else if (RST && r == JUMPED) audit.jumped(due, info, blk);
            else break;
        }
    }
    exit = s;
    count = blk - first_blk;
}

// The entry of subsequence i > 0 given its predecessor's exit: that exit, or the lane's own guess when the predecessor died
JE_HD State entry_from(State prev_exit, State own_guess) { return prev_exit.pos == INVALID ? own_guess : prev_exit; }

// Is the chain broken between subsequence i - 1 and i?  0: no; else the Status it means for the stream when it is the first break
JE_HD int chain_break(State prev_exit, State entry) {
    if (prev_exit.pos == INVALID) return (int)prev_exit.bz;
    return same(prev_exit, entry) ? OK : NOT_SYNCED;
}

// Status of a stream whose chain is whole: `last` is the exit of its last subsequence, `blocks` the sum of the counts
JE_HD int final_status(State last, uint64_t blocks, const Geometry& g) {
    if (last.pos == INVALID) return (int)last.bz;
    if (blocks < g.nblocks) return INPUT_END;
    if (blocks == g.nblocks && last.bz == FRESH) return RESTART;               // a marker behind the last MCU
    if (blocks > g.nblocks || last.bz != 0) return BLOCKS;
    return OK;
}

}  // namespace jpegent
}  // namespace chk
