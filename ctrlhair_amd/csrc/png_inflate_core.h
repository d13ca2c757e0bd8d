// The serial half of the PNG decoder (ch_png_decode, include/ctrlhair_hip.h): a zlib stream (RFC 1950 / 1951) is turned, step by step, into
// TOKENS -- literals and (length, distance) matches with their destination -- and into stored-block copy jobs.  Everything that decides an
// address lives here: the zlib header, the block headers, the code-length parsing, the table construction, the symbol decode and the check
// of every token against the bytes produced so far and against the output bound.  The header is plain C++ (host-compilable: the sanitizer
// program tools/png_inflate_host.cpp runs it on the CPU); the kernel (png_decode.hip) runs step() on one lane and lets the whole wave copy
// the bytes of the tokens step() has checked.
//
// Conformance is that of stock zlib's inflate (not INFLATE_STRICT): the window size of CINFO is not enforced beyond 32768, bytes behind the
// Adler-32 are ignored, an empty stored block is legal anywhere, an incomplete code is legal where it is one single code of length 1
// (ch_png_encode_dist writes such a distance code), a distance code without any code is legal in a block without a match.
//
// Input is read through a WINDOW: bytes [base, end) of the stream (base a multiple of 4, the data 4-byte aligned).  step() asks for a
// window of STEP_INPUT bytes from the read position (or up to the stream's end) before it starts anything (NEED_INPUT otherwise), and no
// step consumes that much: a round of ROUND_TOKENS tokens takes at most 48 bits each, a dynamic block header at most 4554 bits.  A read
// past the window or past the stream yields zero bits, never a memory access; consuming a bit past the stream's end is INPUT_END.
// Termination: every token consumes at least one bit, every step a token, a header or a block.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define PNGINF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define PNGINF_HD inline
#endif

namespace chk {
namespace pnginf {

// == CH_PNG_DEC_* of include/ctrlhair_hip.h (static_assert in ch_api.cpp)
enum Status : int32_t {
    OK = 0, BAD_HEADER = 1, BAD_BLOCK = 2, BAD_CODE = 3, BAD_SYMBOL = 4, BAD_DISTANCE = 5, INPUT_END = 6, SIZE = 7, ADLER = 8, BAD_FILTER = 9
};

constexpr int ROUND_TOKENS = 128;          // tokens one step() decodes at most
constexpr int STEP_INPUT = 1024;           // bytes of window a step needs ahead of the read position (unless the window reaches the end)
constexpr int LIT_FAST = 10, DIST_FAST = 8;
constexpr uint32_t ADLER_MOD = 65521;

// what step() did
enum Result : int { NEED_INPUT = 0, TOKENS = 1, STORED = 2, CONTINUE = 3, DONE = 4 };

enum Phase : int { PH_ZLIB = 0, PH_BLOCK = 1, PH_CODES = 2, PH_TRAILER = 3, PH_DONE = 4 };

// len == 0: the literal byte `val` at rel; else a match of len 3..258 at distance val + 1 (1..32768); rel: destination - Round::out_start
struct Token {
    uint32_t rel;
    uint16_t len;
    uint16_t val;
};

struct Window {
    const uint8_t* data;       // byte i of the stream is data[i - base] for base <= i < end; 4-byte aligned
    uint64_t base, end;
};

struct Huffman {
    uint16_t lit_fast[1 << LIT_FAST];      // (code length << 9 | symbol) by the next LIT_FAST bits, 0: a longer code (or none)
    uint16_t dist_fast[1 << DIST_FAST];    // (code length << 9 | symbol), 0 likewise
    uint16_t lit_sym[288], dist_sym[32];   // the symbols in canonical order, for the count walk of the longer codes
    uint16_t lit_cnt[16], dist_cnt[16];
};

struct State {
    uint64_t in_len, in_pos;               // stream length; next byte the bit buffer takes (a multiple of 4 beyond `base`)
    uint64_t bitbuf;
    int32_t bitcnt;
    uint64_t out_pos, out_len;             // bytes produced, bytes expected (H * (1 + W * C))
    int32_t phase, final_block, status;
    uint32_t adler_stored;                 // the stream's Adler-32 (valid once phase == PH_DONE with status OK)
    // the result of the last step
    uint64_t out_start;                    // TOKENS: destination of rel 0; STORED: destination
    uint64_t src;                          // STORED: offset in the stream
    uint32_t count;                        // TOKENS: number of tokens; STORED: bytes
    uint8_t lens[320];                     // code lengths while a dynamic header is parsed
    uint8_t cl[19];                        // the code-length code: lengths, counts, symbols (arrays here, not locals: no scratch memory)
    uint16_t ccnt[16], csym[19], offs[16];
    Huffman h;
};

PNGINF_HD void init(State& s, uint64_t in_len, uint64_t out_len) {
    s.in_len = in_len;
    s.in_pos = 0;
    s.bitbuf = 0;
    s.bitcnt = 0;
    s.out_pos = 0;
    s.out_len = out_len;
    s.phase = PH_ZLIB;
    s.final_block = 0;
    s.status = OK;
    s.adler_stored = 0;
    s.out_start = s.src = 0;
    s.count = 0;
}

// ---- bit reader (locals of one step) -----------------------------------------------------------------------------------------------
struct Bits {
    uint64_t buf;
    int32_t cnt;
    uint64_t pos;              // next byte to take, (pos - base) % 4 == 0
};

PNGINF_HD uint32_t window_word(const Window& w, uint64_t pos) {
    if (pos >= w.base && pos + 4 <= w.end) {
        uint32_t v;
        memcpy(&v, __builtin_assume_aligned(w.data + (pos - w.base), 4), 4);
        return v;
    }
    uint32_t v = 0;
    for (int k = 0; k < 4; ++k)
        if (pos + k >= w.base && pos + k < w.end) v |= (uint32_t)w.data[pos + k - w.base] << (8 * k);
    return v;
}

// at least 32 bits in the buffer
PNGINF_HD void refill(Bits& b, const Window& w) {
    if (b.cnt <= 32) {
        b.buf |= (uint64_t)window_word(w, b.pos) << b.cnt;
        b.cnt += 32;
        b.pos += 4;
    }
}

PNGINF_HD uint32_t take(Bits& b, int n) {            // n <= 16, after refill
    uint32_t v = (uint32_t)b.buf & ((1u << n) - 1);
    b.buf >>= n;
    b.cnt -= n;
    return v;
}

PNGINF_HD uint64_t bit_position(const Bits& b) { return b.pos * 8 - (uint64_t)b.cnt; }

// restart the reader at byte p of the stream (after a stored block)
PNGINF_HD void seek(Bits& b, const Window& w, uint64_t p) {
    b.pos = p & ~(uint64_t)3;
    b.buf = 0;
    b.cnt = 0;
    refill(b, w);
    int drop = (int)(p & 3) * 8;
    b.buf >>= drop;
    b.cnt -= drop;
}

// ---- canonical Huffman codes -------------------------------------------------------------------------------------------------------
PNGINF_HD uint32_t reverse_bits(uint32_t v, int n) {
    uint32_t r = 0;
    for (int k = 0; k < n; ++k) {
        r = (r << 1) | (v & 1);
        v >>= 1;
    }
    return r;
}

// lens[0..n) -> cnt[16], sym[] in canonical order and the direct table fast[1 << fast_bits].  Returns 0, or BAD_CODE for an
// over-subscribed code and for an incomplete one unless it is a single code of length 1 (allow_single) or no code at all (allow_empty).
PNGINF_HD int build_code(const uint8_t* lens, int n, uint16_t* cnt, uint16_t* sym, uint16_t* offs, uint16_t* fast, int fast_bits,
                         bool allow_single, bool allow_empty) {
    for (int l = 0; l < 16; ++l) cnt[l] = 0;
    for (int i = 0; i < n; ++i) cnt[lens[i] & 15]++;
    int used = n - cnt[0];
    cnt[0] = 0;
    int left = 1, maxlen = 0;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - cnt[l];
        if (left < 0) return BAD_CODE;
        if (cnt[l]) maxlen = l;
    }
    if (left > 0 && !((used == 0 && allow_empty) || (maxlen == 1 && allow_single))) return BAD_CODE;
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (int i = 0; i < n; ++i)
        if (lens[i] & 15) sym[offs[lens[i] & 15]++] = (uint16_t)i;
    if (fast) {
        for (int i = 0; i < (1 << fast_bits); ++i) fast[i] = 0;
        uint32_t code = 0;
        int idx = 0;
        for (int l = 1; l <= fast_bits; ++l) {
            for (int k = 0; k < cnt[l]; ++k) {
                uint16_t e = (uint16_t)((l << 9) | sym[idx + k]);
                for (uint32_t j = reverse_bits(code + k, l); j < (1u << fast_bits); j += 1u << l) fast[j] = e;
            }
            code = (code + cnt[l]) << 1;
            idx += cnt[l];
        }
    }
    return 0;
}

// the count walk (a code of any length): the symbol, or -1 where the next bits are no code (only in an incomplete code)
PNGINF_HD int walk_code(Bits& b, const uint16_t* cnt, const uint16_t* sym) {
    int code = 0, first = 0, index = 0;
    uint32_t bits = (uint32_t)b.buf;
    for (int l = 1; l < 16; ++l) {
        code |= (int)(bits & 1);
        bits >>= 1;
        int c = cnt[l];
        if (code - c < first) {
            b.buf >>= l;
            b.cnt -= l;
            return sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    b.buf >>= 15;                          // consumed, so that the caller's position moves
    b.cnt -= 15;
    return -1;
}

PNGINF_HD int decode_fast(Bits& b, const uint16_t* fast, int fast_bits, const uint16_t* cnt, const uint16_t* sym) {
    uint32_t e = fast[(uint32_t)b.buf & ((1u << fast_bits) - 1)];
    if (e) {
        int l = (int)(e >> 9);
        b.buf >>= l;
        b.cnt -= l;
        return (int)(e & 511);
    }
    return walk_code(b, cnt, sym);
}

// RFC 1951 3.2.5 in closed form (no tables: nothing indexed in memory); i = length symbol - 257, 0..28
PNGINF_HD int length_extra(int i) { return (i < 8 || i == 28) ? 0 : (i - 4) >> 2; }
PNGINF_HD int length_base(int i) { return i < 8 ? 3 + i : i == 28 ? 258 : 3 + ((4 + (i & 3)) << length_extra(i)); }
PNGINF_HD int dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }                    // i = distance symbol 0..29
PNGINF_HD int dist_base(int i) { return i < 4 ? i + 1 : ((2 + (i & 1)) << dist_extra(i)) + 1; }

// ---- the steps ---------------------------------------------------------------------------------------------------------------------
PNGINF_HD int fail(State& s, int status) {
    s.status = status;
    s.phase = PH_DONE;
    return DONE;
}

// fixed or dynamic block header -> tables.  0 or a status.
PNGINF_HD int read_codes(State& s, Bits& b, const Window& w, int btype) {
    int hlit, hdist;
    if (btype == 1) {
        hlit = 288;
        hdist = 32;                                        // the fixed distance code is complete with its two unused symbols 30 and 31
        for (int i = 0; i < 288; ++i) s.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
        for (int i = 0; i < 32; ++i) s.lens[288 + i] = 5;
    } else {
        refill(b, w);
        hlit = (int)take(b, 5) + 257;
        hdist = (int)take(b, 5) + 1;
        int hclen = (int)take(b, 4) + 4;
        if (hlit > 286 || hdist > 30) return BAD_CODE;
        for (int i = 0; i < 19; ++i) s.cl[i] = 0;
        for (int i = 0; i < hclen; ++i) {
            refill(b, w);
            // the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
            int k = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1) ? 7 - ((i - 5) >> 1) : 8 + ((i - 4) >> 1);
            s.cl[k] = (uint8_t)take(b, 3);
        }
        if (build_code(s.cl, 19, s.ccnt, s.csym, s.offs, nullptr, 0, false, false)) return BAD_CODE;
        int n = 0;
        while (n < hlit + hdist) {
            refill(b, w);
            int sy = walk_code(b, s.ccnt, s.csym);
            if (sy < 0) return BAD_CODE;
            if (sy < 16) {
                s.lens[n++] = (uint8_t)sy;
                continue;
            }
            int rep, val = 0;
            if (sy == 16) {
                if (n == 0) return BAD_CODE;
                val = s.lens[n - 1];
                rep = 3 + (int)take(b, 2);
            } else if (sy == 17) {
                rep = 3 + (int)take(b, 3);
            } else {
                rep = 11 + (int)take(b, 7);
            }
            if (n + rep > hlit + hdist) return BAD_CODE;
            for (int k = 0; k < rep; ++k) s.lens[n++] = (uint8_t)val;
        }
        if (s.lens[256] == 0) return BAD_CODE;             // no end-of-block code
    }
    if (build_code(s.lens, hlit, s.h.lit_cnt, s.h.lit_sym, s.offs, s.h.lit_fast, LIT_FAST, true, false)) return BAD_CODE;
    if (build_code(s.lens + hlit, hdist, s.h.dist_cnt, s.h.dist_sym, s.offs, s.h.dist_fast, DIST_FAST, true, true)) return BAD_CODE;
    return 0;
}

// One step of the decoder.  tokens: ROUND_TOKENS entries.  The caller carries out what is returned before the next step:
//   NEED_INPUT  a window with [s.in_pos, min(s.in_pos + STEP_INPUT, s.in_len)) inside it (nothing else changed)
//   TOKENS      s.count tokens, destinations s.out_start + rel: all within [0, out_len), every source within the bytes before it
//   STORED      copy s.count bytes from stream offset s.src (within the stream) to s.out_start (within the output)
//   CONTINUE    nothing to do
//   DONE        s.status is final (OK: the caller compares s.adler_stored with the Adler-32 of the out_len bytes)
PNGINF_HD int step(State& s, const Window& w, Token* tokens) {
    if (s.phase == PH_DONE) return DONE;
    {
        uint64_t want = s.in_pos + STEP_INPUT < s.in_len ? s.in_pos + STEP_INPUT : s.in_len;
        uint64_t from = s.in_pos < s.in_len ? s.in_pos : s.in_len;
        if (from < want && (from < w.base || want > w.end)) return NEED_INPUT;
    }
    Bits b;
    b.buf = s.bitbuf;
    b.cnt = s.bitcnt;
    b.pos = s.in_pos;
    if (b.cnt == 0 && (b.pos & 3)) seek(b, w, b.pos);      // behind a stored block
    int result = CONTINUE, status = OK;
    const uint64_t in_bits = s.in_len * 8;

    if (s.phase == PH_ZLIB) {
        refill(b, w);
        uint32_t cmf = take(b, 8), flg = take(b, 8);
        if (bit_position(b) > in_bits) status = INPUT_END;
        else if ((cmf & 15) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31 != 0 || (flg & 32)) status = BAD_HEADER;
        s.phase = PH_BLOCK;
    } else if (s.phase == PH_BLOCK) {
        refill(b, w);
        s.final_block = (int32_t)take(b, 1);
        int btype = (int)take(b, 2);
        if (bit_position(b) > in_bits) {
            status = INPUT_END;
        } else if (btype == 3) {
            status = BAD_BLOCK;
        } else if (btype == 0) {
            take(b, b.cnt & 7);                            // to the byte boundary (cnt and the bit position agree modulo 8)
            refill(b, w);
            uint32_t len = take(b, 16);
            refill(b, w);
            uint32_t nlen = take(b, 16);
            uint64_t at = bit_position(b) >> 3;
            if (bit_position(b) > in_bits) status = INPUT_END;
            else if (len != (nlen ^ 0xFFFFu)) status = BAD_BLOCK;
            else if (at + len > s.in_len) status = INPUT_END;
            else if (s.out_pos + len > s.out_len) status = SIZE;
            else {
                s.src = at;
                s.out_start = s.out_pos;
                s.count = len;
                s.out_pos += len;
                b.buf = 0;                                 // the next step starts reading at at + len (it seeks there if that is not
                b.cnt = 0;                                 // a multiple of 4, after it has asked for the window that holds it)
                b.pos = at + len;
                result = STORED;
                s.phase = s.final_block ? PH_TRAILER : PH_BLOCK;
            }
        } else {
            status = read_codes(s, b, w, btype);
            s.phase = PH_CODES;
        }
    } else if (s.phase == PH_CODES) {
        uint32_t n = 0;
        uint64_t out = s.out_pos;
        s.out_start = out;
        while (n < (uint32_t)ROUND_TOKENS) {
            refill(b, w);
            int sy = decode_fast(b, s.h.lit_fast, LIT_FAST, s.h.lit_cnt, s.h.lit_sym);
            if (sy < 0) {
                status = bit_position(b) > in_bits ? INPUT_END : BAD_SYMBOL;
                break;
            }
            if (sy < 256) {
                if (bit_position(b) > in_bits) { status = INPUT_END; break; }
                if (out >= s.out_len) { status = SIZE; break; }
                tokens[n].rel = (uint32_t)(out - s.out_start);
                tokens[n].len = 0;
                tokens[n].val = (uint16_t)sy;
                ++n;
                ++out;
                continue;
            }
            if (sy == 256) {
                if (bit_position(b) > in_bits) status = INPUT_END;
                else s.phase = s.final_block ? PH_TRAILER : PH_BLOCK;
                break;
            }
            if (sy > 285) { status = bit_position(b) > in_bits ? INPUT_END : BAD_SYMBOL; break; }
            refill(b, w);
            int li = sy - 257;
            uint32_t len = (uint32_t)length_base(li) + take(b, length_extra(li));
            int ds = decode_fast(b, s.h.dist_fast, DIST_FAST, s.h.dist_cnt, s.h.dist_sym);
            if (ds < 0 || ds > 29) { status = bit_position(b) > in_bits ? INPUT_END : BAD_SYMBOL; break; }
            refill(b, w);
            uint32_t dist = (uint32_t)dist_base(ds) + take(b, dist_extra(ds));
            if (bit_position(b) > in_bits) { status = INPUT_END; break; }
            if (dist > out || dist > 32768) { status = BAD_DISTANCE; break; }
            if (out + len > s.out_len) { status = SIZE; break; }
            tokens[n].rel = (uint32_t)(out - s.out_start);
            tokens[n].len = (uint16_t)len;
            tokens[n].val = (uint16_t)(dist - 1);
            ++n;
            out += len;
        }
        // the tokens before a bad one are valid and are still handed out; the status ends the stream at the next step
        s.out_pos = out;
        s.count = n;
        result = TOKENS;
    } else {                                               // PH_TRAILER
        if (s.out_pos != s.out_len) {
            status = SIZE;
        } else {
            take(b, b.cnt & 7);
            uint32_t a = 0;
            for (int k = 0; k < 4; ++k) {
                refill(b, w);
                a = (a << 8) | take(b, 8);
            }
            if (bit_position(b) > in_bits) status = INPUT_END;
            s.adler_stored = a;
        }
        s.phase = PH_DONE;
        result = DONE;
    }
    s.bitbuf = b.buf;
    s.bitcnt = b.cnt;
    s.in_pos = b.pos;
    if (status != OK) {
        if (bit_position(b) > in_bits) status = INPUT_END; // whatever was found in the zero bits behind the stream's end
        s.status = status;
        s.phase = PH_DONE;
        if (result != TOKENS) result = DONE;
    }
    return result;
}

// Adler-32 of a whole buffer from two plain sums (what the kernel's reduction forms lane by lane): A = 1 + sum b[i], B = n + sum (n - i) b[i]
PNGINF_HD uint32_t adler_from_sums(uint64_t sum_b, uint64_t sum_wb, uint64_t n) {
    uint32_t a = (uint32_t)((1 + sum_b % ADLER_MOD) % ADLER_MOD);
    uint32_t bb = (uint32_t)((n % ADLER_MOD + sum_wb % ADLER_MOD) % ADLER_MOD);
    return (bb << 16) | a;
}

}  // namespace pnginf
}  // namespace chk
