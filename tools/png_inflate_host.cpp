// The inflate core of the PNG decoder (ctrlhair_amd/csrc/png_inflate_core.h) on the CPU, for a sanitizer build: the same step() the kernel
// runs on one lane, with a plain serial loop in place of the wave's copies.  tests/test_pngdec.py compiles this with
// -fsanitize=address,undefined and runs it over the corpus and the malformed set.
//
//   png_inflate_host LIST [WINDOW]
// LIST: a text file, one case per line: <zlib stream file> <H> <row bytes = 1 + W * C> <output file>.  Per case one line on stdout:
// <status> <bytes produced>, and the H * row bytes of output in the output file.  WINDOW (bytes, a multiple of 16, >= 2048; default 0:
// the whole stream): hand the core a window of that many bytes as the kernel does, refilled whenever step() asks.
// The stream, the window and the output are malloc'ed at exactly their sizes: one byte read or written outside is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ctrlhair_amd/csrc/png_inflate_core.h"

namespace pi = chk::pnginf;

static int run_case(const std::string& zpath, long H, long rowbytes, const std::string& opath, long window) {
    FILE* f = fopen(zpath.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", zpath.c_str()); return 2; }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* in = (uint8_t*)malloc((size_t)n);
    if (n && fread(in, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read %s\n", zpath.c_str()); return 2; }
    fclose(f);
    const uint64_t out_len = (uint64_t)H * (uint64_t)rowbytes;
    uint8_t* out = (uint8_t*)malloc(out_len);
    memset(out, 0, out_len);
    pi::State* s = (pi::State*)malloc(sizeof(pi::State));
    pi::Token* tok = (pi::Token*)malloc(sizeof(pi::Token) * pi::ROUND_TOKENS);
    pi::init(*s, (uint64_t)n, out_len);
    pi::Window w{in, 0, (uint64_t)n};
    uint8_t* wbuf = nullptr;
    if (window) w.end = 0;                                   // empty: the first step asks
    long steps = 0;
    for (;;) {
        int r = pi::step(*s, w, tok);
        if (++steps > 100000000L) { fprintf(stderr, "%s: does not terminate\n", zpath.c_str()); return 3; }
        if (r == pi::DONE) break;
        if (r == pi::NEED_INPUT) {
            if (!window) { fprintf(stderr, "%s: NEED_INPUT with the whole stream in the window\n", zpath.c_str()); return 3; }
            free(wbuf);
            uint64_t base = s->in_pos & ~(uint64_t)3;
            uint64_t len = (uint64_t)n - base < (uint64_t)window ? (uint64_t)n - base : (uint64_t)window;
            wbuf = (uint8_t*)malloc(len);
            memcpy(wbuf, in + base, len);
            w = pi::Window{wbuf, base, base + len};
        } else if (r == pi::TOKENS) {
            for (uint32_t k = 0; k < s->count; ++k) {
                uint64_t dst = s->out_start + tok[k].rel;
                if (tok[k].len == 0) {
                    out[dst] = (uint8_t)tok[k].val;
                } else {
                    uint64_t dist = (uint64_t)tok[k].val + 1;
                    for (uint32_t i = 0; i < tok[k].len; ++i) out[dst + i] = out[dst - dist + (i % dist)];
                }
            }
        } else if (r == pi::STORED) {
            memcpy(out + s->out_start, in + s->src, s->count);
        }
    }
    int status = s->status;
    if (status == pi::OK) {
        uint64_t sb = 0, swb = 0;                              // the two sums of the kernel's reduction
        for (uint64_t i = 0; i < out_len; ++i) {
            sb += out[i];
            swb += ((out_len - i) % pi::ADLER_MOD) * out[i];
            if ((i & 0xFFFFF) == 0xFFFFF) swb %= pi::ADLER_MOD;
        }
        if (pi::adler_from_sums(sb, swb, out_len) != s->adler_stored) status = pi::ADLER;
    }
    if (status == pi::OK)
        for (long y = 0; y < H; ++y)
            if (out[(uint64_t)y * rowbytes] > 4) status = pi::BAD_FILTER;
    printf("%d %llu\n", status, (unsigned long long)s->out_pos);
    FILE* g = fopen(opath.c_str(), "wb");
    if (!g || fwrite(out, 1, out_len, g) != out_len) { fprintf(stderr, "cannot write %s\n", opath.c_str()); return 2; }
    fclose(g);
    free(wbuf);
    free(tok);
    free(s);
    free(out);
    free(in);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s LIST [WINDOW]\n", argv[0]); return 2; }
    long window = argc > 2 ? atol(argv[2]) : 0;
    if (window && (window < 2048 || window % 16)) { fprintf(stderr, "WINDOW must be 0 or a multiple of 16 >= 2048\n"); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char zp[4096], op[4096];
    long H, rb;
    while (fscanf(f, "%4095s %ld %ld %4095s", zp, &H, &rb, op) == 4) {
        int rc = run_case(zp, H, rb, op, window);
        if (rc) return rc;
    }
    fclose(f);
    return 0;
}
