// The entropy stage of the JPEG decoder (ctrlhair_amd/csrc/jpeg_entropy_core.h) on the CPU, for a sanitizer build: the same subsequence /
// round scheme the kernels of jpeg_decode.hip run, with serial loops in place of lanes, workgroups and launches.  tests/test_jpegdec.py
// compiles this with -fsanitize=address,undefined and runs it over the corpus and the malformed set.
//
//   jpeg_entropy_host LIST
// LIST: a text file, one case per line: <scan file> <table block file> <H> <W> <C> <sampling> <rounds> <output file> [<Ri>].  Ri: the
// restart interval in MCUs (absent or 0: none), the scan then with its RSTm markers, as ch_jpeg_decode_rst takes it.  Per case one line
// on stdout: <status> <launches after which the chain was whole, 0 if never within 64>, and the int16 [blocks][64] coefficients (natural
// order, DC values summed) in the output file.  The scan, every chunk's window, the state buffers and the coefficients are malloc'ed at
// exactly their sizes: one byte read or written outside is a sanitizer report.  The write pass runs whatever the status, as on the device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ctrlhair_amd/csrc/jpeg_entropy_core.h"

namespace je = chk::jpegent;

static uint8_t* read_file(const std::string& path, long& n) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path.c_str()); exit(2); }
    fseek(f, 0, SEEK_END);
    n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* p = (uint8_t*)malloc((size_t)n ? (size_t)n : 1);
    if (n && fread(p, 1, (size_t)n, f) != (size_t)n) { fprintf(stderr, "short read %s\n", path.c_str()); exit(2); }
    fclose(f);
    return p;
}

struct Chunk {                             // the window of chunk c, malloc'ed at its size
    uint8_t* bytes;
    je::Window w;
    Chunk(const uint8_t* in, uint32_t len, uint32_t c) {
        const uint32_t base = c * (uint32_t)je::CHUNK;
        const uint32_t n = len - base < (uint32_t)(je::CHUNK + je::MARGIN) ? len - base : (uint32_t)(je::CHUNK + je::MARGIN);
        bytes = (uint8_t*)malloc(n ? n : 1);
        memcpy(bytes, in + base, n);
        w = je::Window{bytes, base, n};
    }
    ~Chunk() { free(bytes); }
};

static je::State guess_of(const uint8_t* in, uint32_t i, bool rst) {
    return rst ? je::guess_rst(i, i ? in[i * je::SUBSEQ - 1] : 0, in[i * je::SUBSEQ]) : je::guess(i, i ? in[i * je::SUBSEQ - 1] : 0, in[i * je::SUBSEQ]);
}

// one launch: every chunk from `prev` (null: the first launch) into `cur`
static void launch(const je::Huff* tables, const je::Geometry& g, const uint8_t* in, uint32_t len, uint32_t nsub, const je::SubState* prev,
                   je::SubState* cur, bool rst) {
    for (uint32_t c = 0; c * je::LANES < nsub; ++c) {
        const uint32_t i0 = c * je::LANES, n = nsub - i0 < (uint32_t)je::LANES ? nsub - i0 : (uint32_t)je::LANES;
        Chunk ch(in, len, c);
        je::SubState st[je::LANES];
        bool changed[je::LANES];
        for (uint32_t l = 0; l < n; ++l) {
            const uint32_t i = i0 + l;
            if (!prev) {
                st[l].entry = i ? guess_of(in, i, rst) : je::State{0, 0};
                changed[l] = true;
            } else {
                st[l] = prev[i];
                if (l == 0 && i) {
                    const je::State e = je::entry_from(prev[i - 1].exit, guess_of(in, i, rst));
                    changed[l] = !je::same(e, st[l].entry);
                    st[l].entry = e;
                } else {
                    changed[l] = false;
                }
            }
        }
        for (int round = 0; round <= je::LANES; ++round) {
            for (uint32_t l = 0; l < n; ++l) {
                if (!changed[l]) continue;
                const uint32_t i = i0 + l, end = (i + 1) * je::SUBSEQ < len ? (i + 1) * je::SUBSEQ : len;
                je::NoAudit none;
                if (rst) je::run_subseq<true>(tables, g, ch.w, len, end, st[l].entry, 0u, je::NoSink{}, none, st[l].exit, st[l].count);
                else je::run_subseq<false>(tables, g, ch.w, len, end, st[l].entry, 0u, je::NoSink{}, none, st[l].exit, st[l].count);
            }
            bool any = false;
            changed[0] = false;
            for (uint32_t l = n - 1; l >= 1; --l) {
                const je::State e = je::entry_from(st[l - 1].exit, guess_of(in, i0 + l, rst));
                changed[l] = !je::same(e, st[l].entry);
                st[l].entry = e;
                any |= changed[l];
            }
            if (!any) break;
        }
        for (uint32_t l = 0; l < n; ++l) cur[i0 + l] = st[l];
    }
}

static int status_of(const je::SubState* f, uint32_t nsub, const je::Geometry& g) {
    uint64_t blocks = f[0].count;
    for (uint32_t i = 1; i < nsub; ++i) {
        if (int why = je::chain_break(f[i - 1].exit, f[i].entry)) return why;
        blocks += f[i].count;
    }
    return je::final_status(f[nsub - 1].exit, blocks, g);
}

static int run_case(const std::string& spath, const std::string& tpath, int H, int W, int C, int sampling, int rounds, const std::string& opath,
                    uint32_t restart) {
    long n = 0, tn = 0;
    uint8_t* in = read_file(spath, n);
    uint8_t* tb = read_file(tpath, tn);
    if (tn != je::TABLE_BYTES) { fprintf(stderr, "%s: not a table block\n", tpath.c_str()); return 2; }
    const je::Geometry g = je::geometry(H, W, C, sampling);
    const uint32_t ri = je::effective_restart(g, restart);
    je::Huff* tables = (je::Huff*)malloc(6 * sizeof(je::Huff));
    for (int t = 0; t < 6; ++t) {
        const uint8_t* src = tb + je::TABLE_HUFF + t * je::TABLE_HUFF_STRIDE;
        je::build_codes(tables[t], src);
        memcpy(tables[t].vals, src + 16, 256);
        for (uint32_t e = 0; e < (1u << je::FAST_BITS); ++e) tables[t].fast[e] = je::fast_entry(tables[t], e);
    }
    int16_t* coef = (int16_t*)calloc((size_t)g.nblocks * 64, sizeof(int16_t));
    int status, needed = 0;
    const uint32_t len = (uint32_t)n;
    if ((uint64_t)n >= je::MAX_STREAM) {
        status = je::TOO_LONG;
    } else if (n == 0) {
        status = je::INPUT_END;
    } else {
        const uint32_t nsub = (len + je::SUBSEQ - 1) / je::SUBSEQ;
        je::SubState* buf[2] = {(je::SubState*)malloc(nsub * sizeof(je::SubState)), (je::SubState*)malloc(nsub * sizeof(je::SubState))};
        if (rounds <= 0) rounds = je::DEFAULT_ROUNDS;
        if (rounds > je::MAX_ROUNDS) rounds = je::MAX_ROUNDS;
        status = je::NOT_SYNCED;
        std::vector<je::SubState> fin(nsub);
        for (int k = 0; k < je::MAX_ROUNDS; ++k) {
            launch(tables, g, in, len, nsub, k ? buf[(k - 1) & 1] : nullptr, buf[k & 1], ri != 0);
            const int st = status_of(buf[k & 1], nsub, g);
            if (!needed && st != je::NOT_SYNCED) needed = k + 1;
            if (k + 1 == rounds) {
                status = st;
                memcpy(fin.data(), buf[k & 1], nsub * sizeof(je::SubState));
            }
            if (needed && k + 1 >= rounds) break;
        }
        for (uint32_t i = 0; i + 1 < len; ++i)
            if (in[i] == 0xFF && in[i + 1] != 0 && !(ri && je::is_rst(in[i + 1])) && status == je::OK) status = je::MARKER;
        // the write pass from the final states, whatever the status (its verdict on the restart markers counts where the device runs it)
        uint32_t first = 0;
        const bool audited = status == je::OK;
        je::RstAudit audit{ri * (uint32_t)g.bpm, g.nblocks, false};
        for (uint32_t i = 0; i < nsub; ++i) {
            Chunk ch(in, len, i / je::LANES);
            const uint32_t end = (i + 1) * je::SUBSEQ < len ? (i + 1) * je::SUBSEQ : len;
            je::State ex;
            uint32_t cnt;
            je::NoAudit none;
            if (ri) je::run_subseq<true>(tables, g, ch.w, len, end, fin[i].entry, first, je::CoefSink{coef, g.nblocks}, audit, ex, cnt);
            else je::run_subseq<false>(tables, g, ch.w, len, end, fin[i].entry, first, je::CoefSink{coef, g.nblocks}, none, ex, cnt);
            first += fin[i].count;
        }
        if (audited && audit.bad) status = je::RESTART;
        free(buf[0]);
        free(buf[1]);
    }
    if (status == je::OK) {
        uint32_t pred[3] = {0, 0, 0};
        for (uint32_t b = 0; b < g.nblocks; ++b) {
            if (ri && b % (ri * (uint32_t)g.bpm) == 0) pred[0] = pred[1] = pred[2] = 0;
            const int c = je::comp_of(g, b % (uint32_t)g.bpm);
            pred[c] += (uint32_t)(int32_t)coef[(size_t)b * 64];
            coef[(size_t)b * 64] = (int16_t)(uint16_t)pred[c];
        }
    }
    printf("%d %d\n", status, needed);
    FILE* o = fopen(opath.c_str(), "wb");
    if (!o || fwrite(coef, sizeof(int16_t), (size_t)g.nblocks * 64, o) != (size_t)g.nblocks * 64) { fprintf(stderr, "cannot write %s\n", opath.c_str()); return 2; }
    fclose(o);
    free(coef);
    free(tables);
    free(tb);
    free(in);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s LIST\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    static char line[3 * 4096 + 256], sp[4096], tp[4096], op[4096];
    int H, W, C, sampling, rounds;
    while (fgets(line, sizeof line, f)) {
        unsigned restart = 0;
        const int got = sscanf(line, "%4095s %4095s %d %d %d %d %d %4095s %u", sp, tp, &H, &W, &C, &sampling, &rounds, op, &restart);
        if (got < 8) break;
        if (H < 1 || W < 1 || H > 32768 || W > 32768 || (C != 1 && C != 3) || sampling < 0 || sampling > 2) { fprintf(stderr, "bad case\n"); return 2; }
        if (int rc = run_case(sp, tp, H, W, C, sampling, rounds, op, restart)) return rc;
    }
    fclose(f);
    return 0;
}
