// The host-side check of an ingest batch (ctrlhair_amd/csrc/ingest_batch.h) on the CPU, for a sanitizer build.  tests/test_ingest.py
// compiles this with -fsanitize=address,undefined and runs it over good batches, every documented refusal and batches with words
// overwritten at random.
//
//   ingest_check_host LIST
// LIST: a text file, one case per line: <batch file> <N> <P> <mode>.  Per case one line on stdout: <workspace bytes, 0 = refused> <the
// refusal's message, or ok>.  The batch is malloc'ed at exactly its size, so a read outside it is a sanitizer report.  For a batch that
// passes, every word the kernels of ingest.hip would read from it is read here in the same way -- bounds of every output, and the
// coefficients [0, count) in the pass's layout -- and every tap is asserted to lie inside the image's row or column: what the check lets
// through, the kernels can follow.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../ctrlhair_amd/csrc/ingest_batch.h"

static uint8_t* read_file(const char* path, size_t& n) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short read %s\n", path); exit(2); }
    fclose(f);
    return p;
}

// the reads of one pass of one image; returns false when a tap leaves [0, in)
static bool walk(const int32_t* b32, int at, int in, int P, int layout, long long& sum) {
    const int32_t* tab = b32 + at;
    const int ksize = tab[2];
    const int32_t* bounds = tab + 4;
    const int32_t* k = bounds + 2 * P;
    for (int i = 0; i < P; ++i) {
        const int first = bounds[2 * i], count = bounds[2 * i + 1];
        if (first < 0 || count < 1 || count > ksize || first + count > in) return false;
        for (int j = 0; j < count; ++j) sum += layout ? k[(size_t)j * P + i] : k[(size_t)i * ksize + j];
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: ingest_check_host LIST\n"); return 2; }
    FILE* list = fopen(argv[1], "r");
    if (!list) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char path[4096];
    int N, P, mode;
    long long sum = 0;
    while (fscanf(list, "%4095s %d %d %d", path, &N, &P, &mode) == 4) {
        size_t bytes = 0, need = 0;
        uint8_t* blob = read_file(path, bytes);
        const std::string why = chk::ingest_check(blob, bytes, N, P, mode, need);
        if (why.empty()) {
            const chk::IngestImage* d = reinterpret_cast<const chk::IngestImage*>(blob);
            const int32_t* b32 = reinterpret_cast<const int32_t*>(blob);
            for (int n = 0; n < N; ++n) {
                if (d[n].H < 1 || d[n].W < 1 || d[n].H > chk::INGEST_MAX_SIDE || d[n].W > chk::INGEST_MAX_SIDE) { fprintf(stderr, "%s: image %d passed with sides out of range\n", path, n); return 1; }
                if ((d[n].htab >= 0 && !walk(b32, d[n].htab, d[n].W, P, 1, sum)) || (d[n].vtab >= 0 && !walk(b32, d[n].vtab, d[n].H, P, 0, sum))) {
                    fprintf(stderr, "%s: image %d passed with a tap outside the image\n", path, n);
                    return 1;
                }
                if (mode != chk::INGEST_PIL && (d[n].htab >= 0 || d[n].vtab >= 0)) { fprintf(stderr, "%s: image %d passed with a table in mode %d\n", path, n, mode); return 1; }
            }
            if (need < bytes || need % 256) { fprintf(stderr, "%s: workspace %zu for a batch of %zu bytes\n", path, need, bytes); return 1; }
        } else if (need != 0) {
            fprintf(stderr, "%s: refused with a workspace size\n", path);
            return 1;
        }
        printf("%zu %s\n", need, why.empty() ? "ok" : why.c_str());
        free(blob);
    }
    fclose(list);
    fprintf(stderr, "checksum %lld\n", sum);
    return 0;
}
