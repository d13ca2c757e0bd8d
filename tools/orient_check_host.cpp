// The host-side check of a ch_orient_u8 batch (ctrlhair_amd/csrc/orient_batch.h) on the CPU, for a sanitizer build.  tests/test_orient.py
// compiles this with -fsanitize=address,undefined and runs it over good batches, every documented refusal and batches with words
// overwritten at random.
//
//   orient_check_host LIST
// LIST: a text file, one case per line: <batch file> <N> <dst address> <dst bytes>.  Per case one line on stdout: <workspace bytes, 0 =
// refused> <the refusal's message, or ok>.  The batch is malloc'ed at exactly its size, so a read outside it is a sanitizer report.  For
// a batch that passes, the tile walk of orient.hip is repeated here for every image -- the stored tile's origin and size, the upright
// tile's origin and size, the byte run of each of its rows -- and every run is asserted to lie inside the image's own destination
// extent, which is asserted to lie inside the buffer: what the check lets through, the kernel can follow.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../ctrlhair_amd/csrc/orient_batch.h"

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

// the destination runs of one image; returns false when one leaves [d.dst, d.dst + H * W * C) or that leaves [0, dst_bytes)
static bool walk(const chk::OrientImage& d, uint64_t dst_bytes, unsigned long long& sum) {
    const int T = chk::ORIENT_TILE, o = d.orient, C = d.C;
    const uint64_t bytes = (uint64_t)d.H * d.W * C, first = (uint64_t)d.dst;
    if (first > dst_bytes || bytes > dst_bytes - first) return false;
    const bool tr = o >= 5, FY = o == 3 || o == 4 || o == 6 || o == 7, FX = o == 2 || o == 3 || o == 7 || o == 8;
    const int tiles_x = (d.W + T - 1) / T;
    const uint64_t dpitch = (uint64_t)(tr ? d.H : d.W) * C;
    uint64_t covered = 0;
    for (unsigned b = 0; b < chk::orient_tiles(d.H, d.W); ++b) {
        const int ty = (int)(b / tiles_x), tx = (int)(b % tiles_x), sy0 = ty * T, sx0 = tx * T;
        if (sy0 >= d.H || sx0 >= d.W) return false;
        const int th = d.H - sy0 < T ? d.H - sy0 : T, tw = d.W - sx0 < T ? d.W - sx0 : T;
        const int dh = tr ? tw : th, dw = tr ? th : tw;
        const int dy0 = tr ? (FX ? d.W - sx0 - tw : sx0) : (FY ? d.H - sy0 - th : sy0);
        const int dx0 = tr ? (FY ? d.H - sy0 - th : sy0) : (FX ? d.W - sx0 - tw : sx0);
        if (dy0 < 0 || dx0 < 0) return false;
        for (int r = 0; r < dh; ++r) {
            const uint64_t lo = (uint64_t)(dy0 + r) * dpitch + (uint64_t)dx0 * C, hi = lo + (uint64_t)dw * C;
            if (hi > bytes) return false;
            covered += hi - lo;
            sum += lo;
        }
    }
    return covered == bytes;                                  // the tiles partition the image: every byte is written once
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: orient_check_host LIST\n"); return 2; }
    FILE* list = fopen(argv[1], "r");
    if (!list) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char path[4096];
    int N;
    unsigned long long dst_addr, dst_bytes, sum = 0;
    while (fscanf(list, "%4095s %d %llu %llu", path, &N, &dst_addr, &dst_bytes) == 4) {
        size_t bytes = 0, need = 0;
        uint8_t* blob = read_file(path, bytes);
        const std::string why = chk::orient_check(blob, bytes, N, dst_addr, dst_bytes, need);
        if (why.empty()) {
            const chk::OrientImage* d = reinterpret_cast<const chk::OrientImage*>(blob);
            for (int n = 0; n < N; ++n) {
                if (d[n].C != 1 && d[n].C != 3 && d[n].C != 4) { fprintf(stderr, "%s: image %d passed with C = %d\n", path, n, d[n].C); return 1; }
                if (d[n].orient < 1 || d[n].orient > 8) { fprintf(stderr, "%s: image %d passed with orientation %d\n", path, n, d[n].orient); return 1; }
                if (d[n].H < 1 || d[n].W < 1 || d[n].H > chk::ORIENT_MAX_SIDE || d[n].W > chk::ORIENT_MAX_SIDE) { fprintf(stderr, "%s: image %d passed with sides out of range\n", path, n); return 1; }
                if (!walk(d[n], dst_bytes, sum)) { fprintf(stderr, "%s: image %d passed with a run outside its destination\n", path, n); return 1; }
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
    fprintf(stderr, "checksum %llu\n", sum);
    return 0;
}
