// dng_enc_hostcheck.cpp -- the per-lane routines of csrc/dng_enc_dev.h (the lossless-JPEG encoder of csrc/dng_enc.hip) under a host compiler and
// its sanitizers (tests/test_dng_enc_cpu.py builds this with -fsanitize=address,undefined and runs it; it never runs on a GPU and is never
// loaded into Python).
//
//   dng_enc_hostcheck cases.bin out.bin
//
// cases.bin (written by the test, little-endian): uint32 ncases; per case: uint32 th, tw, P, segment (samples), chunk (bytes); 17 uint32: the
// table, (code length << 16) | code per category; th * tw uint16: the tile.
// Per case the program does what the kernels do, in the kernels' cut: every segment is split into the runs of 256 lanes, each run's bits are
// counted (dng_enc_run_bits), a serial prefix sum stands for the scans and for the host's plan, and dng_enc_run ORs the run into a dword image
// of the stream's exact size -- a plain OR stands for the atomic one.  The image's bytes are then stuffed chunk by chunk, 16 bytes a lane
// (dng_enc_count_ff, a serial prefix sum, dng_enc_stuff), into a buffer of the stuffed stream's exact size.  Every buffer is a heap allocation
// of its exact size, so any access outside it stops the program under AddressSanitizer, and any undefined shift under UBSan.
// out.bin: per case uint32 nbytes and the stuffed entropy-coded bytes; the test compares them with its reference encoder.
// Over all cases the runs must have covered: a sample of 1 bit, a sample of 31 bits, and a run starting at each bit phase 0..31; the program
// prints what it saw and "hostcheck OK", with exit status 0 only then.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../eld_amd/csrc/dng_enc_dev.h"

namespace {

constexpr uint32_t LANES = 256;

bool read_exact(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

struct HeapOr {                                                      // the dword image: exact size, index checked
    uint32_t* img;
    uint32_t ndw;
    bool overflow;
    void operator()(uint32_t i, uint32_t v) {
        if (i >= ndw) { overflow = true; return; }
        img[i] |= v;
    }
};

bool seen_phase[32];
bool seen_1 = false, seen_31 = false;

struct Run { uint32_t first, count, bits; };

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: dng_enc_hostcheck cases.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    FILE* g = fopen(argv[2], "wb");
    if (!g) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    uint32_t ncases = 0;
    if (!read_exact(f, &ncases, 4) || ncases < 1 || ncases > 1000) { fprintf(stderr, "bad case count\n"); return 2; }
    for (uint32_t ci = 0; ci < ncases; ++ci) {
        uint32_t hd[5];
        uint32_t* table = (uint32_t*)malloc(17 * sizeof(uint32_t));
        if (!read_exact(f, hd, sizeof(hd)) || !read_exact(f, table, 17 * sizeof(uint32_t))) { fprintf(stderr, "bad case header\n"); return 2; }
        const uint32_t th = hd[0], tw = hd[1], P = hd[2], segment = hd[3], chunk = hd[4];
        if (th < 1 || tw < 2 || th > 4096 || tw > 4096 || P < 2 || P > 16 || segment < 1 || segment > ELD_DNG_ENC_MAX_SEGMENT || chunk < 16 ||
            chunk > ELD_DNG_ENC_MAX_CHUNK || chunk % 16) { fprintf(stderr, "case %u: bad geometry\n", ci); return 2; }
        const uint32_t n = th * tw;
        uint16_t* tile = (uint16_t*)malloc(n * sizeof(uint16_t));
        if (!read_exact(f, tile, n * sizeof(uint16_t))) { fprintf(stderr, "bad tile\n"); return 2; }
        DngEncSrc src;
        src.mos = tile; src.H = (int)th; src.W = (int)tw; src.y0 = 0; src.x0 = 0; src.tw = (int)tw; src.half = 1u << (P - 1);
        // the cut of the kernels: segments of `segment` samples, 256 runs each
        const uint32_t run = (segment + LANES - 1) / LANES;
        std::vector<Run> runs;
        uint64_t total = 0;
        for (uint32_t s0 = 0; s0 < n; s0 += segment) {
            const uint32_t sc = n - s0 < segment ? n - s0 : segment;
            for (uint32_t l = 0; l < LANES && l * run < sc; ++l) {
                Run r;
                r.first = s0 + l * run;
                r.count = sc - l * run < run ? sc - l * run : run;
                r.bits = dng_enc_run_bits(src, table, r.first, r.count);
                total += r.bits;
                runs.push_back(r);
            }
        }
        if (total == 0 || total >= (1ull << 31)) { fprintf(stderr, "case %u: %llu bits\n", ci, (unsigned long long)total); return 1; }
        const uint32_t pad = (uint32_t)((0 - total) & 7u);
        const uint32_t nraw = (uint32_t)((total + 7) / 8), ndw = (uint32_t)((total + pad + 31) / 32);
        HeapOr put;
        put.img = (uint32_t*)calloc(ndw, sizeof(uint32_t)); put.ndw = ndw; put.overflow = false;
        uint32_t bit = 0;
        for (size_t i = 0; i < runs.size(); ++i) {
            const Run& r = runs[i];
            seen_phase[bit & 31u] = true;
            // the samples' sizes, for the coverage report
            DngEncCursor k = dng_enc_cursor(src, r.first);
            for (uint32_t j = 0; j < r.count; ++j) {
                uint32_t code, nb;
                (void)dng_enc_word(dng_enc_next(src, k, &code), table, &nb);
                if (nb == 0) { fprintf(stderr, "case %u: sample %u falls into a category the table lacks\n", ci, r.first + j); return 1; }
                seen_1 |= nb == 1;
                seen_31 |= nb == 31;
            }
            dng_enc_run(src, table, r.first, r.count, bit, i + 1 == runs.size() ? pad : 0u, put);
            bit += r.bits;
        }
        if (put.overflow) { fprintf(stderr, "case %u: a dword beyond the image\n", ci); return 1; }
        // the image's bytes: bit 0 is the top bit of byte 0
        uint8_t* raw = (uint8_t*)malloc(nraw);
        for (uint32_t i = 0; i < nraw; ++i) raw[i] = (uint8_t)(put.img[i >> 2] >> (24 - 8 * (i & 3)));
        // stuffing, in the kernels' cut: chunks of `chunk` bytes, 16 bytes a lane
        std::vector<uint32_t> ff;
        uint32_t nff = 0;
        for (uint32_t c0 = 0; c0 < nraw; c0 += chunk) {
            const uint32_t cn = nraw - c0 < chunk ? nraw - c0 : chunk;
            for (uint32_t o = 0; o < cn; o += DNG_ENC_LANE_BYTES) {
                const uint32_t m = cn - o < DNG_ENC_LANE_BYTES ? cn - o : DNG_ENC_LANE_BYTES;
                uint8_t* b = (uint8_t*)malloc(DNG_ENC_LANE_BYTES);
                memset(b, 0, DNG_ENC_LANE_BYTES);
                memcpy(b, raw + c0 + o, m);
                const uint32_t c = dng_enc_count_ff(b, m);
                ff.push_back(c);
                nff += c;
                free(b);
            }
        }
        const uint32_t nout = nraw + nff;
        uint8_t* out = (uint8_t*)malloc(nout);
        memset(out, 0xA5, nout);
        uint32_t before = 0, end = 0;
        size_t li = 0;
        for (uint32_t c0 = 0; c0 < nraw; c0 += chunk) {
            const uint32_t cn = nraw - c0 < chunk ? nraw - c0 : chunk;
            for (uint32_t o = 0; o < cn; o += DNG_ENC_LANE_BYTES, ++li) {
                const uint32_t m = cn - o < DNG_ENC_LANE_BYTES ? cn - o : DNG_ENC_LANE_BYTES;
                uint8_t* b = (uint8_t*)malloc(DNG_ENC_LANE_BYTES);
                memset(b, 0, DNG_ENC_LANE_BYTES);
                memcpy(b, raw + c0 + o, m);
                end = dng_enc_stuff(b, m, out, c0 + o + before, nout);
                before += ff[li];
                free(b);
            }
        }
        if (end != nout) { fprintf(stderr, "case %u: the stuffed bytes end at %u of %u\n", ci, end, nout); return 1; }
        if (fwrite(&nout, 4, 1, g) != 1 || fwrite(out, 1, nout, g) != nout) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
        printf("case %u: %u x %u, segment %u, chunk %u: %zu runs, %llu bits, %u bytes, %u stuffed\n", ci, th, tw, segment, chunk, runs.size(),
               (unsigned long long)total, nraw, nff);
        free(out); free(raw); free(put.img); free(tile); free(table);
    }
    fclose(f);
    if (fclose(g) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    int phases = 0;
    for (int i = 0; i < 32; ++i) phases += seen_phase[i] ? 1 : 0;
    printf("coverage: 1-bit sample %s, 31-bit sample %s, %d of 32 start phases\n", seen_1 ? "yes" : "no", seen_31 ? "yes" : "no", phases);
    if (!seen_1 || !seen_31 || phases != 32) { fprintf(stderr, "the cases do not cover what they must\n"); return 1; }
    printf("hostcheck OK\n");
    return 0;
}
