// jpeg_hostcheck.cpp -- the per-block routines of csrc/jpeg_dev.h (the baseline-JPEG encoder of csrc/jpeg.hip) under a host compiler and its
// sanitizers (tests/test_jpeg_cpu.py builds this with -fsanitize=address,undefined and runs it; it never runs on a GPU and is never loaded into
// Python).
//
//   jpeg_hostcheck cases.bin out.bin
//
// cases.bin (written by the test, little-endian): uint32 ncases; per case: uint32 H, W, subsampling (ELD_JPEG_444 / ELD_JPEG_420), segment
// (blocks); 128 uint16: the divisors, natural order, luma then chroma; ELD_JPEG_TABLE uint32: the code tables; 3 * H * W bytes: the planes.
// Per case the program does what the kernels do, in the kernels' cut: a block at a time jpeg_block_coef fills the coefficient buffer; every
// segment's histogram is counted block by block (jpeg_block_hist); every segment is split into the runs of 256 lanes, each run's bits are
// counted (jpeg_run_bits), a serial prefix sum stands for the scans and for the host's plan, and jpeg_run_pack ORs the run into a dword image
// of the segment's exact size -- a plain OR stands for the atomic one -- which then goes, byte-swapped, into the scan's buffer.  Every buffer is
// a heap allocation of its exact size, so any access outside it stops the program under AddressSanitizer, and any undefined shift or overflow
// under UBSan.
// out.bin: per case uint32 nblocks, nblocks * 64 int16 coefficients, ELD_JPEG_HIST uint32 (the histograms summed over the segments), uint32 nbytes
// and the unstuffed entropy-coded bytes; the test compares all of it with its reference encoder.
// Over all cases the runs must have covered a run starting at each bit phase 0..31, the longest words there are (a DC word of 16 + 11 bits and
// an AC word of 16 + 10; the test sends two cases with 16-bit codes for that) and four segment boundaries inside a picture; the program prints
// what it saw and "hostcheck OK", with exit status 0 only then.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../eld_amd/csrc/jpeg_dev.h"

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

struct HeapAdd {
    uint32_t* h;
    bool overflow;
    void operator()(uint32_t bin) {
        if (bin >= (uint32_t)ELD_JPEG_HIST) { overflow = true; return; }
        h[bin] += 1u;
    }
};

struct LongestSink {                                                 // the longest words (code and extra bits) of a block
    const uint32_t* dct;
    const uint32_t* act;
    uint32_t dc_bits, ac_bits;
    bool missing;
    void dc(uint32_t d) {
        uint32_t nb;
        (void)dng_enc_word(d, dct, &nb);
        missing |= nb == 0;
        dc_bits = nb > dc_bits ? nb : dc_bits;
    }
    void ac(uint32_t sym, int v) {
        uint32_t nb;
        (void)jpeg_ac_word(sym, v, act, &nb);
        missing |= nb == 0;
        ac_bits = nb > ac_bits ? nb : ac_bits;
    }
};

bool seen_phase[32];
uint32_t longest_dc = 0, longest_ac = 0, boundaries = 0;

struct Run { uint32_t first, count, bits; };

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: jpeg_hostcheck cases.bin out.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    uint32_t ncases = 0;
    if (!read_exact(f, &ncases, 4) || ncases < 1 || ncases > 1000) { fprintf(stderr, "bad case count\n"); return 2; }
    for (uint32_t ci = 0; ci < ncases; ++ci) {
        uint32_t hd[4];
        uint16_t* q = (uint16_t*)malloc(128 * sizeof(uint16_t));
        uint32_t* tables = (uint32_t*)malloc(ELD_JPEG_TABLE * sizeof(uint32_t));
        if (!read_exact(f, hd, sizeof(hd)) || !read_exact(f, q, 128 * sizeof(uint16_t)) || !read_exact(f, tables, ELD_JPEG_TABLE * sizeof(uint32_t))) {
            fprintf(stderr, "bad case header\n");
            return 2;
        }
        const uint32_t H = hd[0], W = hd[1], sub = hd[2], segment = hd[3];
        JpegGeom g;
        if (H > 4096 || W > 4096 || !jpeg_geom(&g, (int)H, (int)W, (int)sub) || segment < ELD_JPEG_MIN_SEGMENT || segment > ELD_JPEG_MAX_SEGMENT ||
            segment % ELD_JPEG_MIN_SEGMENT) { fprintf(stderr, "case %u: bad geometry\n", ci); return 2; }
        for (int i = 0; i < 128; ++i)
            if (q[i] < 1 || q[i] > 255) { fprintf(stderr, "case %u: bad divisor\n", ci); return 2; }
        const size_t npix = (size_t)H * W;
        uint8_t* rgb = (uint8_t*)malloc(3 * npix);
        if (!read_exact(f, rgb, 3 * npix)) { fprintf(stderr, "bad picture\n"); return 2; }
        JpegSrc src;
        src.rgb = rgb; src.H = (int)H; src.W = (int)W;
        // coef: a block at a time into a buffer of the exact size
        int16_t* coef = (int16_t*)malloc((size_t)g.nblocks * 64 * sizeof(int16_t));
        for (uint32_t b = 0; b < g.nblocks; ++b) {
            int16_t* blk = (int16_t*)malloc(64 * sizeof(int16_t));
            jpeg_block_coef(src, g, q, b, blk);
            memcpy(coef + (size_t)b * 64, blk, 64 * sizeof(int16_t));
            free(blk);
        }
        const JpegCoefMem cm = {coef};
        // hist: per segment, summed
        uint32_t* hist = (uint32_t*)calloc(ELD_JPEG_HIST, sizeof(uint32_t));
        HeapAdd add = {hist, false};
        for (uint32_t b = 0; b < g.nblocks; ++b) jpeg_block_hist(cm, g, b, add);
        if (add.overflow) { fprintf(stderr, "case %u: a bin beyond the histogram\n", ci); return 1; }
        // pack: the cut of the kernel
        const uint32_t run = (segment + LANES - 1) / LANES;
        uint64_t total = 0;
        std::vector<std::vector<Run>> segs;
        for (uint32_t s0 = 0; s0 < g.nblocks; s0 += segment) {
            const uint32_t sc = g.nblocks - s0 < segment ? g.nblocks - s0 : segment;
            std::vector<Run> runs;
            for (uint32_t l = 0; l < LANES && l * run < sc; ++l) {
                Run r;
                r.first = s0 + l * run;
                r.count = sc - l * run < run ? sc - l * run : run;
                r.bits = jpeg_run_bits(cm, g, tables, r.first, r.count);
                total += r.bits;
                runs.push_back(r);
            }
            segs.push_back(runs);
        }
        if (total == 0 || total >= (1ull << 31)) { fprintf(stderr, "case %u: %llu bits\n", ci, (unsigned long long)total); return 1; }
        boundaries += (uint32_t)segs.size() - 1;
        const uint32_t pad = (uint32_t)((0 - total) & 7u);
        const uint32_t nraw = (uint32_t)((total + 7) / 8), raw_dwords = (uint32_t)((total + pad + 31) / 32);
        uint32_t* raw = (uint32_t*)calloc(raw_dwords, sizeof(uint32_t));
        uint64_t b0 = 0;
        for (size_t si = 0; si < segs.size(); ++si) {
            uint32_t seg_bits = 0;
            for (const Run& r : segs[si]) seg_bits += r.bits;
            const bool last = si + 1 == segs.size();
            const uint32_t phase = (uint32_t)(b0 & 31u), ndw = (phase + seg_bits + (last ? pad : 0u) + 31u) >> 5;
            HeapOr put;
            put.img = (uint32_t*)calloc(ndw ? ndw : 1, sizeof(uint32_t)); put.ndw = ndw; put.overflow = false;
            uint32_t ex = 0;
            for (size_t i = 0; i < segs[si].size(); ++i) {
                const Run& r = segs[si][i];
                seen_phase[(phase + ex) & 31u] = true;
                for (uint32_t b = r.first; b < r.first + r.count; ++b) {
                    const bool c = jpeg_comp(g, b % g.bpm) != 0;
                    LongestSink ls = {tables + (c ? JPEG_TAB_DC : 0u), tables + (c ? JPEG_TAB_AC1 : JPEG_TAB_AC0), 0u, 0u, false};
                    jpeg_walk(cm.block(b), jpeg_pred(cm, g, b), ls);
                    if (ls.missing) { fprintf(stderr, "case %u: block %u uses a symbol the tables lack\n", ci, b); return 1; }
                    longest_dc = ls.dc_bits > longest_dc ? ls.dc_bits : longest_dc;
                    longest_ac = ls.ac_bits > longest_ac ? ls.ac_bits : longest_ac;
                }
                const bool tail = last && i + 1 == segs[si].size();
                jpeg_run_pack(cm, g, tables, r.first, r.count, phase + ex, tail ? pad : 0u, put);
                ex += r.bits;
            }
            if (put.overflow) { fprintf(stderr, "case %u: a dword beyond the image of segment %zu\n", ci, si); return 1; }
            const size_t dw0 = (size_t)(b0 >> 5);
            for (uint32_t i = 0; i < ndw; ++i) {
                if (dw0 + i >= raw_dwords) { fprintf(stderr, "case %u: a dword beyond the scan\n", ci); return 1; }
                raw[dw0 + i] |= __builtin_bswap32(put.img[i]);
            }
            free(put.img);
            b0 += seg_bits;
        }
        if (fwrite(&g.nblocks, 4, 1, o) != 1 || fwrite(coef, sizeof(int16_t), (size_t)g.nblocks * 64, o) != (size_t)g.nblocks * 64 ||
            fwrite(hist, 4, ELD_JPEG_HIST, o) != ELD_JPEG_HIST || fwrite(&nraw, 4, 1, o) != 1 || fwrite(raw, 1, nraw, o) != nraw) {
            fprintf(stderr, "cannot write %s\n", argv[2]);
            return 2;
        }
        printf("case %u: %u x %u, subsampling %u, segment %u: %u blocks, %zu segments, %llu bits, %u bytes\n", ci, H, W, sub, segment, g.nblocks,
               segs.size(), (unsigned long long)total, nraw);
        free(raw); free(hist); free(coef); free(rgb); free(tables); free(q);
    }
    fclose(f);
    if (fclose(o) != 0) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    int phases = 0;
    for (int i = 0; i < 32; ++i) phases += seen_phase[i] ? 1 : 0;
    printf("coverage: longest DC word %u bits, longest AC word %u bits, %d of 32 start phases, %u segment boundaries\n", longest_dc, longest_ac, phases,
           boundaries);
    if (longest_dc != 27 || longest_ac != 26 || phases != 32 || boundaries < 4) { fprintf(stderr, "the cases do not cover what they must\n"); return 1; }
    printf("hostcheck OK\n");
    return 0;
}
