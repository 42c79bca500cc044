// dng_hostcheck.cpp -- the per-stream lossless-JPEG decoder of csrc/dng_dev.h under a host compiler and its sanitizers (tests/test_dng_cpu.py
// builds this with -fsanitize=address,undefined and runs it; it never runs on a GPU).
//
//   dng_hostcheck cases.bin
//
// cases.bin (written by the test, little-endian): uint32 ncases; per case: EldDngStream record (64 bytes), uint32 ntables, the EldDngHuff
// records, uint32 nbytes, the stream's entropy-coded bytes (the record's data_off is 0 and data_len nbytes), uint32 nexpect, nexpect uint16:
// the samples the tile must hold after the decode (tw * th, row-major).
// 1. every case decodes with status ok and the expected samples;
// 2. every truncation of case 0 (each length 0 .. nbytes - 1) ends with a status; ok only where the cut removed nothing but padding bits or the
//    EOI marker, and then the samples are still the expected ones;
// 3. 4000 single-byte corruptions of case 0 from a fixed seed, and the same with the record's geometry enlarged (more samples than the tile):
//    each run ends with one of the five status words.
// Every buffer is a heap allocation of its exact size, so any read or write outside it stops the program under AddressSanitizer.
// Prints one line per stage and "hostcheck OK"; exit status 0 only then.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../eld_amd/csrc/dng_dev.h"

namespace {

struct Case {
    EldDngStream rec;
    std::vector<EldDngHuff> tables;
    std::vector<uint8_t> data;
    std::vector<uint16_t> expect;
};

bool read_exact(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

// one decode with exact-size heap buffers; -> status, the tile in `tile`
int run(const Case& c, const EldDngStream& rec, const uint8_t* bytes, size_t nbytes, std::vector<uint16_t>& tile) {
    uint8_t* blob = (uint8_t*)malloc(nbytes ? nbytes : 1);
    if (nbytes) memcpy(blob, bytes, nbytes);
    const size_t ws_elems = (size_t)c.rec.X * (size_t)c.rec.Nf;      // the room the honest record asked for
    uint16_t* ws = (uint16_t*)malloc(ws_elems * sizeof(uint16_t));
    memset(ws, 0, ws_elems * sizeof(uint16_t));
    const size_t n = (size_t)c.rec.tw * (size_t)c.rec.th;
    uint16_t* out = (uint16_t*)malloc(n * sizeof(uint16_t));
    memset(out, 0, n * sizeof(uint16_t));
    EldDngHuff* tabs = (EldDngHuff*)malloc(c.tables.size() * sizeof(EldDngHuff));
    memcpy(tabs, c.tables.data(), c.tables.size() * sizeof(EldDngHuff));
    DngOut o;
    o.out = out; o.H = c.rec.th; o.W = c.rec.tw; o.top = 0; o.left = 0; o.Hm = c.rec.th; o.Wm = c.rec.tw; o.lin = nullptr; o.lin_len = 0;
    EldDngStream r = rec;
    r.data_off = 0; r.data_len = (uint32_t)nbytes; r.x0 = 0; r.y0 = 0; r.ws_off = 0;
    const int st = dng_ljpeg_stream(blob, nbytes, r, tabs, (int)c.tables.size(), ws, ws_elems, o);
    tile.assign(out, out + n);
    free(tabs); free(out); free(ws); free(blob);
    return st;
}

uint32_t rng_state = 2018u;
uint32_t rnd() {                                                     // xorshift32
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: dng_hostcheck cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t ncases = 0;
    if (!read_exact(f, &ncases, 4) || ncases < 1 || ncases > 1000) { fprintf(stderr, "bad case count\n"); return 2; }
    std::vector<Case> cases(ncases);
    for (auto& c : cases) {
        uint32_t n = 0;
        if (!read_exact(f, &c.rec, sizeof(c.rec)) || !read_exact(f, &n, 4) || n < 1 || n > 16) { fprintf(stderr, "bad case header\n"); return 2; }
        c.tables.resize(n);
        if (!read_exact(f, c.tables.data(), n * sizeof(EldDngHuff)) || !read_exact(f, &n, 4) || n > (1u << 24)) { fprintf(stderr, "bad tables\n"); return 2; }
        c.data.resize(n);
        if ((n && !read_exact(f, c.data.data(), n)) || !read_exact(f, &n, 4) || n > (1u << 24)) { fprintf(stderr, "bad data\n"); return 2; }
        c.expect.resize(n);
        if (n && !read_exact(f, c.expect.data(), n * 2)) { fprintf(stderr, "bad expectation\n"); return 2; }
    }
    fclose(f);
    std::vector<uint16_t> tile;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        const int st = run(c, c.rec, c.data.data(), c.data.size(), tile);
        if (st != ELD_DNG_OK || tile != c.expect) { fprintf(stderr, "case %zu: status %d, samples %s\n", i, st, tile == c.expect ? "equal" : "differ"); return 1; }
    }
    printf("%zu streams decode to the expected samples\n", cases.size());
    const Case& c0 = cases[0];
    int count[5] = {0, 0, 0, 0, 0};
    for (size_t len = 0; len < c0.data.size(); ++len) {
        const int st = run(c0, c0.rec, c0.data.data(), len, tile);
        if (st < 0 || st > 4) { fprintf(stderr, "truncation to %zu bytes: status %d\n", len, st); return 1; }
        if (st == ELD_DNG_OK && tile != c0.expect) { fprintf(stderr, "truncation to %zu bytes: ok with other samples\n", len); return 1; }
        count[st]++;
    }
    if (count[ELD_DNG_TRUNCATED] == 0) { fprintf(stderr, "no truncation was reported as truncated\n"); return 1; }
    printf("%zu truncations: %d ok (padding or EOI cut), %d truncated, %d invalid code\n", c0.data.size(), count[0], count[1], count[2]);
    int seen[5] = {0, 0, 0, 0, 0};
    std::vector<uint8_t> bytes;
    for (int pass = 0; pass < 2; ++pass) {
        EldDngStream rec = c0.rec;
        if (pass == 1) rec.Y = rec.Y + 3;                            // more samples than the tile: the decoder must stop at the tile's end
        for (int k = 0; k < 4000; ++k) {
            bytes = c0.data;
            bytes[rnd() % bytes.size()] = (uint8_t)rnd();
            const int st = run(c0, rec, bytes.data(), bytes.size(), tile);
            if (st < 0 || st > 4) { fprintf(stderr, "corruption %d of pass %d: status %d\n", k, pass, st); return 1; }
            seen[st]++;
        }
    }
    // the enlarged record on the intact stream: the data lasts for the tile, so the end of the tile is what stops it
    {
        EldDngStream rec = c0.rec;
        rec.Y = rec.Y + 3;
        const int st = run(c0, rec, c0.data.data(), c0.data.size(), tile);
        if (st != ELD_DNG_TOOMANY) { fprintf(stderr, "enlarged record: status %d\n", st); return 1; }
        if (tile != c0.expect) { fprintf(stderr, "enlarged record: the tile's samples changed\n"); return 1; }
    }
    // a record that points outside its buffers is refused before a byte is read
    {
        EldDngStream rec = c0.rec;
        rec.table[0] = 999;
        if (run(c0, rec, c0.data.data(), c0.data.size(), tile) != ELD_DNG_BADRECORD) { fprintf(stderr, "table index 999 accepted\n"); return 1; }
        rec = c0.rec;
        rec.X = 60000;
        rec.pred = 7;
        if (run(c0, rec, c0.data.data(), c0.data.size(), tile) != ELD_DNG_BADRECORD) { fprintf(stderr, "a row beyond the workspace accepted\n"); return 1; }
    }
    printf("8000 corruptions: %d ok, %d truncated, %d invalid code, %d too many samples, %d bad record\n", seen[0], seen[1], seen[2], seen[3], seen[4]);
    printf("hostcheck OK\n");
    return 0;
}
