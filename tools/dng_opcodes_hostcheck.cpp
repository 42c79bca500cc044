// dng_opcodes_hostcheck.cpp -- the per-site opcode evaluator of csrc/dng_opcodes_dev.h under a host compiler and its sanitizers
// (tests/test_dng_opcodes_cpu.py builds this with -fsanitize=address,undefined -ffp-contract=off and runs it; it never runs on a GPU).
//
//   dng_opcodes_hostcheck cases.bin
//
// cases.bin (written by the test, little-endian): uint32 ncases; per case uint32 Hm, Wm, nops, blob_bytes, gain_mode, nsites; the EldDngOp
// records (104 bytes each); the blob; nsites x (int32 y, int32 x, float32 in, float32 expect).
// 1. every site of every case evaluates to the expected bits (the values come from tests/dng_opcodes_ref.py);
// 2. 4000 single-field corruptions of the valid records from a fixed seed (an integer field, or one of the float64 parameters): the corrupted
//    record runs alone and inside its program on a handful of sites; when opc_record_ok refuses it, the site keeps its value (1 in gain mode);
// 3. records that point outside the blob (data_off at and around its end, counts that run beyond it) are refused: sites unchanged.
// The records and the blob are heap allocations of their exact size, so any read outside them stops the program under AddressSanitizer.
// Prints one line per stage and "hostcheck OK"; exit status 0 only then.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../eld_amd/csrc/dng_opcodes_dev.h"

namespace {

struct Site {
    int32_t y, x;
    float in, expect;
};

struct Case {
    uint32_t Hm, Wm, nops, blob_bytes, gain_mode, nsites;
    std::vector<EldDngOp> ops;
    std::vector<uint8_t> blob;
    std::vector<Site> sites;
};

bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return u;
}

// the program on exact-size heap copies of the records and the blob
float run(const Case& c, const std::vector<EldDngOp>& ops, int y, int x, float v) {
    EldDngOp* o = (EldDngOp*)malloc(ops.size() * sizeof(EldDngOp) + (ops.empty() ? 1 : 0));
    if (!ops.empty()) memcpy(o, ops.data(), ops.size() * sizeof(EldDngOp));
    uint8_t* blob = (uint8_t*)malloc(c.blob.size() ? c.blob.size() : 1);
    if (!c.blob.empty()) memcpy(blob, c.blob.data(), c.blob.size());
    const float r = opc_eval_site(o, (int)ops.size(), blob, c.blob.size(), (int)c.Hm, (int)c.Wm, y, x, v, c.gain_mode != 0);
    free(blob);
    free(o);
    return r;
}

uint32_t rng_state = 2018u;
uint32_t rnd() {                                                     // xorshift32
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state;
}

int32_t nasty_int(const Case& c) {
    switch (rnd() % 10u) {
        case 0: return 0;
        case 1: return -1;
        case 2: return 1;
        case 3: return std::numeric_limits<int32_t>::max();
        case 4: return std::numeric_limits<int32_t>::min();
        case 5: return (int32_t)c.blob_bytes - 8 + (int32_t)(rnd() % 17u);
        case 6: return (int32_t)(rnd() % 64u);
        case 7: return -(int32_t)(rnd() % 64u);
        case 8: return (int32_t)(rnd() % (2u * (c.Hm + c.Wm)));
        default: return (int32_t)rnd();
    }
}

double nasty_double() {
    static const double v[] = {0.0, -0.0, 1e300, -1e300, 1e-300, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                               -std::numeric_limits<double>::infinity(), 0.5, -3.0, 1e9};
    return v[rnd() % (sizeof(v) / sizeof(v[0]))];
}

// a refused record leaves every probed site as it was; a record that is still valid only has to stay inside its buffers
bool probe(const Case& c, const std::vector<EldDngOp>& ops, size_t which, const char* what) {
    const EldDngOp& bad = ops[which];
    const bool ok = opc_record_ok(bad, c.blob.size(), (int)c.Hm, (int)c.Wm);
    const std::vector<EldDngOp> alone(1, bad);
    for (int k = 0; k < 6; ++k) {
        int y, x;
        if (k == 0) { y = 0; x = 0; }
        else if (k == 1) { y = (int)c.Hm - 1; x = (int)c.Wm - 1; }
        else { y = (int)(rnd() % c.Hm); x = (int)(rnd() % c.Wm); }
        const float in = (float)(rnd() % 1001u) / 1000.f;
        (void)run(c, ops, y, x, in);
        const float r = run(c, alone, y, x, in);
        if (!ok && bits(r) != bits(c.gain_mode ? 1.f : in)) {
            printf("%s: a refused record changed site (%d, %d): %.9g -> %.9g\n", what, y, x, (double)in, (double)r);
            return false;
        }
    }
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    static_assert(sizeof(EldDngOp) == 104, "the record the test writes");
    if (argc != 2) {
        fprintf(stderr, "usage: dng_opcodes_hostcheck cases.bin\n");
        return 2;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    uint32_t ncases = 0;
    if (!read_exact(f, &ncases, 4) || ncases < 1 || ncases > 64) return 2;
    std::vector<Case> cases(ncases);
    for (auto& c : cases) {
        if (!read_exact(f, &c.Hm, 24) || c.nops > ELD_DNG_MAX_OPS || c.blob_bytes > (1u << 24) || c.nsites > (1u << 20) || c.Hm < 1 || c.Wm < 1) return 2;
        c.ops.resize(c.nops);
        c.blob.resize(c.blob_bytes);
        c.sites.resize(c.nsites);
        if (!read_exact(f, c.ops.data(), c.nops * sizeof(EldDngOp)) || !read_exact(f, c.blob.data(), c.blob_bytes) ||
            !read_exact(f, c.sites.data(), c.nsites * sizeof(Site)))
            return 2;
    }
    fclose(f);
    // 1. the expected values
    size_t nsites = 0;
    for (size_t i = 0; i < cases.size(); ++i) {
        const Case& c = cases[i];
        for (const auto& op : c.ops)
            if (!opc_record_ok(op, c.blob.size(), (int)c.Hm, (int)c.Wm)) {
                printf("case %zu: a record of the test's own program is refused\n", i);
                return 1;
            }
        for (const Site& s : c.sites) {
            const float r = run(c, c.ops, s.y, s.x, s.in);
            if (bits(r) != bits(s.expect)) {
                printf("case %zu site (%d, %d): %.9g -> %.9g (%08x), expected %.9g (%08x)\n", i, s.y, s.x, (double)s.in, (double)r, bits(r),
                       (double)s.expect, bits(s.expect));
                return 1;
            }
            ++nsites;
        }
    }
    printf("%zu sites of %zu cases: the expected bits\n", nsites, cases.size());
    // 2. single-field corruptions
    int refused = 0;
    const int trials = 4000;
    for (int t = 0; t < trials; ++t) {
        const Case& c = cases[rnd() % cases.size()];
        if (c.ops.empty()) continue;
        std::vector<EldDngOp> ops = c.ops;
        const size_t which = rnd() % ops.size();
        const uint32_t field = rnd() % 17u;                           // 10 integer fields, 7 float64 parameters
        if (field < 10u) {
            int32_t* w = (int32_t*)&ops[which];
            w[field] = nasty_int(c);
        } else {
            ops[which].p[field - 10u] = nasty_double();
        }
        refused += !opc_record_ok(ops[which], c.blob.size(), (int)c.Hm, (int)c.Wm);
        if (!probe(c, ops, which, "corruption")) return 1;
    }
    printf("%d single-field corruptions: %d refused, every refused record left its sites unchanged\n", trials, refused);
    // 3. records that point outside the blob
    int outside = 0;
    for (const Case& c : cases) {
        for (size_t which = 0; which < c.ops.size(); ++which) {
            if (opc_data_bytes(c.ops[which]) == 0) continue;
            for (int d = -16; d <= 16; d += 4) {
                std::vector<EldDngOp> ops = c.ops;
                ops[which].data_off = (uint32_t)((int64_t)c.blob.size() + d);
                const bool must_refuse = (uint64_t)ops[which].data_off + opc_data_bytes(ops[which]) > c.blob.size();
                if (must_refuse && opc_record_ok(ops[which], c.blob.size(), (int)c.Hm, (int)c.Wm)) {
                    printf("a record whose data ends beyond the blob is accepted\n");
                    return 1;
                }
                if (!probe(c, ops, which, "outside the blob")) return 1;
                outside += must_refuse;
            }
            std::vector<EldDngOp> ops = c.ops;
            ops[which].data_off = 0xFFFFFFFCu;
            if (opc_record_ok(ops[which], c.blob.size(), (int)c.Hm, (int)c.Wm) || !probe(c, ops, which, "outside the blob")) {
                printf("a record at the end of the 32-bit range is accepted or followed\n");
                return 1;
            }
            ++outside;
        }
    }
    printf("%d records pointing outside the blob: refused, sites unchanged\n", outside);
    printf("hostcheck OK\n");
    return 0;
}
