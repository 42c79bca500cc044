// burst_dev.h -- what the two burst stacks share (burst.hip: a tripod burst; align.hip: a burst gathered through a displacement field): the
// leave-one-out rule for one sample and the photon-transfer accumulation (per-lane runs -> copies of the table in LDS -> 64-bit integer
// atomics into ptc[]).  Widths and the reasoning behind both are at the head of burst.hip; DESIGN.md sec. 20.
#pragma once
#include "levelbins.h"
#include "mosaic_dev.h"

namespace {

constexpr int BT = 256;                          // threads per workgroup
constexpr int BS_TW = 4 * PS_NB;                 // table entries (G <= 4)
constexpr int BS_COPIES = 4;                     // 23.6 KB of LDS: six workgroups fit a CU, the registers allow four
constexpr int BS_OFF_V = 2 * BS_TW;              // words: TW double words of sum S1, TW double words of sum Vlo, TW words n, TW words sum Vhi
constexpr int BS_OFF_N = 4 * BS_TW;
constexpr int BS_OFF_H = 5 * BS_TW;
constexpr int BS_STRIDE = 1474;                  // >= 6 * TW = 1464, even, and 2 modulo 32
static_assert(BS_STRIDE >= 6 * BS_TW && BS_STRIDE % 32 == 2, "LDS layout");
static_assert(BS_COPIES * BS_STRIDE * 4 <= 65536, "static LDS");
static_assert(256ll * 65535 < (1ll << 24) && 256ll * 65535 * 65535 < (1ll << 40), "S1, |d| < 2^24 and S2 < 2^40");
static_assert(255ull * 255 * 65535 * 65535 / 4 < (1ull << 46) && 256ull * 256 * 65535 * 65535 / 4 < (1ull << 46), "V1, V < 2^46");
static_assert(4ull * 254 * (255ull * 65535) * (255ull * 65535) < (1ull << 58), "4 (N - 2) d^2 < 2^58");

// The rule for one sample x of a site with sums s1, s2 over its n samples (n >= 4, k2q > 0: the caller decides whether the rule is on).
struct BurstRule {
    uint32_t n, dev_floor, c_left, c_right;      // (n - 1) min_dev < 2^24, 4 (n - 2) < 2^10, k2q (n - 1) <= 2^16
    __device__ __forceinline__ BurstRule(int n_, int k2q, int min_dev)
        : n((uint32_t)n_), dev_floor((uint32_t)(n_ - 1) * (uint32_t)min_dev), c_left(4u * (uint32_t)(n_ - 2)), c_right((uint32_t)k2q * (uint32_t)(n_ - 1)) {}
    __device__ __forceinline__ bool rejected(uint32_t x, uint32_t s1, unsigned long long s2) const {
        const int32_t d = (int32_t)(n * x) - (int32_t)s1;
        const uint32_t ad = d < 0 ? (uint32_t)-d : (uint32_t)d;
        if (ad <= dev_floor) return false;
        const unsigned long long d2 = (unsigned long long)ad * ad;                                 // < 2^48
        const uint32_t r1 = s1 - x;
        const unsigned long long v1 = (unsigned long long)(n - 1) * (s2 - (unsigned long long)(x * x)) - (unsigned long long)r1 * r1;   // < 2^46
        return d2 * c_left > v1 * c_right;                                                         // < 2^58, < 2^62
    }
};

// the pending run of one column parity
struct Run {
    int key;
    uint32_t n, vhi;
    unsigned long long s1, vlo;
};

__device__ __forceinline__ void run_clear(Run& r) { r.key = -1; r.n = 0; r.vhi = 0; r.s1 = 0; r.vlo = 0; }

__device__ __forceinline__ void run_flush(uint32_t* __restrict__ tab, const Run& r) {
    if (r.key >= 0) {
        atomicAdd(reinterpret_cast<unsigned long long*>(tab) + r.key, r.s1);
        atomicAdd(reinterpret_cast<unsigned long long*>(tab + BS_OFF_V) + r.key, r.vlo);
        atomicAdd(tab + BS_OFF_N + r.key, r.n);
        atomicAdd(tab + BS_OFF_H + r.key, r.vhi);
    }
}

// one eligible site joins its run, or flushes it and starts the next
__device__ __forceinline__ void run_add(uint32_t* __restrict__ tab, Run& r, int key, uint32_t s1, unsigned long long v) {
    if (key == r.key) {
        r.n += 1; r.vhi += (uint32_t)(v >> 32); r.s1 += s1; r.vlo += (uint32_t)v;
    } else {
        run_flush(tab, r);
        r.key = key; r.n = 1; r.vhi = (uint32_t)(v >> 32); r.s1 = s1; r.vlo = (uint32_t)v;
    }
}

// after the workgroup's last run_flush and a barrier: the copies of the table meet in ptc[]
__device__ __forceinline__ void ptc_merge(const uint32_t* __restrict__ lds, unsigned long long* __restrict__ ptc, int G) {
    const int tw = G * PS_NB;
    for (int k = threadIdx.x; k < tw; k += BT) {
        uint32_t n = 0, vhi = 0;
        unsigned long long s1 = 0, vlo = 0;
        for (int c = 0; c < BS_COPIES; ++c) {
            const uint32_t* t = lds + c * BS_STRIDE;
            s1 += reinterpret_cast<const unsigned long long*>(t)[k];
            vlo += reinterpret_cast<const unsigned long long*>(t + BS_OFF_V)[k];
            n += t[BS_OFF_N + k];
            vhi += t[BS_OFF_H + k];
        }
        unsigned long long* o = ptc + 4 * k;
        if (n) {                                                 // an entry without sites has all four sums zero
            atomicAdd(o, (unsigned long long)n);
            atomicAdd(o + 1, s1);
            if (vlo) atomicAdd(o + 2, vlo);
            if (vhi) atomicAdd(o + 3, (unsigned long long)vhi);
        }
    }
}

}  // namespace
