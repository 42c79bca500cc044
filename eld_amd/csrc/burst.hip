// burst.hip -- stack a burst of a static scene: robust per-site mean and exact photon-transfer sums (eld_amd/burst.py).
//
//   eld_burst_stack_u16   frames uint16 [N,Hm,Wm], 2 <= N <= 256 -> mean uint16 [Hm,Wm], kept uint8 [Hm,Wm], ptc int64 [G][61][4]
// Per site, over its N samples x: S1 = sum x, S2 = sum x^2, min, max.  Leave-one-out rejection (N >= 4 and k2q > 0): with d = N x - S1 and
// V1 = (N - 1)(S2 - x^2) - (S1 - x)^2 the sample is rejected iff |d| > (N - 1) min_dev and 4 d^2 (N - 2) > k2q (N - 1) V1.  mean = the kept
// samples' mean rounded half up, kept = their count (256 is written as 0).  ptc[g][bin] += (1, S1, V mod 2^32, V >> 32), V = N S2 - S1^2, for the
// eligible sites: group >= 0, not flagged, nothing rejected, max < white, min > 0; bin = bin_of(mean, mean - black[cell], white) (levelbins.h).
//
// Operand widths (x <= 65535 = R, N <= 256, k2q <= 256, min_dev <= 65535):
//   S1 <= 256 R < 2^24 (uint32), S2 <= 256 R^2 < 2^40 (uint64), |d| <= (N - 1) R < 2^24 (int32), (N - 1) min_dev < 2^24, d^2 < 2^48;
//   V1 = n sum' x^2 - (sum' x)^2 over the n = N - 1 other samples, so 0 <= V1 <= n^2 R^2 / 4 < 2^46 (the variance of n values in [0, R] is at
//   most R^2 / 4); its two terms (N - 1)(S2 - x^2) < 2^48 and (S1 - x)^2 < 2^48;
//   left side 4 (N - 2) d^2 < 2^10 2^48 = 2^58, right side k2q (N - 1) V1 < 2^8 2^8 2^46 = 2^62: both fit unsigned 64 bits;
//   V = N S2 - S1^2 <= N^2 R^2 / 4 < 2^46; the mean's numerator 2 S + n < 2^26.
//
// The rule in terms of the whole site: N V1 = (N - 1) V - d^2, so the right side falls and the left side rises with |d|: a sample is rejected
// iff every sample at least as far from the site's mean is.  Hence (a) nothing is rejected at a site unless its furthest sample is, and with
// the identity the rule reads d^2 A > V B, A = 4 N (N - 2) + k2q (N - 1) < 2^19, B = k2q (N - 1)^2 < 2^24: one test per site on
// max |d| = max(N max - S1, S1 - N min) and on the V that ptc needs anyway.  The products can exceed 64 bits (2^67, 2^70), so both sides
// drop their `shift` low bits first, the left side rounded up and the right side down: ((d^2 >> shift) + 1) A > (V >> shift) B holds
// whenever the rule does (the host picks the smallest shift without overflow from N and k2q: 0 up to N of about 100).  The second look at
// the samples is taken only by the sites that pass this test (a fraction of a percent of a real burst) and applies the rule as written
// to each sample, so a site the test passes without need just keeps all N; and (b) summing
// the rule over all samples of a site gives 4 (N - 2) N V on the left and k2q (N - 1)(N - 2) V on the right: every sample can be rejected only
// if 4 N > k2q (N - 1), that is k2q <= 5 (k < 1.2); from k2q = 6 on at least one sample is kept.  For the k2q <= 5 that the interface still
// accepts a site may lose all samples: n = 0 writes mean = 0 and kept = 0.
//
// One streaming pass, 2 N bytes read per site: a lane owns CW adjacent columns of one row (a "unit") and reads them frame by frame, four
// frames' loads in flight.
//   * CW = 8  frames and mean 16-byte aligned, kept 8-byte aligned, Wm % 8 == 0: one 16-byte load per frame
//   * CW = 2  frames and mean 4-byte aligned, kept 2-byte aligned, Wm even: one 32-bit word per frame
//   * CW = 1  anything else: 2-byte loads
// The second look re-reads the unit's N loads right after the first (the lines were just read by this lane: L2 / Infinity Cache hits) and
// evaluates the rule for the flagged sites of the unit only.
// ptc accumulates like pairstats.hip: per lane one pending run per column parity (a constant region costs no LDS add), BS_COPIES copies of
// the table in LDS with a copy stride of 2 modulo 32 words, then at most G * 61 * 4 64-bit global integer atomics per workgroup of
// BS_UNITS * CW <= 16384 sites into ptc[], which a kernel of this call zeroes first.  Integer adds only: any arrival order gives the same
// bits.  No floating point, no environment switch, no workspace.
#include "burst_dev.h"

namespace {

constexpr int BS_TURNS = 8;                      // units per lane
constexpr int BS_UNITS = BT * BS_TURNS;          // 2048 units per workgroup (eld_amd/burst.py TILE_UNITS mirrors it for the tests)
constexpr int BS_DEPTH = 4;                      // frames whose loads are in flight
static_assert((long long)BS_UNITS * 8 * (1 << 14) < (1ll << 32), "32-bit partial sums of V >> 32 (V < 2^46) and of the site count");

struct BurstArgs {
    const uint16_t* frames;
    const uint32_t* bitmap;
    uint16_t* mean;
    uint8_t* kept;
    unsigned long long* ptc;
    int N, Wm, G, white, wpr, k2q, min_dev, shift;
    uint32_t pre_a, pre_b;                       // A, B of the per-site test (head of the file)
    uint32_t hw, upr, units;                     // sites per frame, units per row, units per frame
    FastDiv dupr;
    int32_t tab[36];                             // cell -> black | (group + 1) << 16
};

template <int P, int CW>
__global__ __launch_bounds__(BT) void burst_stack_kernel(BurstArgs a) {
    constexpr int NW = (CW + 1) / 2;
    __shared__ int32_t s_tab[P * CELL_ROW];
    __shared__ unsigned long long s_lds[BS_COPIES * BS_STRIDE / 2];
    uint32_t* lds = reinterpret_cast<uint32_t*>(s_lds);
    const bool want_ptc = a.ptc != nullptr;
    if (want_ptc)
        for (int i = threadIdx.x; i < BS_COPIES * BS_STRIDE; i += BT) lds[i] = 0;
    fill_cell_rows<P>(s_tab, a.tab);
    __syncthreads();
    uint32_t* tab = lds + (threadIdx.x & (BS_COPIES - 1)) * BS_STRIDE;
    const int N = a.N, white = a.white;
    const bool rej_on = N >= 4 && a.k2q > 0;
    const BurstRule rule(N, a.k2q, a.min_dev);
    const uint32_t dev_floor = rule.dev_floor;                   // < 2^24
    Run run[2];
    run_clear(run[0]);
    run_clear(run[1]);

    const uint32_t u0 = blockIdx.x * (uint32_t)BS_UNITS;
    const uint32_t u1 = min(u0 + (uint32_t)BS_UNITS, a.units);
    for (uint32_t u = u0 + threadIdx.x; u < u1; u += BT) {
        const size_t i0 = (size_t)u * CW;                        // the unit's first site: units tile the rows exactly (Wm = upr * CW)
        const uint16_t* src = a.frames + i0;
        uint32_t S1[CW], mn[CW], mx[CW];
        unsigned long long S2[CW];
#pragma unroll
        for (int j = 0; j < CW; ++j) { S1[j] = 0; S2[j] = 0; mn[j] = 65535u; mx[j] = 0; }
        int f = 0;
        for (; f + BS_DEPTH <= N; f += BS_DEPTH) {
            uint32_t w[BS_DEPTH][NW];
#pragma unroll
            for (int k = 0; k < BS_DEPTH; ++k) load_codes<CW>(src + (size_t)(f + k) * a.hw, w[k]);
#pragma unroll
            for (int k = 0; k < BS_DEPTH; ++k)
#pragma unroll
                for (int j = 0; j < CW; ++j) {
                    const uint32_t x = code_of(w[k], j);
                    S1[j] += x; S2[j] += (unsigned long long)(x * x);        // x^2 <= 65535^2 < 2^32
                    mn[j] = min(mn[j], x); mx[j] = max(mx[j], x);
                }
        }
        for (; f < N; ++f) {
            uint32_t w[NW];
            load_codes<CW>(src + (size_t)f * a.hw, w);
#pragma unroll
            for (int j = 0; j < CW; ++j) {
                const uint32_t x = code_of(w, j);
                S1[j] += x; S2[j] += (unsigned long long)(x * x);
                mn[j] = min(mn[j], x); mx[j] = max(mx[j], x);
            }
        }

        // the second look, for the sites whose furthest sample may be rejected (see the head of the file)
        uint32_t Sk[CW], nk[CW];
        unsigned long long V[CW];
        uint32_t need = 0;
#pragma unroll
        for (int j = 0; j < CW; ++j) {
            Sk[j] = S1[j]; nk[j] = (uint32_t)N;
            V[j] = (unsigned long long)(uint32_t)N * S2[j] - (unsigned long long)S1[j] * S1[j];     // < 2^46
            const uint32_t ad = max((uint32_t)N * mx[j] - S1[j], S1[j] - (uint32_t)N * mn[j]);     // both >= 0: N min <= S1 <= N max
            if (rej_on && ad > dev_floor && ((((unsigned long long)ad * ad) >> a.shift) + 1) * a.pre_a > (V[j] >> a.shift) * a.pre_b) need |= 1u << j;
        }
        if (need) {
#pragma unroll
            for (int j = 0; j < CW; ++j)
                if ((need >> j) & 1u) { Sk[j] = 0; nk[j] = 0; }
            auto look = [&](const uint32_t* w) __attribute__((always_inline)) {
#pragma unroll
                for (int j = 0; j < CW; ++j)
                    if ((need >> j) & 1u) {
                        const uint32_t x = code_of(w, j);
                        if (!rule.rejected(x, S1[j], S2[j])) { Sk[j] += x; nk[j] += 1; }
                    }
            };
            int f2 = 0;
            for (; f2 + BS_DEPTH <= N; f2 += BS_DEPTH) {
                uint32_t w[BS_DEPTH][NW];
#pragma unroll
                for (int k = 0; k < BS_DEPTH; ++k) load_codes<CW>(src + (size_t)(f2 + k) * a.hw, w[k]);
#pragma unroll
                for (int k = 0; k < BS_DEPTH; ++k) look(w[k]);
            }
            for (; f2 < N; ++f2) {
                uint32_t w[NW];
                load_codes<CW>(src + (size_t)f2 * a.hw, w);
                look(w);
            }
        }

        const uint32_t y = fdiv_u32(u, a.dupr);
        const uint32_t x0 = (u - y * a.upr) * (uint32_t)CW;
        const int32_t* trow = cell_row<P>(s_tab, y, x0);
        uint32_t bad = 0;
        if (a.bitmap) bad = a.bitmap[(size_t)y * a.wpr + (x0 >> 5)] >> (x0 & 31u);   // defect_bits, written out: the call changes the CW = 1 kernels
        uint32_t m[CW];
#pragma unroll
        for (int j = 0; j < CW; ++j) {
            const uint32_t n = nk[j];
            m[j] = n ? (2u * Sk[j] + n) / (2u * n) : 0u;         // rounds half up; 2 S + n < 2^26
            if (want_ptc) {
                const int t = trow[j];
                const int g = (t >> 16) - 1;
                if (g >= 0 && !((bad >> j) & 1u) && n == (uint32_t)N && (int)mx[j] < white && mn[j] > 0) {
                    const int key = g * PS_NB + bin_of((int)m[j], (int)m[j] - (t & 0xFFFF), white);
                    const unsigned long long v = V[j];
                    Run& r = run[CW % 2 == 0 ? (j & 1) : 0];     // x0 is even when CW is; CW = 1 keeps one run (a static index: registers)
                    run_add(tab, r, key, S1[j], v);
                }
            }
        }
        if constexpr (CW == 8) {
            *reinterpret_cast<uint4*>(a.mean + i0) = make_uint4(m[0] | (m[1] << 16), m[2] | (m[3] << 16), m[4] | (m[5] << 16), m[6] | (m[7] << 16));
            if (a.kept)
                *reinterpret_cast<uint2*>(a.kept + i0) = make_uint2((nk[0] & 255u) | ((nk[1] & 255u) << 8) | ((nk[2] & 255u) << 16) | ((nk[3] & 255u) << 24),
                                                                    (nk[4] & 255u) | ((nk[5] & 255u) << 8) | ((nk[6] & 255u) << 16) | ((nk[7] & 255u) << 24));
        } else if constexpr (CW == 2) {
            *reinterpret_cast<uint32_t*>(a.mean + i0) = m[0] | (m[1] << 16);
            if (a.kept) *reinterpret_cast<uint16_t*>(a.kept + i0) = (uint16_t)((nk[0] & 255u) | ((nk[1] & 255u) << 8));
        } else {
            a.mean[i0] = (uint16_t)m[0];
            if (a.kept) a.kept[i0] = (uint8_t)nk[0];
        }
    }
    if (!want_ptc) return;                                       // launch-uniform
    run_flush(tab, run[0]);
    run_flush(tab, run[1]);

    __syncthreads();
    ptc_merge(lds, a.ptc, a.G);
}

template <int P, int CW>
int launch_burst(const BurstArgs& a, hipStream_t s) {
    ELD_LAUNCH((burst_stack_kernel<P, CW>), dim3((a.units + BS_UNITS - 1) / BS_UNITS), dim3(BT), 0, s, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" size_t eld_burst_stack_workspace_bytes(int N, int Hm, int Wm) {
    (void)N; (void)Hm; (void)Wm;
    return 0;                                                    // the sums meet in LDS and in ptc[] itself
}

extern "C" int eld_burst_stack_u16(const uint16_t* frames, int N, int Hm, int Wm, int p, const int* group, int G, const int32_t* black, int white,
                                   const uint32_t* bitmap, int k2q, int min_dev, uint16_t* mean, uint8_t* kept, int64_t* ptc, void* ws,
                                   size_t ws_bytes, void* stream) {
    if ((p != 2 && p != 6) || Hm < 0 || Wm < 0 || G < 1 || G > 4) return ELD_EINVAL;
    if ((uint64_t)Hm * (uint64_t)Wm >= (1ull << 31) || !cell_groups_ok(p, group, G, black, white)) return ELD_EINVAL;
    if (N < 2 || N > 256 || k2q < 0 || k2q > 256 || min_dev < 0 || min_dev > 65535) return ELD_EINVAL;
    (void)ws;
    if (ws_bytes < eld_burst_stack_workspace_bytes(N, Hm, Wm)) return ELD_EWS;
    if ((uintptr_t)ptc & 7u) return ELD_EINVAL;
    const bool empty = Hm == 0 || Wm == 0;
    if (!empty && (!frames || !mean || ((uintptr_t)frames & 1u) || ((uintptr_t)mean & 1u) || ((uintptr_t)bitmap & 3u))) return ELD_EINVAL;
    hipStream_t s = as_stream(stream);
    if (ptc)
        if (int rc = zero_u64(ptc, (size_t)G * PS_NB * 4, s)) return rc;
    if (empty) return 0;
    BurstArgs a;
    a.frames = frames; a.bitmap = bitmap; a.mean = mean; a.kept = kept; a.ptc = (unsigned long long*)ptc;
    a.N = N; a.Wm = Wm; a.G = G; a.white = white; a.wpr = bitmap_pitch(Wm); a.k2q = k2q; a.min_dev = min_dev;
    a.hw = (uint32_t)Hm * (uint32_t)Wm;
    // the per-site test: the smallest shift at which neither ((d^2 >> shift) + 1) A nor (V >> shift) B can exceed 64 bits for this N
    const uint64_t pre_a = 4ull * N * (N - 2) + (uint64_t)k2q * (N - 1), pre_b = (uint64_t)k2q * (N - 1) * (N - 1);
    const uint64_t d2max = (uint64_t)(N - 1) * 65535u * ((uint64_t)(N - 1) * 65535u), vmax = (uint64_t)N * N * 65535u * 65535u / 4;
    a.pre_a = (uint32_t)pre_a; a.pre_b = (uint32_t)pre_b; a.shift = 0;
    while ((pre_a && (d2max >> a.shift) + 1 > UINT64_MAX / pre_a) || (pre_b && (vmax >> a.shift) > UINT64_MAX / pre_b)) ++a.shift;
    pack_cell_tab(a.tab, p, group, black);
    const uintptr_t fm = (uintptr_t)frames | (uintptr_t)mean;
    const int cw = (!(fm & 15u) && !((uintptr_t)kept & 7u) && Wm % 8 == 0) ? 8 : (!(fm & 3u) && !((uintptr_t)kept & 1u) && Wm % 2 == 0) ? 2 : 1;
    a.upr = (uint32_t)(Wm / cw);
    a.units = (uint32_t)Hm * a.upr;
    a.dupr = make_fastdiv(a.upr);
    if (p == 2) {
        if (cw == 8) return launch_burst<2, 8>(a, s);
        if (cw == 2) return launch_burst<2, 2>(a, s);
        return launch_burst<2, 1>(a, s);
    }
    if (cw == 8) return launch_burst<6, 8>(a, s);
    if (cw == 2) return launch_burst<6, 2>(a, s);
    return launch_burst<6, 1>(a, s);
}
