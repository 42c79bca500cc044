// calib.hip -- noise-parameter calibration from bias frames and flat-field pairs (eld_amd/calibrate.py, DESIGN.md "Calibration").
// One set of pixel passes serves every CFA: they return per-cell sums of a mosaic of period 2 (Bayer) or 6 (X-Trans) and leave the
// colours to the host.  The Bayer entry points (eld_calib_bias_stats, _bias_residual, _flat_stats) are the period-2 case with the cells
// stored in the channel order of a 2x2 raw_pattern.
//
// Four passes; everything else is derived on the host in float64 from their outputs:
//   bias statistics   uint16 mosaics -> per row: sums over each column class; per frame and cell: sum u, sum u^2 (uint64, exact)
//   bias residual     t = float32(((u - black_k) - cb_k) - rho_y), float64 arithmetic, one rounding (NumPy's, bit for bit)
//   flat statistics   uint16 pairs (a, b) -> per pair and cell: sum(a+b), sum(a-b), sum((a-b)^2), saturated pixels (int64, exact)
//   PPCC              sorted residuals -> per Tukey-lambda shape: sum t*M, sum M^2 (and sum t, sum t^2), float64, fixed order
// Cell of mosaic pixel (y, x): (y % p, x % p); its Bayer channel is raw_pattern[y&1][x&1] (R, G1, B, G2 = 0..3), as eld_pack_raw_bayer_u16.
// No atomics anywhere: every sum is reduced in an order fixed by the shape alone, so two launches give identical bits.
#include "mosaic_dev.h"

namespace {

constexpr int CB_THREADS = 256;
constexpr int CB_WAVES = CB_THREADS / ELD_WAVE;

// Where cell k = r*p + c of the pattern lives in the caller's per-cell arrays (the sums written, the colour bias read): slot s[k].  The
// cell entry points store cells in order (identity); the Bayer ones in channel order, s = the 2x2 raw_pattern.
struct CellSlots {
    unsigned char s[36];
};

// Sum NV uint64 values over the block (256 threads); the block's totals land in tot[] (LDS, valid after the call).  Integer sums:
// exact, order-independent.
template <int NV>
__device__ __forceinline__ void block_sum_u64(uint64_t (&v)[NV], uint64_t* red /* LDS [CB_WAVES][NV] */, uint64_t* tot /* LDS [NV] */) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) red[wv * NV + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < NV) {
        uint64_t s = 0;
        for (int w = 0; w < CB_WAVES; ++w) s += red[w * NV + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
}

// ---- PPCC over a Tukey-lambda grid -----------------------------------------------------------------------------------------
// Sorted t_0 <= ... <= t_{n-1}; Filliben's medians m_i (i = 1..n) with m_{n+1-i} = 1 - m_i, so pair i (0-based, i < n/2) with
// j = n-1-i: M(m_j) = -M(m_i), sum M = 0 exactly, and the pair contributes M_j (t_j - t_i) to sum t*M and 2 M_j^2 to sum M^2.
// With a = log2 m_i, b = log2(1 - m_i), h = (a+b)/2, g = (b-a) ln2/2 >= 0:
//   M_j = (2^(lam b) - 2^(lam a)) / lam = 2^(lam h + 1) g shc(lam g),  shc(x) = sinh(x)/x  (= 2g at lam = 0: the logistic quantile)
// shc is even and >= 1: below |x| = 1 a Taylor polynomial (no cancellation at small |lam|); at |x| >= 1 the first form, whose two
// powers then differ by more than a factor e^2.  Each lane evaluates only its own form.
constexpr int PP_THREADS = 256;
constexpr int PP_PAIRS = 8;                      // pairs per thread per block: a block covers PP_THREADS * PP_PAIRS pairs
constexpr int PP_BLOCK_PAIRS = PP_THREADS * PP_PAIRS;
constexpr int PP_LG = 16;                        // lambdas per block (grid.y covers the grid in groups of PP_LG)

__host__ __device__ inline size_t pp_blocks(size_t n) { return (n / 2 + PP_BLOCK_PAIRS - 1) / PP_BLOCK_PAIRS; }

// partial layout: [F][nb][L][2] (sum t*M, sum M^2) then [F][nb][2] (sum t, sum t^2)
__global__ __launch_bounds__(PP_THREADS) void ppcc_partial_kernel(const float* __restrict__ ts, size_t n, const float* __restrict__ lam, int L,
                                                                  double* __restrict__ part, double* __restrict__ tpart) {
    __shared__ double red[PP_THREADS / ELD_WAVE][2 * PP_LG];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t nb = gridDim.x, blk = blockIdx.x, np = n / 2;
    const int l0 = blockIdx.y * PP_LG, f = blockIdx.z;
    const float* t = ts + (size_t)f * n;
    const double rdn = 1.0 / ((double)n + 0.365);
    const double mn = exp2(-1.0 / (double)n), m1 = 1.0 - mn;  // m_n = 0.5^(1/n), m_1 = 1 - m_n

    float lm[PP_LG];
#pragma unroll
    for (int q = 0; q < PP_LG; ++q) lm[q] = (l0 + q < L) ? lam[l0 + q] : 0.0f;
    float il[PP_LG];                                           // 1/lam (used only where |lam g| >= 1, so never at lam = 0)
#pragma unroll
    for (int q = 0; q < PP_LG; ++q) il[q] = lm[q] != 0.0f ? 1.0f / lm[q] : 0.0f;
    double stm[PP_LG], smm[PP_LG];
#pragma unroll
    for (int q = 0; q < PP_LG; ++q) { stm[q] = 0.0; smm[q] = 0.0; }
    double st = 0.0, stt = 0.0;

    for (int k = 0; k < PP_PAIRS; ++k) {
        const size_t i = blk * PP_BLOCK_PAIRS + (size_t)k * PP_THREADS + threadIdx.x;
        if (i >= np) break;
        // m_i and 1 - m_i, each without cancellation (1-based index i+1); rounded to float32 below, so 1/(n + 0.365) once suffices
        const double mi = i == 0 ? m1 : ((double)(i + 1) - 0.3175) * rdn;
        const double mj = i == 0 ? mn : ((double)n + 0.6825 - (double)(i + 1)) * rdn;
        const float a = __builtin_amdgcn_logf((float)mi), b = __builtin_amdgcn_logf((float)mj);
        const float h = 0.5f * (a + b), g = (b - a) * 0.34657359027997264f;
        const float ti = t[i], tj = t[n - 1 - i];
        const double dt = (double)tj - (double)ti;
        if (blockIdx.y == 0) {
            st += (double)ti + (double)tj;
            stt += (double)ti * (double)ti + (double)tj * (double)tj;
        }
#pragma unroll
        for (int q = 0; q < PP_LG; ++q) {
            const float x = lm[q] * g;
            float M;
            if (fabsf(x) < 1.0f) {                             // one form per lane: a wave of adjacent pairs nearly always takes one
                const float x2 = x * x;
                float poly = __builtin_fmaf(x2, 1.0f / 39916800.0f, 1.0f / 362880.0f);
                poly = __builtin_fmaf(poly, x2, 1.0f / 5040.0f);
                poly = __builtin_fmaf(poly, x2, 1.0f / 120.0f);
                poly = __builtin_fmaf(poly, x2, 1.0f / 6.0f);
                poly = __builtin_fmaf(poly, x2, 1.0f);
                M = __builtin_amdgcn_exp2f(__builtin_fmaf(lm[q], h, 1.0f)) * g * poly;
            } else {                                           // |lam (b-a)| >= 2/ln2: the two powers differ by > 7x, no cancellation
                M = (__builtin_amdgcn_exp2f(lm[q] * b) - __builtin_amdgcn_exp2f(lm[q] * a)) * il[q];
            }
            const double Md = (double)M;
            stm[q] = __builtin_fma(Md, dt, stm[q]);
            smm[q] = __builtin_fma(Md, Md, smm[q]);
        }
    }
    // block reduction in a fixed order: wave butterflies, then waves 0..3 in order
#pragma unroll
    for (int q = 0; q < PP_LG; ++q) {
        const double s1 = wave_sum(stm[q]), s2 = wave_sum(smm[q]);
        if (lane == 0) { red[wv][2 * q] = s1; red[wv][2 * q + 1] = 2.0 * s2; }
    }
    const double a1 = wave_sum(st), a2 = wave_sum(stt);
    __syncthreads();
    if (threadIdx.x < 2 * PP_LG) {
        double s = 0.0;
        for (int w = 0; w < PP_THREADS / ELD_WAVE; ++w) s += red[w][threadIdx.x];
        const int l = l0 + threadIdx.x / 2;
        if (l < L) part[(((size_t)f * nb + blk) * L + l) * 2 + (threadIdx.x & 1)] = s;
    }
    __syncthreads();
    if (blockIdx.y == 0) {
        if (lane == 0) { red[wv][0] = a1; red[wv][1] = a2; }
        __syncthreads();
        if (threadIdx.x < 2) {
            double s = 0.0;
            for (int w = 0; w < PP_THREADS / ELD_WAVE; ++w) s += red[w][threadIdx.x];
            tpart[((size_t)f * nb + blk) * 2 + threadIdx.x] = s;
        }
    }
}

// one block per (frame, lambda) and one per frame for the t sums: thread k sums blocks k, k+256, ... in order, then the fixed
// block reduction
__global__ __launch_bounds__(256) void ppcc_final_kernel(const float* __restrict__ ts, size_t n, int L, size_t nb,
                                                         const double* __restrict__ part, const double* __restrict__ tpart,
                                                         double* __restrict__ sums, double* __restrict__ tsums) {
    __shared__ double red[256 / ELD_WAVE][2];
    const int f = blockIdx.y, l = blockIdx.x;                  // l == L: the t sums
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double s1 = 0.0, s2 = 0.0;
    for (size_t b = threadIdx.x; b < nb; b += 256) {
        const double* p = l < L ? part + (((size_t)f * nb + b) * L + l) * 2 : tpart + ((size_t)f * nb + b) * 2;
        s1 += p[0];
        s2 += p[1];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) { red[wv][0] = s1; red[wv][1] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        s1 = 0.0; s2 = 0.0;
        for (int w = 0; w < 256 / ELD_WAVE; ++w) { s1 += red[w][0]; s2 += red[w][1]; }
        if (l < L) {
            sums[((size_t)f * L + l) * 2] = s1;
            sums[((size_t)f * L + l) * 2 + 1] = s2;
        } else {
            if (n & 1) {                                       // the median element: M = 0, it enters the t sums only
                const double tm = ts[(size_t)f * n + n / 2];
                s1 += tm;
                s2 += tm * tm;
            }
            tsums[(size_t)f * 2] = s1;
            tsums[(size_t)f * 2 + 1] = s2;
        }
    }
}

// ---- cell statistics of a pattern of period PP = 2 * P2 (2: Bayer, 6: X-Trans) ----------------------------------------------
// Word k of a row holds columns 2k, 2k+1: column classes 2 (k % P2) and 2 (k % P2) + 1.  A lane takes G consecutive words per step (G a
// multiple of P2, starting at a multiple of G), so word j of the step has class j % P2 at compile time; the last nw % G words of the row
// (fewer than G, starting at a multiple of P2) go to lanes 0.. one word each.  NR rows of one alignment (a bias row; the a and b rows of
// a flat pair) are walked together: fn(q, w, take) adds the rows' words w[0..NR) at one word index to class q where `take`.
// VEC: 16-byte loads (4 words) when Wm % 8 == 0 and the base is 16-byte aligned (rows and frames then start 16-byte aligned too).
// Accumulators v[(q*2 + px)*NS + s]: word class q, column parity px (column class 2q + px), statistic s.
template <int P2, bool VEC, int NR>
struct CellWalk {
    static constexpr int G = VEC ? 4 * P2 : P2;
    template <typename Fn>
    __device__ __forceinline__ static void run(const uint32_t* const (&row)[NR], int nw, Fn fn) {
        const int ng = nw / G;
        for (int kk = threadIdx.x; kk < ng; kk += CB_THREADS) {
            uint32_t w[G][NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                if (VEC) {
#pragma unroll
                    for (int i = 0; i < G / 4; ++i) {
                        const uint4 q = reinterpret_cast<const uint4*>(row[r])[kk * (G / 4) + i];
                        w[4 * i][r] = q.x; w[4 * i + 1][r] = q.y; w[4 * i + 2][r] = q.z; w[4 * i + 3][r] = q.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < G; ++j) w[j][r] = row[r][kk * G + j];
                }
            }
#pragma unroll
            for (int j = 0; j < G; ++j) fn(j % P2, w[j], true);
        }
        const int tail = nw - ng * G;
        if ((int)threadIdx.x < tail) {
            uint32_t wt[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) wt[r] = row[r][ng * G + threadIdx.x];
#pragma unroll
            for (int q = 0; q < P2; ++q) fn(q, wt, (int)threadIdx.x % P2 == q);   // every class, masked: no indexed registers
        }
    }
};

// bias pass 1: one block per (row, frame).  rows[(f*Hm + y)*PP + c] = sum of u over the columns of class c;
// part[((f*Hm + y)*PP + c)*2 + {0, 1}] = sum u, sum u^2 there.
template <int P2, bool VEC>
__global__ __launch_bounds__(CB_THREADS) void cell_row_kernel(const uint16_t* __restrict__ u, int Hm, int Wm, uint64_t* __restrict__ rows,
                                                               uint64_t* __restrict__ part) {
    constexpr int PP = 2 * P2, NV = PP * 2;
    __shared__ uint64_t red[CB_WAVES * NV], tot[NV];
    const int y = blockIdx.x, f = blockIdx.y;
    const size_t ro = (size_t)f * Hm + y;
    const uint32_t* const row[1] = {reinterpret_cast<const uint32_t*>(u + ro * Wm)};
    uint64_t v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0;
    CellWalk<P2, VEC, 1>::run(row, Wm / 2, [&](int q, const uint32_t (&w)[1], bool take) __attribute__((always_inline)) {
        const uint32_t e = take ? w[0] & 0xFFFFu : 0u, o = take ? w[0] >> 16 : 0u;
        v[(2 * q) * 2] += e; v[(2 * q + 1) * 2] += o;
        v[(2 * q) * 2 + 1] += (uint64_t)(e * e); v[(2 * q + 1) * 2 + 1] += (uint64_t)(o * o);   // < 2^32: exact in uint32
    });
    block_sum_u64<NV>(v, red, tot);
    if (threadIdx.x < PP) rows[ro * PP + threadIdx.x] = tot[threadIdx.x * 2];
    if (threadIdx.x < NV) part[ro * NV + threadIdx.x] = tot[threadIdx.x];
}

// flat pass 1: one block per (row, pair).  part[((p*Hm + y)*PP + c)*4 + s] = sum(a+b), sum(a-b), sum((a-b)^2), #(a or b >= white)
template <int P2, bool VEC>
__global__ __launch_bounds__(CB_THREADS) void cell_flat_row_kernel(const uint16_t* __restrict__ ab, int Hm, int Wm, uint32_t white,
                                                                    uint64_t* __restrict__ part) {
    constexpr int PP = 2 * P2, NV = PP * 4;
    __shared__ uint64_t red[CB_WAVES * NV], tot[NV];
    const int y = blockIdx.x, pr = blockIdx.y;
    const size_t frame = (size_t)Hm * Wm;
    const uint16_t* a = ab + (size_t)pr * 2 * frame + (size_t)y * Wm;
    const uint32_t* const row[2] = {reinterpret_cast<const uint32_t*>(a), reinterpret_cast<const uint32_t*>(a + frame)};
    uint64_t v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0;
    CellWalk<P2, VEC, 2>::run(row, Wm / 2, [&](int q, const uint32_t (&w)[2], bool take) __attribute__((always_inline)) {
#pragma unroll
        for (int px = 0; px < 2; ++px) {
            const uint32_t x = take ? (w[0] >> (16 * px)) & 0xFFFFu : 0u, z = take ? (w[1] >> (16 * px)) & 0xFFFFu : 0u;
            const int32_t d = (int32_t)x - (int32_t)z;
            uint64_t* vv = v + (2 * q + px) * 4;
            vv[0] += x + z;
            vv[1] += (uint64_t)(int64_t)d;
            vv[2] += (uint64_t)((uint32_t)d * (uint32_t)d);          // d^2 < 2^32: exact modulo 2^32
            vv[3] += (take && (x >= white || z >= white)) ? 1u : 0u;
        }
    });
    block_sum_u64<NV>(v, red, tot);
    if (threadIdx.x < NV) part[((size_t)pr * Hm + y) * NV + threadIdx.x] = tot[threadIdx.x];
}

// pass 2 (bias and flat): one block per frame / pair folds the per-row partials part[F][Hm][PP][NS] into out[F][PP*PP][NS] (row class
// y % PP; cell (rc, c) goes to slot.s[rc*PP + c]).  Lanes take rows y = tid, tid + RS, ... with RS a multiple of PP, so a lane's rows
// share one class.  The upper half of the lanes is then folded onto the lower while both halves hold the same classes (RS = 256 -> 2 at
// PP = 2, 252 -> 126 at PP = 6), and one lane per output sums what is left of its class.
template <int PP, int NS>
__global__ __launch_bounds__(CB_THREADS) void cell_reduce_kernel(const uint64_t* __restrict__ part, int Hm, CellSlots slot, uint64_t* __restrict__ out) {
    constexpr int RS = CB_THREADS - CB_THREADS % PP, NV = PP * NS;
    static_assert(PP * NV <= CB_THREADS, "one lane per output");
    __shared__ uint64_t red[RS * NV];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int rc = tid / NV, k = tid - rc * NV;                      // output tid = rc * NV + (c * NS + s), for tid < PP * NV
    const int cell = tid < PP * NV ? slot.s[rc * PP + k / NS] : 0;
    const uint64_t* p = part + (size_t)f * Hm * NV;
    if (tid < RS) {
        uint64_t v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = 0;
        for (int y = tid; y < Hm; y += RS)
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] += p[(size_t)y * NV + i];
#pragma unroll
        for (int i = 0; i < NV; ++i) red[tid * NV + i] = v[i];
    }
    __syncthreads();
    int h = RS;
    while (h % (2 * PP) == 0) {
        h /= 2;
        if (tid < h)
#pragma unroll
            for (int i = 0; i < NV; ++i) red[tid * NV + i] += red[(tid + h) * NV + i];
        __syncthreads();
    }
    if (tid < PP * NV) {
        uint64_t s = 0;
        for (int l = rc; l < h; l += PP) s += red[l * NV + k];
        out[((size_t)f * PP * PP + cell) * NS + k % NS] = s;
    }
}

// residual: t = float32(((u - black[k]) - cb[f][slot.s[k]]) - rho[f][y]), k = (y % PP) * PP + x % PP, in float64.  One block per (row, frame).
struct CellBlack {
    double b[36];
};

template <int P2>
__global__ __launch_bounds__(CB_THREADS) void cell_residual_kernel(const uint16_t* __restrict__ u, int Hm, int Wm, CellBlack blk, CellSlots slot,
                                                                   const double* __restrict__ cb, const double* __restrict__ rho,
                                                                   float* __restrict__ t) {
    constexpr int PP = 2 * P2;
    __shared__ double s_b[PP], s_cb[PP];
    const int y = blockIdx.x, f = blockIdx.y;
    const size_t ro = (size_t)f * Hm + y;
    const int rc = y % PP;
    if (threadIdx.x < PP) {
        s_b[threadIdx.x] = blk.b[rc * PP + threadIdx.x];
        s_cb[threadIdx.x] = cb[(size_t)f * PP * PP + slot.s[rc * PP + threadIdx.x]];
    }
    __syncthreads();
    const uint32_t* row = reinterpret_cast<const uint32_t*>(u + ro * Wm);
    float2* out = reinterpret_cast<float2*>(t + ro * Wm);
    const double r = rho[ro];
    for (int k = threadIdx.x; k < Wm / 2; k += CB_THREADS) {
        const uint32_t w = row[k];
        const int c0 = 2 * (k % P2);
        const double e = (((double)(w & 0xFFFFu) - s_b[c0]) - s_cb[c0]) - r;
        const double o = (((double)(w >> 16) - s_b[c0 + 1]) - s_cb[c0 + 1]) - r;
        out[k] = make_float2((float)e, (float)o);
    }
}

// a 2x2 raw_pattern (a permutation of the channels 0..3) as the slots of the period-2 cells
int parse_pattern(const int* raw_pattern, CellSlots& p) {
    if (!raw_pattern || !bayer_permutation(raw_pattern)) return ELD_EINVAL;
    for (int i = 0; i < 4; ++i) p.s[i] = (unsigned char)raw_pattern[i];
    return 0;
}

CellSlots cells_in_order() {
    CellSlots p;
    for (int k = 0; k < 36; ++k) p.s[k] = (unsigned char)k;
    return p;
}

bool mosaic_ok(int F, int Hm, int Wm) { return F >= 0 && Hm >= 0 && Wm >= 0 && Hm % 2 == 0 && Wm % 2 == 0 && F <= 65535; }
bool cell_ok(int F, int Hm, int Wm, int p) { return (p == 2 || p == 6) && F >= 0 && Hm >= 0 && Wm >= 0 && Wm % 2 == 0 && F <= 65535; }
bool vec_ok(const void* p, int Wm) { return Wm % 8 == 0 && ((uintptr_t)p & 15u) == 0; }
bool word_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0; }   // rows are read as 32-bit words (two pixels)

// The launches behind the entry points (arguments checked by the caller, nothing empty): the statistics' two passes and the residual.
template <int P2>
int launch_cell_stats(const uint16_t* u, int F, int Hm, int Wm, const CellSlots& slot, uint64_t* cell_sums, uint64_t* row_sums, uint64_t* part,
                      hipStream_t s) {
    const dim3 g(Hm, F), b(CB_THREADS);
    if (vec_ok(u, Wm)) ELD_LAUNCH((cell_row_kernel<P2, true>), g, b, 0, s, u, Hm, Wm, row_sums, part);
    else ELD_LAUNCH((cell_row_kernel<P2, false>), g, b, 0, s, u, Hm, Wm, row_sums, part);
    ELD_LAUNCH_CHECK();
    ELD_LAUNCH((cell_reduce_kernel<2 * P2, 2>), dim3(F), b, 0, s, part, Hm, slot, cell_sums);
    ELD_LAUNCH_CHECK();
    return 0;
}

template <int P2>
int launch_cell_flat_stats(const uint16_t* ab, int P, int Hm, int Wm, const CellSlots& slot, uint32_t white, uint64_t* out, uint64_t* part,
                           hipStream_t s) {
    const dim3 g(Hm, P), b(CB_THREADS);
    if (vec_ok(ab, Wm)) ELD_LAUNCH((cell_flat_row_kernel<P2, true>), g, b, 0, s, ab, Hm, Wm, white, part);
    else ELD_LAUNCH((cell_flat_row_kernel<P2, false>), g, b, 0, s, ab, Hm, Wm, white, part);
    ELD_LAUNCH_CHECK();
    ELD_LAUNCH((cell_reduce_kernel<2 * P2, 4>), dim3(P), b, 0, s, part, Hm, slot, out);
    ELD_LAUNCH_CHECK();
    return 0;
}

template <int P2>
int launch_cell_residual(const uint16_t* u, int F, int Hm, int Wm, const CellBlack& blk, const CellSlots& slot, const double* cb,
                         const double* rho, float* t, hipStream_t s) {
    ELD_LAUNCH(cell_residual_kernel<P2>, dim3(Hm, F), dim3(CB_THREADS), 0, s, u, Hm, Wm, blk, slot, cb, rho, t);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" size_t eld_calib_bias_stats_workspace_bytes(int F, int Hm) {
    return F <= 0 || Hm <= 0 ? 0 : (size_t)F * Hm * 4 * sizeof(uint64_t);
}

extern "C" int eld_calib_bias_stats(const uint16_t* u, int F, int Hm, int Wm, const int* raw_pattern, uint64_t* chan_sums, uint64_t* row_sums,
                                    void* ws, size_t ws_bytes, void* stream) {
    CellSlots pat = {};
    if (!mosaic_ok(F, Hm, Wm) || parse_pattern(raw_pattern, pat)) return ELD_EINVAL;
    if (F == 0 || Hm == 0 || Wm == 0) return 0;
    if (!u || !chan_sums || !row_sums || !ws || !word_aligned(u)) return ELD_EINVAL;
    if (ws_bytes < eld_calib_bias_stats_workspace_bytes(F, Hm)) return ELD_EWS;
    return launch_cell_stats<1>(u, F, Hm, Wm, pat, chan_sums, row_sums, static_cast<uint64_t*>(ws), as_stream(stream));
}

extern "C" int eld_calib_bias_residual(const uint16_t* u, int F, int Hm, int Wm, const int* raw_pattern, const double* black_level,
                                       const double* color_bias, const double* row_offset, float* t, void* stream) {
    CellSlots pat = {};
    if (!mosaic_ok(F, Hm, Wm) || parse_pattern(raw_pattern, pat) || !black_level) return ELD_EINVAL;
    if (F == 0 || Hm == 0 || Wm == 0) return 0;
    if (!u || !color_bias || !row_offset || !t || !word_aligned(u) || ((uintptr_t)t & 7u)) return ELD_EINVAL;
    CellBlack blk = {};
    for (int k = 0; k < 4; ++k) blk.b[k] = black_level[pat.s[k]];
    return launch_cell_residual<1>(u, F, Hm, Wm, blk, pat, color_bias, row_offset, t, as_stream(stream));
}

extern "C" size_t eld_calib_flat_stats_workspace_bytes(int P, int Hm) {
    return P <= 0 || Hm <= 0 ? 0 : (size_t)P * Hm * 8 * sizeof(uint64_t);
}

extern "C" int eld_calib_flat_stats(const uint16_t* ab, int P, int Hm, int Wm, const int* raw_pattern, int white_level, int64_t* out,
                                    void* ws, size_t ws_bytes, void* stream) {
    CellSlots pat = {};
    if (!mosaic_ok(P, Hm, Wm) || parse_pattern(raw_pattern, pat) || white_level < 0) return ELD_EINVAL;
    if (P == 0 || Hm == 0 || Wm == 0) return 0;
    if (!ab || !out || !ws || !word_aligned(ab)) return ELD_EINVAL;
    if (ws_bytes < eld_calib_flat_stats_workspace_bytes(P, Hm)) return ELD_EWS;
    return launch_cell_flat_stats<1>(ab, P, Hm, Wm, pat, (uint32_t)white_level, reinterpret_cast<uint64_t*>(out), static_cast<uint64_t*>(ws),
                                     as_stream(stream));
}

extern "C" size_t eld_calib_ppcc_workspace_bytes(int F, size_t n, int L) {
    if (F <= 0 || n < 3 || L <= 0) return 0;
    const size_t nb = pp_blocks(n);
    return (size_t)F * nb * ((size_t)L + 1) * 2 * sizeof(double);
}

extern "C" int eld_calib_ppcc(const float* t_sorted, int F, size_t n, const float* lambdas, int L, double* sums, double* tsums,
                              void* ws, size_t ws_bytes, void* stream) {
    if (F < 0 || L < 0 || F > 65535 || (n < 3 && F > 0) || n > ((size_t)1 << 40)) return ELD_EINVAL;
    if (F == 0 || L == 0) return 0;
    if (!t_sorted || !lambdas || !sums || !tsums || !ws) return ELD_EINVAL;
    if (ws_bytes < eld_calib_ppcc_workspace_bytes(F, n, L)) return ELD_EWS;
    const size_t nb = pp_blocks(n);
    if (nb > 0x7FFFFFFFu) return ELD_EINVAL;
    double* part = static_cast<double*>(ws);
    double* tpart = part + (size_t)F * nb * L * 2;
    hipStream_t s = as_stream(stream);
    ELD_LAUNCH(ppcc_partial_kernel, dim3((unsigned)nb, (L + PP_LG - 1) / PP_LG, F), dim3(PP_THREADS), 0, s, t_sorted, n, lambdas, L, part, tpart);
    ELD_LAUNCH_CHECK();
    ELD_LAUNCH(ppcc_final_kernel, dim3(L + 1, F), dim3(256), 0, s, t_sorted, n, L, nb, part, tpart, sums, tsums);
    ELD_LAUNCH_CHECK();
    return 0;
}

// ---- cell statistics (any CFA of period 2 or 6) ----------------------------------------------------------------------------------
extern "C" size_t eld_calib_cell_stats_workspace_bytes(int F, int Hm, int p) {
    return F <= 0 || Hm <= 0 || (p != 2 && p != 6) ? 0 : (size_t)F * Hm * p * 2 * sizeof(uint64_t);
}

extern "C" int eld_calib_cell_stats(const uint16_t* u, int F, int Hm, int Wm, int p, uint64_t* cell_sums, uint64_t* row_sums,
                                    void* ws, size_t ws_bytes, void* stream) {
    if (!cell_ok(F, Hm, Wm, p)) return ELD_EINVAL;
    if (F == 0 || Hm == 0 || Wm == 0) return 0;
    if (!u || !cell_sums || !row_sums || !ws || !word_aligned(u)) return ELD_EINVAL;
    if (ws_bytes < eld_calib_cell_stats_workspace_bytes(F, Hm, p)) return ELD_EWS;
    uint64_t* part = static_cast<uint64_t*>(ws);
    return p == 2 ? launch_cell_stats<1>(u, F, Hm, Wm, cells_in_order(), cell_sums, row_sums, part, as_stream(stream))
                  : launch_cell_stats<3>(u, F, Hm, Wm, cells_in_order(), cell_sums, row_sums, part, as_stream(stream));
}

extern "C" int eld_calib_cell_residual(const uint16_t* u, int F, int Hm, int Wm, int p, const double* black, const double* cell_bias,
                                       const double* row_offset, float* t, void* stream) {
    if (!cell_ok(F, Hm, Wm, p) || !black) return ELD_EINVAL;
    if (F == 0 || Hm == 0 || Wm == 0) return 0;
    if (!u || !cell_bias || !row_offset || !t || !word_aligned(u) || ((uintptr_t)t & 7u)) return ELD_EINVAL;
    CellBlack blk;
    for (int k = 0; k < 36; ++k) blk.b[k] = k < p * p ? black[k] : 0.0;
    return p == 2 ? launch_cell_residual<1>(u, F, Hm, Wm, blk, cells_in_order(), cell_bias, row_offset, t, as_stream(stream))
                  : launch_cell_residual<3>(u, F, Hm, Wm, blk, cells_in_order(), cell_bias, row_offset, t, as_stream(stream));
}

extern "C" size_t eld_calib_cell_flat_stats_workspace_bytes(int P, int Hm, int p) {
    return P <= 0 || Hm <= 0 || (p != 2 && p != 6) ? 0 : (size_t)P * Hm * p * 4 * sizeof(uint64_t);
}

extern "C" int eld_calib_cell_flat_stats(const uint16_t* ab, int P, int Hm, int Wm, int p, int white_level, int64_t* out,
                                         void* ws, size_t ws_bytes, void* stream) {
    if (!cell_ok(P, Hm, Wm, p) || white_level < 0) return ELD_EINVAL;
    if (P == 0 || Hm == 0 || Wm == 0) return 0;
    if (!ab || !out || !ws || !word_aligned(ab)) return ELD_EINVAL;
    if (ws_bytes < eld_calib_cell_flat_stats_workspace_bytes(P, Hm, p)) return ELD_EWS;
    uint64_t* part = static_cast<uint64_t*>(ws);
    uint64_t* o = reinterpret_cast<uint64_t*>(out);
    return p == 2 ? launch_cell_flat_stats<1>(ab, P, Hm, Wm, cells_in_order(), (uint32_t)white_level, o, part, as_stream(stream))
                  : launch_cell_flat_stats<3>(ab, P, Hm, Wm, cells_in_order(), (uint32_t)white_level, o, part, as_stream(stream));
}
