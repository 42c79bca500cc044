// nlm.hip -- non-local means over the packed planes of a variance-stabilised frame: the classical baseline beside the U-Net
// (eld_amd/classical.py).
//
//   eld_nlm_vst_f32      float32 planes [N][C][h][w] of codes / qscale -> stabilised codes through a per-plane table -> the weighted mean of
//                        the search window, weights shared by the C planes, int32 in units of 2^-frac of a stabilised code
// Integer arithmetic from the table lookup on: the output does not depend on the launch geometry, and tests/nlm_ref.py restates the contract
// of include/eld_amd.h in NumPy, bit for bit.
//
// A workgroup of 256 lanes owns a tile of NLM_T x NLM_T sites.  It stages the tile and a halo of S + P as 16-bit stabilised codes in LDS once
// (edge replication is the clamp of the source coordinate, so every later read is an in-range LDS read), then walks the (2S + 1)^2 offsets d.
// Per offset, with E_d(r) = sum over the planes of clamp(V_c(r) - V_c(r + d))^2 a function of the POSITION r alone:
//   pass 1   E_d over the tile extended by P: (T + 2P)^2 values, 2 C LDS reads each                                     -> LDS
//   pass 2   row sums of 2P + 1 of them: (T + 2P) x T values                                                          -> LDS
//   pass 3   a lane owns 4 consecutive rows of one column: the column sum of its first site, then one row in and one out per further site;
//            weight = table[min(D >> sh, 255)]; C multiply-adds into the numerators and one add into the denominator, all in registers
// so with r = 1 + 2P / T a site and offset cost about 3 C r^2 + 2P r + (2P + 6) / 4 + 4 + C vector operations (tools/nlm_time.py counts them)
// instead of the (2P + 1)^2 * 3 C of re-summing the patch: from P = 1 to P = 3 the count grows by 1.37 at C = 4, not by 49 / 9.  Two barriers
// per offset:
// pass 1 of the next offset writes what pass 2 of this one read, behind the barrier that follows pass 2.
// An offset that leaves the plane for every site of the tile is skipped by the whole workgroup (planes smaller than the search window).
//
// Widths (the argument ranges of the header make them provable): |diff| <= 1023 and codes <= 32767 are 24-bit multiplies; E <= 1023^2 * 16,
// D <= 49 E < 2^31; numerator <= 255 * 32767 * 441 < 2^32; denominator <= 255 * 441 < 2^17.  The final quotient
// (2 (num << frac) + den) / (2 den) is split as (num / den << frac) + (2 (num % den << frac) + den) / (2 den): two 32-bit divisions.
#include "common.h"

namespace {

constexpr int NLM_T = 32;                         // tile side
constexpr int NLM_THREADS = 256;
constexpr int NLM_ROWS = 4;                       // rows of one column a lane owns in pass 3: NLM_THREADS / NLM_T * NLM_ROWS == NLM_T
constexpr int NLM_MAX_S = 10, NLM_MAX_P = 3, NLM_MAX_C = 16, NLM_MAX_SH = 24, NLM_MAX_FRAC = 8;
constexpr int NLM_EW_MAX = NLM_T + 2 * NLM_MAX_P;
constexpr int NLM_EPT = (NLM_EW_MAX * NLM_EW_MAX + NLM_THREADS - 1) / NLM_THREADS;       // pass-1 values per lane, at most: 6
constexpr size_t NLM_LDS_MAX = 120 * 1024;            // >= nlm_lds_bytes(16, 10, 3) = 118800
constexpr int NLM_HPT = (NLM_EW_MAX * NLM_T + NLM_THREADS - 1) / NLM_THREADS;            // pass-2 values per lane, at most: 5

struct NlmArgs {
    const float* x;
    const uint16_t* fwd;
    int32_t* out;
    int C, h, w, S, P, sh, frac, tiles_x, tiles_y;
    float qscale;
    FastDiv div_lw, div_ew;
    uint16_t wtab[256];
};

size_t nlm_lds_bytes(int C, int S, int P) {
    const int H = S + P, LW = NLM_T + 2 * H, EW = NLM_T + 2 * P;
    size_t planes = (size_t)C * LW * LW * sizeof(uint16_t);
    planes = (planes + 3) & ~(size_t)3;
    return planes + (size_t)EW * EW * 4 + (size_t)EW * NLM_T * 4 + 256 * sizeof(uint16_t);
}

// CMAX: the planes the register file holds (C <= CMAX; the loops over planes are unrolled to CMAX and cut by the launch-uniform C)
template <int CMAX>
__global__ __launch_bounds__(NLM_THREADS) void nlm_kernel(NlmArgs a) {
    extern __shared__ __align__(16) unsigned char nlm_smem[];
    const int C = a.C, S = a.S, P = a.P, H = S + P;
    const int LW = NLM_T + 2 * H, PS = LW * LW;                    // staged row pitch and plane pitch, in codes
    const int EW = NLM_T + 2 * P;
    uint16_t* pl = reinterpret_cast<uint16_t*>(nlm_smem);
    uint32_t* E = reinterpret_cast<uint32_t*>(nlm_smem + ((((size_t)C * PS * 2) + 3) & ~(size_t)3));
    uint32_t* R = E + EW * EW;
    uint16_t* wt_s = reinterpret_cast<uint16_t*>(R + EW * NLM_T);

    const int t = threadIdx.x;
    const unsigned tiles = (unsigned)a.tiles_x * (unsigned)a.tiles_y;
    const int n = (int)(blockIdx.x / tiles), tile = (int)(blockIdx.x % tiles);
    const int ty0 = (tile / a.tiles_x) * NLM_T, tx0 = (tile % a.tiles_x) * NLM_T;
    const size_t hw = (size_t)a.h * a.w;

    // ---- stage: codes of the tile and its halo, through the forward table ---------------------------------------------------------------------
    wt_s[t] = a.wtab[t];                                            // NLM_THREADS == 256
    for (int c = 0; c < C; ++c) {
        const float* src = a.x + ((size_t)n * C + c) * hw;
        const uint16_t* tab = a.fwd + (size_t)c * 65536;
        for (int k = t; k < PS; k += NLM_THREADS) {
            const int ly = (int)fdiv_u32((uint32_t)k, a.div_lw), lx = k - ly * LW;
            const int gy = min(max(ty0 - H + ly, 0), a.h - 1), gx = min(max(tx0 - H + lx, 0), a.w - 1);
            const float f = fminf(fmaxf(rintf(src[(size_t)gy * a.w + gx] * a.qscale), 0.f), 65535.f);    // fmaxf(NaN, 0) = 0
            const uint32_t v = tab[(int)f];
            pl[c * PS + k] = (uint16_t)(v < 32767u ? v : 32767u);
        }
    }

    // ---- what does not change with the offset -------------------------------------------------------------------------------------------------
    int ebase[NLM_EPT];                                             // pass 1: staged index of position r, or -1
#pragma unroll
    for (int k = 0; k < NLM_EPT; ++k) {
        const int i = t + k * NLM_THREADS;
        const int ey = (int)fdiv_u32((uint32_t)i, a.div_ew), ex = i - ey * EW;
        ebase[k] = i < EW * EW ? (ey + S) * LW + ex + S : -1;       // r = tile origin - P + (ey, ex); staged at + H
    }
    const int px = t & (NLM_T - 1), py = (t >> 5) * NLM_ROWS;       // pass 3: column and first row of the lane
    const int gx = tx0 + px;
    const int cbase = (py + H) * LW + px + H;                       // staged index of the lane's first site
    uint32_t num[CMAX][NLM_ROWS], den[NLM_ROWS];
#pragma unroll
    for (int j = 0; j < NLM_ROWS; ++j) {
        den[j] = 0u;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) num[c][j] = 0u;
    }
    const int rows_in = min(NLM_T, a.h - ty0), cols_in = min(NLM_T, a.w - tx0);      // the tile's sites inside the plane: >= 1 each
    __syncthreads();

    for (int dy = -S; dy <= S; ++dy) {
        if (ty0 + rows_in - 1 + dy < 0 || ty0 + dy > a.h - 1) continue;             // workgroup-uniform: no site of the tile has q + d inside
        for (int dx = -S; dx <= S; ++dx) {
            if (tx0 + cols_in - 1 + dx < 0 || tx0 + dx > a.w - 1) continue;
            const int doff = dy * LW + dx;
            // pass 1
#pragma unroll
            for (int k = 0; k < NLM_EPT; ++k) {
                if (ebase[k] >= 0) {
                    uint32_t e = 0u;
#pragma unroll
                    for (int c = 0; c < CMAX; ++c) {
                        if (c < C) {
                            const int p0 = c * PS + ebase[k];
                            const int df = min(max((int)pl[p0] - (int)pl[p0 + doff], -1023), 1023);
                            e += (uint32_t)__mul24(df, df);
                        }
                    }
                    E[t + k * NLM_THREADS] = e;
                }
            }
            __syncthreads();
            // pass 2
#pragma unroll
            for (int k = 0; k < NLM_HPT; ++k) {
                const int i = t + k * NLM_THREADS;
                if (i < EW * NLM_T) {
                    const int ey = i >> 5, ex = i & (NLM_T - 1);
                    const uint32_t* row = E + ey * EW + ex;
                    uint32_t s = row[0];
                    for (int j = 1; j <= 2 * P; ++j) s += row[j];
                    R[i] = s;
                }
            }
            __syncthreads();
            // pass 3
            const uint32_t* col = R + py * NLM_T + px;
            uint32_t D = 0u;
            for (int j = 0; j <= 2 * P; ++j) D += col[j * NLM_T];
            const bool xin = gx + dx >= 0 && gx + dx < a.w;
#pragma unroll
            for (int j = 0; j < NLM_ROWS; ++j) {
                const int gy = ty0 + py + j;
                const bool ok = xin && gy + dy >= 0 && gy + dy < a.h;                // a site outside the plane is never written: any weight
                const uint32_t wt = ok ? (uint32_t)wt_s[min(D >> a.sh, 255u)] : 0u;
                den[j] += wt;
                const int p0 = cbase + j * LW + doff;
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C) num[c][j] += __umul24(wt, (uint32_t)pl[c * PS + p0]);
                if (j + 1 < NLM_ROWS) D += col[(j + 2 * P + 1) * NLM_T] - col[j * NLM_T];
            }
        }
    }

    // ---- the quotient ---------------------------------------------------------------------------------------------------------------------------
    if (gx < a.w) {
#pragma unroll
        for (int j = 0; j < NLM_ROWS; ++j) {
            const int gy = ty0 + py + j;
            if (gy < a.h) {
                const uint32_t d = den[j];                          // >= wtab[0] >= 1: d = 0 always counts
#pragma unroll
                for (int c = 0; c < CMAX; ++c) {
                    if (c < C) {
                        const uint32_t q = num[c][j] / d, r = num[c][j] - q * d;
                        const uint32_t v = (q << a.frac) + (2u * (r << a.frac) + d) / (2u * d);
                        a.out[((size_t)n * C + c) * hw + (size_t)gy * a.w + gx] = (int32_t)v;
                    }
                }
            }
        }
    }
}

template <int CMAX>
int nlm_launch(const NlmArgs& a, unsigned blocks, size_t lds, hipStream_t st) {
    static EldAttrOnce once;
    const int rc = once.ensure(nlm_kernel<CMAX>, NLM_LDS_MAX);
    if (rc) return rc;
    ELD_LAUNCH(nlm_kernel<CMAX>, dim3(blocks), dim3(NLM_THREADS), lds, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int eld_nlm_vst_f32(const float* x, int N, int C, int h, int w, float qscale, const uint16_t* fwd, int S, int P, int sh,
                               const uint16_t* wtab, int frac, int32_t* out, void* stream) {
    if (N < 1 || C < 1 || C > NLM_MAX_C || h < 1 || w < 1 || S < 0 || S > NLM_MAX_S || P < 0 || P > NLM_MAX_P || sh < 0 || sh > NLM_MAX_SH ||
        frac < 0 || frac > NLM_MAX_FRAC || !wtab || !x || !fwd || !out)
        return ELD_EINVAL;
    if (((uintptr_t)x & 3u) || ((uintptr_t)fwd & 1u) || ((uintptr_t)out & 3u)) return ELD_EINVAL;
    for (int k = 0; k < 256; ++k)
        if (wtab[k] > 255) return ELD_EINVAL;
    if (wtab[0] < 1) return ELD_EINVAL;
    NlmArgs a;
    a.x = x; a.fwd = fwd; a.out = out;
    a.C = C; a.h = h; a.w = w; a.S = S; a.P = P; a.sh = sh; a.frac = frac; a.qscale = qscale;
    a.tiles_x = (w + NLM_T - 1) / NLM_T; a.tiles_y = (h + NLM_T - 1) / NLM_T;
    const long long blocks = (long long)a.tiles_x * a.tiles_y * N;
    if (blocks > 0x7FFFFFFFll) return ELD_EINVAL;
    a.div_lw = make_fastdiv((uint32_t)(NLM_T + 2 * (S + P)));
    a.div_ew = make_fastdiv((uint32_t)(NLM_T + 2 * P));
    for (int k = 0; k < 256; ++k) a.wtab[k] = wtab[k];
    const size_t lds = nlm_lds_bytes(C, S, P);                      // at most 118.8 KB of the 160 KB
    const hipStream_t st = as_stream(stream);
    if (C <= 4) return nlm_launch<4>(a, (unsigned)blocks, lds, st);
    if (C <= 9) return nlm_launch<9>(a, (unsigned)blocks, lds, st);
    return nlm_launch<16>(a, (unsigned)blocks, lds, st);
}
