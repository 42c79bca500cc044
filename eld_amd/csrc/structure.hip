// structure.hip -- exact integer sums for the spatial structure of noise (eld_amd/structure.py).
//
//   eld_struct_sums_u16    uint16 mosaics [F,Hm,Wm] -> row[F][Hm][p][2] (n, sum d), col[F][Wm][p][2] (n, sum d), cell[F][p*p][3] (n, sum d, sum d^2)
//   eld_struct_cross_u16   the same stack and Q frame pairs -> cross[Q][p*p] = sum d_a d_b
// d = int(u) - centre[cell (y % p, x % p)], |d| <= 65535; a site flagged in the defect bitmap contributes nothing.  Integer adds only: any
// arrival order gives the same bits.  sum d^2 <= 65535^2 (Hm Wm) < 2^32 * 2^31 = 2^63, so every output fits int64.
//
// One pass over each frame.  A workgroup (256 threads, 4 waves) owns a band of bh rows by a span of 64 * NPX columns; a lane holds NPX
// consecutive columns (8: one 16-byte load per row; 2: one 32-bit word).  The four waves take the band's rows in turns of U rows (U = a
// multiple of p, bands start at a multiple of U), so the row phase y % p is the unrolled loop index: a compile-time register index.
//   * column partials (n, sum d) per row phase and column stay in the lane's registers over the band: int32, |sum d| <= (bh / p) * 65535 with
//     bh <= S_MAX_BH = 8192, so below 2^28.  At the end of the band the four waves add them into one LDS table (one ds_add per register per
//     band, the sum of four waves stays below 2^30), and the workgroup adds the non-zero entries to col[] with 64-bit global integer atomics.
//   * row partials are complete within a wave's row: the lane sums its columns per column phase (|sum| <= 8 * 65535), a butterfly of
//     __shfl_xor adds the 64 lanes (|sum| <= 512 * 65535 < 2^25, int32), the counts travel packed, 10 bits per phase (<= 256 per phase and
//     wave), and lane 0 adds the totals to row[].
//   * cell sums: n and sum d follow from the column partials, sum d^2 is kept per row phase and per column phase relative to the lane's first
//     column in uint64 (d * d + acc is one v_mad_u64_u32); they are widened to 64 bits BEFORE the wave butterfly.
// Period 6: a lane's first column x0 is a multiple of NPX, so x0 % 6 is 0, 2 or 4; sums by relative column phase are rotated to absolute
// phases with two selects each.  The cell centres come from a small LDS table (row phase x 12 entries, read at x0 % 6 + j).
// Grid: blockIdx.x = band * spans + span, blockIdx.y = frame (pair).  The band height starts at 32 (p = 2) or 48 (p = 6) rows per wave and
// doubles while the call would still start more than 8 workgroups per CU (eld_num_cus()): larger bands mean fewer atomics per pixel.
#include "mosaic_dev.h"

namespace {

constexpr int ST = 256;                          // threads per workgroup
constexpr int SWAVES = ST / ELD_WAVE;
constexpr int S_MAX_BH = 8192;                   // rows per band: (8192 / 2) * 65535 < 2^28 bounds every 32-bit column partial
constexpr int S_PAIRS = 64;                      // frame pairs per launch of the cross kernel (they travel as kernel arguments)

struct StructArgs {
    const uint16_t* u;
    const uint32_t* bitmap;
    long long* row;
    long long* col;
    long long* cell;                             // the cross kernel: cross + q0 * p * p
    int Hm, Wm, wpr, bh, nspans;
    int32_t cen[36];
};

struct PairArgs {
    int32_t ab[S_PAIRS][2];
};

__device__ __forceinline__ void add64(long long* p, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// sums by column phase relative to the lane's first column -> absolute phases.  cm = x0 % P (0 when P == 2; 0, 2 or 4 when P == 6):
// relative phase k is absolute phase (cm + k) % P.  KC = the relative phases a lane of NPX columns can hold.
template <int P, int KC, typename T>
__device__ __forceinline__ void rotate_phases(const T (&rel)[KC], int cm, T (&ab)[P]) {
#pragma unroll
    for (int c = 0; c < P; ++c) {
        const T v0 = c < KC ? rel[c < KC ? c : 0] : T(0);
        if constexpr (P == 2) {
            ab[c] = v0;
        } else {
            constexpr int PP = P;
            const int k2 = (c + PP - 2) % PP, k4 = (c + PP - 4) % PP;
            const T v2 = k2 < KC ? rel[k2 < KC ? k2 : 0] : T(0);
            const T v4 = k4 < KC ? rel[k4 < KC ? k4 : 0] : T(0);
            ab[c] = cm == 0 ? v0 : (cm == 2 ? v2 : v4);
        }
    }
}

template <int P, int NPX>
__global__ __launch_bounds__(ST) void struct_sums_kernel(StructArgs a) {
    constexpr int NW = NPX / 2;
    constexpr int KC = P < NPX ? P : NPX;
    constexpr int U = P == 2 ? 4 : P;                            // rows in flight per wave
    constexpr int E = ELD_WAVE * NPX * P * 2;                    // column partials of the span: [lane][j][row phase][n, sum]
    constexpr int NPK = (P + 2) / 3;                             // packed count words: three 10-bit fields each
    __shared__ uint32_t s_col[E + E / 32];                       // entry e lies at e + e / 32: a lane stride of 32 (96) words becomes 33 (99)
    __shared__ int32_t s_cen[P * CELL_ROW];
    const int lane = threadIdx.x & (ELD_WAVE - 1), wave = threadIdx.x / ELD_WAVE;
    const int f = blockIdx.y;
    const int span = blockIdx.x % a.nspans, band = blockIdx.x / a.nspans;
    for (int i = threadIdx.x; i < E + E / 32; i += ST) s_col[i] = 0;
    fill_cell_rows<P>(s_cen, a.cen);
    __syncthreads();

    const int x0 = (span * ELD_WAVE + lane) * NPX;
    const bool act = x0 < a.Wm;                                  // Wm is a multiple of NPX: a lane is inside with all its columns or with none
    const int cm = P == 2 ? 0 : x0 % P;
    const int y0 = band * a.bh, y1 = min(y0 + a.bh, a.Hm);
    const uint16_t* fb = a.u + (size_t)f * a.Hm * a.Wm;
    const int32_t* cenl = s_cen + cm;

    int cn[P][NPX] = {}, cs[P][NPX] = {};
    unsigned long long sq[P][KC] = {};

    for (int yg = y0 + wave * U; yg < y1; yg += SWAVES * U) {
        uint32_t w[U][NW], bad[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int y = yg + i;
            const bool in = act && y < y1;
#pragma unroll
            for (int k = 0; k < NW; ++k) w[i][k] = 0;
            bad[i] = ~0u;
            if (in) {
                load_codes<NPX>(fb + (size_t)y * a.Wm + x0, w[i]);
                bad[i] = a.bitmap ? defect_bits(a.bitmap, a.wpr, y, x0) : 0u;
            }
        }
#pragma unroll
        for (int i = 0; i < U; ++i) {
            constexpr int PP = P;
            const int r = i % PP;                                // yg is a multiple of U, U of P: the row phase of row yg + i
            const int y = yg + i;
            if (y < y1) {                                        // wave-uniform
                int srel[KC] = {}, nrel[KC] = {};
#pragma unroll
                for (int j = 0; j < NPX; ++j) {
                    const int code = (int)((w[i][j / 2] >> (16 * (j & 1))) & 0xFFFFu);   // written out, here and below: code_of changes the NPX = 2 kernels
                    const int good = (int)(~(bad[i] >> j) & 1u);
                    const int d = good ? code - cenl[r * CELL_ROW + j] : 0;
                    cn[r][j] += good;
                    cs[r][j] += d;
                    nrel[j % PP] += good;
                    srel[j % PP] += d;
                    sq[r][j % PP] += (unsigned long long)((long long)d * d);
                }
                int sab[P], nab[P];
                rotate_phases<P, KC>(srel, cm, sab);
                rotate_phases<P, KC>(nrel, cm, nab);
                uint32_t npk[NPK] = {};
#pragma unroll
                for (int c = 0; c < P; ++c) npk[c / 3] += (uint32_t)nab[c] << (10 * (c % 3));
#pragma unroll
                for (int c = 0; c < P; ++c) sab[c] = wave_sum(sab[c]);
#pragma unroll
                for (int k = 0; k < NPK; ++k) npk[k] = wave_sum(npk[k]);
                if (lane == 0) {
                    long long* out = a.row + ((size_t)f * a.Hm + y) * (P * 2);
#pragma unroll
                    for (int c = 0; c < P; ++c) {
                        const int n = (int)((npk[c / 3] >> (10 * (c % 3))) & 1023u);
                        if (n) add64(out + 2 * c, n);
                        if (sab[c]) add64(out + 2 * c + 1, sab[c]);
                    }
                }
            }
        }
    }

    // column partials: the four waves meet in the LDS table
#pragma unroll
    for (int j = 0; j < NPX; ++j)
#pragma unroll
        for (int r = 0; r < P; ++r) {
            const int e = ((lane * NPX + j) * P + r) * 2;
            if (cn[r][j]) atomicAdd(&s_col[e + e / 32], (uint32_t)cn[r][j]);
            if (cs[r][j]) atomicAdd(&s_col[e + 1 + (e + 1) / 32], (uint32_t)cs[r][j]);
        }

    // cell sums of this wave
#pragma unroll
    for (int r = 0; r < P; ++r) {
        long long nrel[KC] = {}, srel[KC] = {}, qrel[KC];
#pragma unroll
        for (int j = 0; j < NPX; ++j) {
            nrel[j % P] += cn[r][j];
            srel[j % P] += cs[r][j];
        }
#pragma unroll
        for (int k = 0; k < KC; ++k) qrel[k] = (long long)sq[r][k];
        long long nab[P], sab[P], qab[P];
        rotate_phases<P, KC>(nrel, cm, nab);
        rotate_phases<P, KC>(srel, cm, sab);
        rotate_phases<P, KC>(qrel, cm, qab);
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const long long n = wave_sum(nab[c]), s = wave_sum(sab[c]), q = wave_sum(qab[c]);
            if (lane == 0 && n) {
                long long* out = a.cell + ((size_t)f * (P * P) + r * P + c) * 3;
                add64(out, n);
                if (s) add64(out + 1, s);
                if (q) add64(out + 2, q);
            }
        }
    }

    __syncthreads();
    const size_t cbase = ((size_t)f * a.Wm + (size_t)span * (ELD_WAVE * NPX)) * (P * 2);
    const int ecols = min(a.Wm - span * (ELD_WAVE * NPX), ELD_WAVE * NPX) * (P * 2);   // entries of the columns inside the frame
    for (int e = threadIdx.x; e < ecols; e += ST) {
        const int v = (int)s_col[e + e / 32];
        if (v) add64(a.col + cbase + e, v);
    }
}

template <int P, int NPX>
__global__ __launch_bounds__(ST) void struct_cross_kernel(StructArgs a, PairArgs pr) {
    constexpr int NW = NPX / 2;
    constexpr int KC = P < NPX ? P : NPX;
    constexpr int U = P == 2 ? 2 : 3;                            // rows in flight per wave and frame (P == 6: two turns make a period)
    __shared__ int32_t s_cen[P * CELL_ROW];
    const int lane = threadIdx.x & (ELD_WAVE - 1), wave = threadIdx.x / ELD_WAVE;
    const int span = blockIdx.x % a.nspans, band = blockIdx.x / a.nspans;
    fill_cell_rows<P>(s_cen, a.cen);
    __syncthreads();

    const int x0 = (span * ELD_WAVE + lane) * NPX;
    const bool act = x0 < a.Wm;
    const int cm = P == 2 ? 0 : x0 % P;
    const int y0 = band * a.bh, y1 = min(y0 + a.bh, a.Hm);
    const uint16_t* fa = a.u + (size_t)pr.ab[blockIdx.y][0] * a.Hm * a.Wm;
    const uint16_t* fb = a.u + (size_t)pr.ab[blockIdx.y][1] * a.Hm * a.Wm;
    const int32_t* cenl = s_cen + cm;

    long long acc[P][KC] = {};
    for (int yg = y0 + wave * P; yg < y1; yg += SWAVES * P) {    // a wave's turn is one period of rows, in P / U steps
#pragma unroll
        for (int h = 0; h < P / U; ++h) {
            uint32_t wa[U][NW], wb[U][NW], bad[U];
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const int y = yg + h * U + i;
#pragma unroll
                for (int k = 0; k < NW; ++k) wa[i][k] = wb[i][k] = 0;
                bad[i] = ~0u;
                if (act && y < y1) {
                    load_codes<NPX>(fa + (size_t)y * a.Wm + x0, wa[i]);
                    load_codes<NPX>(fb + (size_t)y * a.Wm + x0, wb[i]);
                    bad[i] = a.bitmap ? defect_bits(a.bitmap, a.wpr, y, x0) : 0u;
                }
            }
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const int r = h * U + i;                         // yg is a multiple of P
#pragma unroll
                for (int j = 0; j < NPX; ++j) {
                    const int good = (int)(~(bad[i] >> j) & 1u);
                    const int c = cenl[r * CELL_ROW + j];
                    const int da = good ? (int)((wa[i][j / 2] >> (16 * (j & 1))) & 0xFFFFu) - c : 0;
                    const int db = (int)((wb[i][j / 2] >> (16 * (j & 1))) & 0xFFFFu) - c;
                    acc[r][j % P] += (long long)da * db;         // |da db| < 2^32, at most Hm * Wm < 2^31 terms
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < P; ++r) {
        long long ab[P];
        rotate_phases<P, KC>(acc[r], cm, ab);
#pragma unroll
        for (int c = 0; c < P; ++c) {
            const long long s = wave_sum(ab[c]);
            if (lane == 0 && s) add64(a.cell + (size_t)blockIdx.y * (P * P) + r * P + c, s);
        }
    }
}

// rows per band: a multiple of `unit` (the rows the four waves take per turn); doubled while the call would start more than 8 workgroups per CU
int band_height(int Hm, int nspans, int others, int unit) {
    int bh = unit * 8;
    const long long cap = 8ll * eld_num_cus();
    while (bh * 2 <= S_MAX_BH && (long long)((Hm + bh - 1) / bh) * nspans * others > cap) bh *= 2;
    return bh;
}

// the argument rules the two entries share; 0 = go on
int check_common(const uint16_t* u, int F, int Hm, int Wm, int p, const int32_t* centre, const uint32_t* bitmap) {
    if ((p != 2 && p != 6) || F < 0 || F > 65535 || Hm < 0 || Wm < 0 || Wm % 2 || !centre) return ELD_EINVAL;
    if ((uint64_t)Hm * (uint64_t)Wm >= (1ull << 31)) return ELD_EINVAL;
    for (int k = 0; k < p * p; ++k)
        if (centre[k] < 0 || centre[k] > 65535) return ELD_EINVAL;
    if (((uintptr_t)u & 3u) || ((uintptr_t)bitmap & 3u)) return ELD_EINVAL;
    if (F > 0 && Hm > 0 && Wm > 0 && !u) return ELD_EINVAL;
    return 0;
}

bool bad_out(const void* p, size_t n) { return ((uintptr_t)p & 7u) || (n && !p); }

void fill_args(StructArgs& a, const uint16_t* u, int Hm, int Wm, int p, const int32_t* centre, const uint32_t* bitmap, bool vec, int others) {
    a.u = u; a.bitmap = bitmap;
    a.Hm = Hm; a.Wm = Wm; a.wpr = bitmap_pitch(Wm);
    const int lane_cols = ELD_WAVE * (vec ? 8 : 2);
    a.nspans = (Wm + lane_cols - 1) / lane_cols;
    a.bh = band_height(Hm, a.nspans, others, SWAVES * (p == 2 ? 4 : 6));
    for (int k = 0; k < 36; ++k) a.cen[k] = k < p * p ? centre[k] : 0;
}

}  // namespace

extern "C" int eld_struct_sums_u16(const uint16_t* u, int F, int Hm, int Wm, int p, const int32_t* centre, const uint32_t* bitmap, int64_t* row,
                                   int64_t* col, int64_t* cell, void* stream) {
    int rc = check_common(u, F, Hm, Wm, p, centre, bitmap);
    if (rc) return rc;
    const size_t nrow = (size_t)F * Hm * p * 2, ncol = (size_t)F * Wm * p * 2, ncell = (size_t)F * p * p * 3;
    if (bad_out(row, nrow) || bad_out(col, ncol) || bad_out(cell, ncell)) return ELD_EINVAL;
    if (F == 0) return 0;
    hipStream_t s = as_stream(stream);
    if ((rc = zero_u64(row, nrow, s)) || (rc = zero_u64(col, ncol, s)) || (rc = zero_u64(cell, ncell, s))) return rc;
    if (Hm == 0 || Wm == 0) return 0;
    const bool vec = Wm % 8 == 0 && !((uintptr_t)u & 15u);
    StructArgs a;
    fill_args(a, u, Hm, Wm, p, centre, bitmap, vec, F);
    a.row = (long long*)row; a.col = (long long*)col; a.cell = (long long*)cell;
    const dim3 grid((unsigned)((Hm + a.bh - 1) / a.bh) * (unsigned)a.nspans, (unsigned)F);
    if (p == 2) {
        if (vec) ELD_LAUNCH((struct_sums_kernel<2, 8>), grid, dim3(ST), 0, s, a);
        else ELD_LAUNCH((struct_sums_kernel<2, 2>), grid, dim3(ST), 0, s, a);
    } else {
        if (vec) ELD_LAUNCH((struct_sums_kernel<6, 8>), grid, dim3(ST), 0, s, a);
        else ELD_LAUNCH((struct_sums_kernel<6, 2>), grid, dim3(ST), 0, s, a);
    }
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_struct_cross_u16(const uint16_t* u, int F, int Hm, int Wm, int p, const int32_t* centre, const uint32_t* bitmap,
                                    const int32_t* pairs, int Q, int64_t* cross, void* stream) {
    int rc = check_common(u, F, Hm, Wm, p, centre, bitmap);
    if (rc) return rc;
    if (Q < 0 || Q > (1 << 24) || (Q && !pairs)) return ELD_EINVAL;
    for (int q = 0; q < 2 * Q; ++q)
        if (pairs[q] < 0 || pairs[q] >= F) return ELD_EINVAL;
    const size_t ncross = (size_t)Q * p * p;
    if (bad_out(cross, ncross)) return ELD_EINVAL;
    if (Q == 0) return 0;
    hipStream_t s = as_stream(stream);
    if ((rc = zero_u64(cross, ncross, s))) return rc;
    if (Hm == 0 || Wm == 0) return 0;
    const bool vec = Wm % 8 == 0 && !((uintptr_t)u & 15u);
    StructArgs a;
    fill_args(a, u, Hm, Wm, p, centre, bitmap, vec, Q < S_PAIRS ? Q : S_PAIRS);
    a.row = a.col = nullptr;
    for (int q0 = 0; q0 < Q; q0 += S_PAIRS) {
        const int nq = Q - q0 < S_PAIRS ? Q - q0 : S_PAIRS;
        PairArgs pr = {};
        for (int q = 0; q < nq; ++q) {
            pr.ab[q][0] = pairs[2 * (q0 + q)];
            pr.ab[q][1] = pairs[2 * (q0 + q) + 1];
        }
        a.cell = (long long*)cross + (size_t)q0 * p * p;
        const dim3 grid((unsigned)((Hm + a.bh - 1) / a.bh) * (unsigned)a.nspans, (unsigned)nq);
        if (p == 2) {
            if (vec) ELD_LAUNCH((struct_cross_kernel<2, 8>), grid, dim3(ST), 0, s, a, pr);
            else ELD_LAUNCH((struct_cross_kernel<2, 2>), grid, dim3(ST), 0, s, a, pr);
        } else {
            if (vec) ELD_LAUNCH((struct_cross_kernel<6, 8>), grid, dim3(ST), 0, s, a, pr);
            else ELD_LAUNCH((struct_cross_kernel<6, 2>), grid, dim3(ST), 0, s, a, pr);
        }
        ELD_LAUNCH_CHECK();
    }
    return 0;
}
