// flatfield.hip -- flat-field maps: what multiplies the signal (pixel response non-uniformity and lens shading), measured from the flat pairs of
// a calibration manifest and divided out (eld_amd/flatfield.py).
//
//   eld_flat_sums_u16                  flat frames in a frame pool -> per site S = sum of codes, D = sum over pairs of (a - b)^2, a bad flag
//   eld_flat_box_u32                   S and the flag -> per site the sum and the count of the good sites of its window, in its position plane
//   eld_flat_apply_u16                 uint16 codes [N,Hm,Wm] -> clamp(rint((u - black) * gain + black), 0, 65535)
// The input stage that multiplies by the gain plane in float32 (eld_pack_raw_*_u16_flat) is in pack_raw.hip.
// The first two are integer arithmetic throughout: their outputs do not depend on the launch geometry, and tests/flatfield_ref.py restates them
// (and the float32 operation order of the other three) in NumPy.  The library is built with -ffp-contract=off; the pragma says so for this file.
//
// Sums and apply: a lane owns 8 consecutive columns of one row, as in shading.hip (one 16-byte load of codes where the row pitch and the frame's
// start allow it, else one word per column pair).  The flag bitmap has pack_bitmap's layout (bit x & 31 of word [y][x >> 5]); a lane's 8 bits are
// one BYTE of it, written with one byte store: no atomics, and the pad bytes of a row are written (zero) by the row's last lane.
//
// Box: the window of a site is (2R + 1)^2 sites at steps of the period p around it, clipped at the frame.  Two separable passes over one packed
// 64-bit word per site, (S << 16) | 1 at a good site and 0 at a bad one: the low 16 bits count (at most 129^2 = 16641 < 2^16), the rest sums
// (S < 2^32, so a window stays below 2^47 and the packed word below 2^63).  Integer adds in any order are exact, so both passes are running
// sums: a lane starts its segment with the 2R + 1 taps of its first window and then slides (one tap in, one out).
//   rows     a workgroup stages FF_TW<P> columns of one row plus p R on either side in LDS (coalesced reads), each lane slides along FF_SEG
//            plane columns of one column phase, results go back through LDS for coalesced 8-byte stores into the workspace
//   columns  a lane owns one mosaic column (coalesced across the wave) and slides down FF_VSEG plane rows of each of the p row phases
// The cost per site is 2 + (2R + 1) / FF_SEG LDS reads and 2 + (2R + 1) / FF_VSEG global reads: linear in R with a small slope, not R^2.
#include "mosaic_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int FF_T = 256;                        // threads per workgroup
constexpr int FF_MAX_FRAMES = 65536;             // 65536 * 65535 < 2^32 keeps S exact in uint32
constexpr int FF_MAX_RADIUS = 64;
constexpr int FF_SEG = 9;                        // plane columns per lane of the row pass (odd: lanes of a wave spread over the LDS banks)
constexpr int FF_VSEG = 16;                      // plane rows per lane and row phase of the column pass

template <int P> struct BoxTile {
    static constexpr int NSEG = FF_T / P;                        // segments per workgroup and column phase
    static constexpr int TW = NSEG * FF_SEG * P;                 // mosaic columns per workgroup of the row pass: 2304 (p = 2), 2268 (p = 6)
    static constexpr int LW = TW + 2 * P * FF_MAX_RADIUS;        // with the halo of the largest radius
    static constexpr int TH = P * FF_VSEG;                       // mosaic rows per workgroup of the column pass: 32, 96
};

struct SumsArgs {
    const uint16_t* pool;
    size_t pool_elems;
    const EldPoolFrame* frames;
    const uint32_t* bitmap;
    uint32_t* S;
    uint64_t* D;
    uint32_t* bad;
    int Hm, Wm, wpr, lpr, F, white, vec_in, vec_out;   // lpr = lanes per row = ceil(Wm / 8)
};

struct ApplyArgs {
    const uint16_t* in;
    uint16_t* out;
    const float* gain;
    const uint32_t* bitmap;
    int N, Hm, Wm, wpr, lpr, white;
    float black[36];
};

// ---- pass 1: one read of every flat code ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FF_T) void flat_sums_kernel(SumsArgs a) {
    const uint32_t units = (uint32_t)a.Hm * (uint32_t)a.lpr;             // Hm * Wm < 2^31
    const size_t fsz = (size_t)a.Hm * a.Wm;
    for (uint32_t i = blockIdx.x * FF_T + threadIdx.x; i < units; i += gridDim.x * FF_T) {
        const int y = (int)(i / (uint32_t)a.lpr), l = (int)(i - (uint32_t)y * (uint32_t)a.lpr), x0 = l * ROW_NPX;
        const size_t site = (size_t)y * a.Wm + x0;
        uint32_t T[ROW_NPX], sat = 0u;
        uint64_t Q[ROW_NPX];
#pragma unroll
        for (int j = 0; j < ROW_NPX; ++j) { T[j] = 0u; Q[j] = 0ull; }
        for (int f0 = 0; f0 < a.F; f0 += POOL_U) {                       // F is even: a group of four holds whole pairs
            const uint16_t* src[POOL_U];
            bool ok[POOL_U], wide = a.vec_in;
#pragma unroll
            for (int u = 0; u < POOL_U; ++u) {                           // launch-uniform: the table entry decides, not the lane
                ok[u] = f0 + u < a.F;
                src[u] = a.pool;
                if (ok[u]) {
                    const EldPoolFrame e = a.frames[f0 + u];
                    // an entry that is not an Hm x Wm frame inside the pool contributes no codes: nothing outside the pool is read
                    ok[u] = e.Hm == a.Hm && e.Wm == a.Wm && !(e.offset & 1u) && e.offset <= a.pool_elems && fsz <= a.pool_elems - e.offset;
                    if (ok[u]) {
                        src[u] = a.pool + e.offset + site;
                        wide = wide && e.offset % ROW_NPX == 0;
                    }
                }
            }
            uint32_t w[POOL_U][4];
            if (wide) {
#pragma unroll
                for (int u = 0; u < POOL_U; ++u) {
                    if (ok[u]) load_codes8<true>(src[u], x0, a.Wm, w[u]);
                    else w[u][0] = w[u][1] = w[u][2] = w[u][3] = 0u;
                }
            } else {
#pragma unroll
                for (int u = 0; u < POOL_U; ++u) {
                    if (ok[u]) load_codes8<false>(src[u], x0, a.Wm, w[u]);
                    else w[u][0] = w[u][1] = w[u][2] = w[u][3] = 0u;
                }
            }
#pragma unroll
            for (int h = 0; h < POOL_U / 2; ++h)
#pragma unroll
                for (int j = 0; j < ROW_NPX; ++j) {
                    const uint32_t ca = code_of(w[2 * h], j), cb = code_of(w[2 * h + 1], j);
                    const uint32_t d = ca > cb ? ca - cb : cb - ca;
                    T[j] += ca + cb;
                    Q[j] += (uint64_t)(d * d);                           // d <= 65535: the square fits 32 bits
                    sat |= (uint32_t)(((int)ca >= a.white) | ((int)cb >= a.white)) << j;
                }
        }
        uint32_t flag = sat | (a.bitmap ? defect_bits(a.bitmap, a.wpr, y, x0) : 0u);
        const int inside = a.Wm - x0 < ROW_NPX ? a.Wm - x0 : ROW_NPX;    // columns of this lane that lie in the row: no bits beyond it
        flag &= (1u << inside) - 1u;
        uint8_t* bytes = reinterpret_cast<uint8_t*>(a.bad) + (size_t)y * a.wpr * 4;
        bytes[l] = (uint8_t)flag;
        if (l == a.lpr - 1)
            for (int k = a.lpr; k < a.wpr * 4; ++k) bytes[k] = 0;        // the pad bytes of the row's last word
        if (a.vec_out) {
            uint4* ps = reinterpret_cast<uint4*>(a.S + site);
            ps[0] = make_uint4(T[0], T[1], T[2], T[3]); ps[1] = make_uint4(T[4], T[5], T[6], T[7]);
            ulonglong2* pd = reinterpret_cast<ulonglong2*>(a.D + site);
#pragma unroll
            for (int k = 0; k < 4; ++k) pd[k] = make_ulonglong2(Q[2 * k], Q[2 * k + 1]);
        } else {
#pragma unroll
            for (int j = 0; j < ROW_NPX; ++j)
                if (x0 + j < a.Wm) { a.S[site + j] = T[j]; a.D[site + j] = Q[j]; }
        }
    }
}

// ---- pass 2: the window sums ---------------------------------------------------------------------------------------------------------------------
// rows: ws[y][x] = sum over |d| <= R, 0 <= x + p d < Wm of the packed word of site (y, x + p d)
template <int P>
__global__ __launch_bounds__(FF_T) void flat_box_rows_kernel(const uint32_t* __restrict__ S, const uint32_t* __restrict__ bad, uint64_t* __restrict__ ws,
                                                             int Hm, int Wm, int wpr, int R, int tiles_x) {
    using BT = BoxTile<P>;
    __shared__ uint64_t g[BT::LW];
    __shared__ uint64_t res[BT::TW];
    const int y = (int)(blockIdx.x / (unsigned)tiles_x), xt = (int)(blockIdx.x % (unsigned)tiles_x) * BT::TW;
    const int halo = P * R, n = BT::TW + 2 * halo;                       // n <= LW because R <= FF_MAX_RADIUS
    const int t = threadIdx.x;
    for (int k = t; k < n; k += FF_T) {
        const int x = xt - halo + k;
        uint64_t v = 0ull;
        if (x >= 0 && x < Wm && !defect_bit(bad, wpr, y, x)) v = ((uint64_t)S[(size_t)y * Wm + x] << 16) | 1ull;
        g[k] = v;
    }
    __syncthreads();
    if (t < BT::NSEG * P) {
        const int c = t % P, s = t / P;
        int base = P * (s * FF_SEG) + c;                                 // LDS index of the leftmost tap of the segment's first window
        if (xt + base < Wm) {
            uint64_t acc = 0ull;
            for (int d = 0; d <= 2 * R; ++d) acc += g[base + P * d];
            for (int k = 0;; ++k) {
                res[base] = acc;                                         // base < TW
                if (k + 1 == FF_SEG) break;
                acc += g[base + P * (2 * R + 1)] - g[base];              // base <= TW - 2 P + c here: the tap in lies below TW + 2 halo = n
                base += P;
            }
        }
    }
    __syncthreads();
    uint64_t* o = ws + (size_t)y * Wm;
    for (int k = t; k < BT::TW; k += FF_T)
        if (xt + k < Wm) o[xt + k] = res[k];
}

// columns: the same sum down the rows of ws, then unpacked
template <int P>
__global__ __launch_bounds__(FF_T) void flat_box_cols_kernel(const uint64_t* __restrict__ ws, uint64_t* __restrict__ Bsum, uint32_t* __restrict__ Bcnt,
                                                             int Hm, int Wm, int R, int tiles_x) {
    const int x = (int)(blockIdx.x % (unsigned)tiles_x) * FF_T + threadIdx.x;
    const int y0 = (int)(blockIdx.x / (unsigned)tiles_x) * BoxTile<P>::TH;
    if (x >= Wm) return;
    for (int r = 0; r < P; ++r) {
        int y = y0 + r;
        if (y >= Hm) break;
        uint64_t acc = 0ull;
        for (int d = -R; d <= R; ++d) {
            const int yy = y + P * d;                                    // |P d| <= 384, y < 2^30
            if (yy >= 0 && yy < Hm) acc += ws[(size_t)yy * Wm + x];
        }
        for (int k = 0; k < FF_VSEG && y < Hm; ++k) {
            Bsum[(size_t)y * Wm + x] = acc >> 16;
            Bcnt[(size_t)y * Wm + x] = (uint32_t)(acc & 0xFFFFull);
            const int yin = y + P * (R + 1), yout = y - P * R;
            if (yin < Hm) acc += ws[(size_t)yin * Wm + x];
            if (yout >= 0) acc -= ws[(size_t)yout * Wm + x];
            y += P;
        }
    }
}

// ---- the integer path ----------------------------------------------------------------------------------------------------------------------------
// in and out may be the same buffer: a lane reads its own 8 codes of a frame before it writes them, and touches no others
template <int P, bool VEC>
__global__ __launch_bounds__(FF_T) void flat_apply_kernel(ApplyArgs a) {
    __shared__ float s_blk[P * CELL_ROW];
    fill_cell_rows<P>(s_blk, a.black);
    __syncthreads();
    const uint32_t units = (uint32_t)a.Hm * (uint32_t)a.lpr;
    const size_t fsz = (size_t)a.Hm * a.Wm;
    for (uint32_t i = blockIdx.x * FF_T + threadIdx.x; i < units; i += gridDim.x * FF_T) {
        const int y = (int)(i / (uint32_t)a.lpr), x0 = (int)(i - (uint32_t)y * (uint32_t)a.lpr) * ROW_NPX;
        const size_t site = (size_t)y * a.Wm + x0;
        const float* blk = s_blk + (y % P) * CELL_ROW + (P == 2 ? 0 : x0 % P);
        float fg[ROW_NPX];
        if (VEC) {
            const float4 g0 = reinterpret_cast<const float4*>(a.gain + site)[0], g1 = reinterpret_cast<const float4*>(a.gain + site)[1];
            fg[0] = g0.x; fg[1] = g0.y; fg[2] = g0.z; fg[3] = g0.w; fg[4] = g1.x; fg[5] = g1.y; fg[6] = g1.z; fg[7] = g1.w;
        } else {
#pragma unroll
            for (int j = 0; j < ROW_NPX; ++j) fg[j] = x0 + j < a.Wm ? a.gain[site + j] : 1.f;
        }
        const uint32_t bad = a.bitmap ? defect_bits(a.bitmap, a.wpr, y, x0) : 0u;
        for (int n = 0; n < a.N; ++n) {
            uint32_t w[4], o[4];
            load_codes8<VEC>(a.in + (size_t)n * fsz + site, x0, a.Wm, w);
            int q[ROW_NPX];
#pragma unroll
            for (int j = 0; j < ROW_NPX; ++j) {
                const int u = (int)code_of(w, j);
                const float v = (float)u - blk[j];
                const float m = v * fg[j];
                const float r = fminf(fmaxf(rintf(m + blk[j]), 0.f), 65535.f);           // ties to even; clamped before the conversion
                q[j] = (((bad >> j) & 1u) || u >= a.white) ? u : (int)r;                 // a flagged or saturated site passes through
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (uint32_t)q[2 * k] | ((uint32_t)q[2 * k + 1] << 16);
            uint16_t* dst = a.out + (size_t)n * fsz + site;
            if (VEC) {
                *reinterpret_cast<uint4*>(dst) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (x0 + 2 * k < a.Wm) *reinterpret_cast<uint32_t*>(dst + 2 * k) = o[k];
            }
        }
    }
}

template <int P>
int box_launch(const uint32_t* S, const uint32_t* bad, int Hm, int Wm, int radius, uint64_t* Bsum, uint32_t* Bcnt, uint64_t* ws, hipStream_t st) {
    const int wpr = bitmap_pitch(Wm);
    const long long tx = (Wm + BoxTile<P>::TW - 1) / BoxTile<P>::TW, nb1 = tx * Hm;
    const long long cx = (Wm + FF_T - 1) / FF_T, nb2 = cx * ((Hm + BoxTile<P>::TH - 1) / BoxTile<P>::TH);
    if (nb1 > 0x7FFFFFFFll || nb2 > 0x7FFFFFFFll) return ELD_EINVAL;
    ELD_LAUNCH(flat_box_rows_kernel<P>, dim3((unsigned)nb1), dim3(FF_T), 0, st, S, bad, ws, Hm, Wm, wpr, radius, (int)tx);
    ELD_LAUNCH_CHECK();
    ELD_LAUNCH(flat_box_cols_kernel<P>, dim3((unsigned)nb2), dim3(FF_T), 0, st, ws, Bsum, Bcnt, Hm, Wm, radius, (int)cx);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int eld_flat_sums_u16(const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int Hm, int Wm, int white_level,
                                 const uint32_t* bitmap, uint32_t* S, uint64_t* D, uint32_t* bad, void* stream) {
    if (bad_shape(Hm, Wm) || F < 2 || F % 2 || F > FF_MAX_FRAMES || white_level < 1 || white_level > 65536) return ELD_EINVAL;
    if (((uintptr_t)pool & 3u) || ((uintptr_t)bitmap & 3u) || ((uintptr_t)frames & 7u) || ((uintptr_t)S & 3u) || ((uintptr_t)D & 7u) || ((uintptr_t)bad & 3u))
        return ELD_EINVAL;
    if (Hm == 0 || Wm == 0) return 0;
    if (!pool || !frames || !S || !D || !bad) return ELD_EINVAL;
    SumsArgs a;
    a.pool = pool; a.pool_elems = pool_elems; a.frames = frames; a.bitmap = bitmap; a.S = S; a.D = D; a.bad = bad;
    a.Hm = Hm; a.Wm = Wm; a.wpr = bitmap_pitch(Wm); a.lpr = (Wm + ROW_NPX - 1) / ROW_NPX; a.F = F; a.white = white_level;
    a.vec_in = Wm % ROW_NPX == 0 && !((uintptr_t)pool & 15u);
    a.vec_out = Wm % ROW_NPX == 0 && !(((uintptr_t)S | (uintptr_t)D) & 15u);
    ELD_LAUNCH(flat_sums_kernel, dim3(stride_grid((uint32_t)Hm * (uint32_t)a.lpr, FF_T)), dim3(FF_T), 0, as_stream(stream), a);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t eld_flat_box_workspace_bytes(int Hm, int Wm) {
    if (bad_shape(Hm, Wm)) return 0;
    return (size_t)Hm * (size_t)Wm * sizeof(uint64_t);
}

extern "C" int eld_flat_box_tile(int period, int* row_pass_columns, int* column_pass_rows) {
    if ((period != 2 && period != 6) || !row_pass_columns || !column_pass_rows) return ELD_EINVAL;
    *row_pass_columns = period == 2 ? BoxTile<2>::TW : BoxTile<6>::TW;
    *column_pass_rows = period == 2 ? BoxTile<2>::TH : BoxTile<6>::TH;
    return 0;
}

extern "C" int eld_flat_box_u32(const uint32_t* S, const uint32_t* bad, int Hm, int Wm, int period, int radius, uint64_t* Bsum, uint32_t* Bcnt,
                                void* ws, size_t ws_bytes, void* stream) {
    if ((period != 2 && period != 6) || bad_shape(Hm, Wm) || radius < 0 || radius > FF_MAX_RADIUS) return ELD_EINVAL;
    if (((uintptr_t)S & 3u) || ((uintptr_t)bad & 3u) || ((uintptr_t)Bsum & 7u) || ((uintptr_t)Bcnt & 3u) || ((uintptr_t)ws & 7u)) return ELD_EINVAL;
    if (Hm == 0 || Wm == 0) return 0;
    if (!S || !bad || !Bsum || !Bcnt || !ws) return ELD_EINVAL;
    if (ws_bytes < eld_flat_box_workspace_bytes(Hm, Wm)) return ELD_EWS;
    if (period == 2) return box_launch<2>(S, bad, Hm, Wm, radius, Bsum, Bcnt, (uint64_t*)ws, as_stream(stream));
    return box_launch<6>(S, bad, Hm, Wm, radius, Bsum, Bcnt, (uint64_t*)ws, as_stream(stream));
}

extern "C" int eld_flat_apply_u16(const uint16_t* in, uint16_t* out, int N, int Hm, int Wm, const float* gain, const float* black, int period,
                                  int white_level, const uint32_t* bitmap, void* stream) {
    if ((period != 2 && period != 6) || bad_shape(Hm, Wm) || N < 0 || white_level < 1 || white_level > 65536 || !black) return ELD_EINVAL;
    for (int k = 0; k < period * period; ++k)
        if (!(black[k] >= 0.f && black[k] <= 65535.f)) return ELD_EINVAL;
    if (((uintptr_t)in & 3u) || ((uintptr_t)out & 3u) || ((uintptr_t)bitmap & 3u) || ((uintptr_t)gain & 3u)) return ELD_EINVAL;
    if (N == 0 || Hm == 0 || Wm == 0) return 0;
    if (!in || !out || !gain) return ELD_EINVAL;
    ApplyArgs a;
    a.in = in; a.out = out; a.gain = gain; a.bitmap = bitmap;
    a.N = N; a.Hm = Hm; a.Wm = Wm; a.wpr = bitmap_pitch(Wm); a.lpr = (Wm + ROW_NPX - 1) / ROW_NPX; a.white = white_level;
    for (int k = 0; k < 36; ++k) a.black[k] = k < period * period ? black[k] : 0.f;
    // Wm % 8 == 0 makes a frame a multiple of 16 bytes: every frame of an aligned stack is aligned
    const bool vec = Wm % ROW_NPX == 0 && !(((uintptr_t)in | (uintptr_t)out | (uintptr_t)gain) & 15u);
    const dim3 grid(stride_grid((uint32_t)Hm * (uint32_t)a.lpr, FF_T));
    if (period == 2) {
        if (vec) ELD_LAUNCH((flat_apply_kernel<2, true>), grid, dim3(FF_T), 0, as_stream(stream), a);
        else ELD_LAUNCH((flat_apply_kernel<2, false>), grid, dim3(FF_T), 0, as_stream(stream), a);
    } else {
        if (vec) ELD_LAUNCH((flat_apply_kernel<6, true>), grid, dim3(FF_T), 0, as_stream(stream), a);
        else ELD_LAUNCH((flat_apply_kernel<6, false>), grid, dim3(FF_T), 0, as_stream(stream), a);
    }
    ELD_LAUNCH_CHECK();
    return 0;
}
