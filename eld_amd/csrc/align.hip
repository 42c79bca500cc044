// align.hip -- register a hand-held burst to one of its frames and stack it through the displacement field (eld_amd/burst.py).
//
//   eld_burst_luma_pyramid_u16    frames uint16 [N,Hm,Wm] -> every level of every frame's luma pyramid, uint16
//   eld_burst_align_u16           frames -> disp int16 [N,TY0,TX0,2] (dy, dx in luma units = CFA periods), cost uint32 [N,TY0,TX0]
//   eld_burst_stack_aligned_u16   frames, disp -> mean, kept, present, ptc: eld_burst_stack_u16 over the samples the field points at
// The contract (luma, pyramid, tiles, candidates, key, presence) is in include/eld_amd.h; tests/align_ref.py restates it in NumPy.
//
// Operand widths (codes <= 65535, p*p <= 36, T = 16, R = 4, at most 4 levels):
//   a cell sum <= 36 * 65535 < 2^22 and a 2 x 2 sum + 2 < 2^18 (uint32); a tile's cost <= 256 * 65535 < 2^24, a half tile's < 2^23;
//   the key (cost << 7) | rank < 2^31 with rank < 81 < 2^7: a signed 32-bit minimum orders it;
//   |disp| <= R (1 + 2 + 4 + 8) = 60 at level 0 (a start is twice the parent's displacement, at most 2 * 28 = 56, plus R), int16;
//   a sample's row y + p dy lies in (-361, Hm + 361): int32, tested against [0, Hm) before it becomes an address.
//
// Search: one wave per tile, four tiles per 256-thread workgroup, one launch per level over all (frame != ref, tile) pairs.  The wave stages the
// reference tile (16 x 16) and the alternate frame's 24 x 24 window around the start (coordinates clamped to the level) in LDS, the window
// twice: as it is and one pixel to the left, so that a row of 16 pixels at any offset 0..8 starts on a 32-bit word of one of the two.  The
// 81 candidates x 2 half tiles are 162 work items over 64 lanes (three turns, 84 % of the lanes busy); an item is 64 v_sad_u16 (two pixels
// each) over words read from LDS, the reference words as broadcasts.  The halves meet through LDS, every lane forms the keys of its one
// or two candidates, and the minimum is taken in registers: four DPP row rotations, then four lane reads.  Integer only, no scratch.
//
// Aligned stack: the unit is two adjacent sites of a row (one 32-bit word: a displacement moves a row by p dx pixels, p even, so a shifted row is
// only 4-byte aligned and 32-bit loads are the wide path here; 16-byte loads are burst.hip's privilege) or one site (2-byte loads: an odd base or an
// odd width).  A tile boundary is a multiple of 16 p pixels, so both sites of a word share a tile and a presence.  An absent sample's load is
// turned onto the site itself (always inside the frame) and masked, so the loads of four frames stay in flight.  The rule is burst_dev.h's
// with N = M, the site's present samples; whether a site needs the second look is decided by putting its smallest and its largest sample
// to the rule itself (a sample is rejected only if every sample at least as far from the mean is: head of burst.hip), exact in 64 bits.
#include "burst_dev.h"

namespace {

constexpr int AL_T = 16;                         // tile side, luma pixels
constexpr int AL_R = 4;                          // search radius per level
constexpr int AL_D = 2 * AL_R + 1;               // candidates per axis
constexpr int AL_NC = AL_D * AL_D;               // 81
constexpr int AL_WIN = AL_T + 2 * AL_R;          // 24
constexpr int AL_S = 13;                         // words per window row in LDS (12 used; odd: rows fall on different banks)
constexpr int AL_MAXL = 4;
constexpr int AL_MAXD = AL_R * (1 + 2 + 4 + 8);  // 60
constexpr int AL_ITEMS = 2 * AL_NC;              // (candidate, half tile)
constexpr int AL_TURNS = (AL_ITEMS + ELD_WAVE - 1) / ELD_WAVE;
constexpr int AL_WAVES = BT / ELD_WAVE;          // tiles per workgroup
static_assert(AL_T == 16 && AL_T % 2 == 0 && AL_WIN % 2 == 0 && 2 * AL_S >= AL_WIN, "a tile row is 8 words, a window row 12");
static_assert(36ll * 65535 + 18 < (1ll << 22), "a cell sum");
static_assert((long long)AL_T * AL_T * 65535 < (1ll << 24), "a tile's cost < 2^24");
static_assert(AL_NC <= 128 && ((((long long)AL_T * AL_T * 65535) << 7) | (AL_NC - 1)) < (1ll << 31), "the key < 2^31");
static_assert(AL_MAXD == 60 && 6 * AL_MAXD < 32768, "displacements: int16 in luma units and in pixels");
static_assert(AL_NC <= 2 * ELD_WAVE, "two candidates per lane at most");
static_assert((long long)BT * 8 * 2 * (1 << 14) < (1ll << 32), "32-bit partial sums of V >> 32 and of the site count (aligned stack)");

// rank of candidate k = (v + R) * D + (u + R) in ascending (|v| + |u|, v, u), and the candidate of a rank
struct AlTables {
    uint8_t rank[AL_NC], cand[AL_NC];
};
constexpr AlTables al_make_tables() {
    AlTables t{};
    int r = 0;
    for (int m = 0; m <= 2 * AL_R; ++m)
        for (int v = -AL_R; v <= AL_R; ++v)
            for (int u = -AL_R; u <= AL_R; ++u)
                if ((v < 0 ? -v : v) + (u < 0 ? -u : u) == m) {
                    const int k = (v + AL_R) * AL_D + (u + AL_R);
                    t.rank[k] = (uint8_t)r;
                    t.cand[r] = (uint8_t)k;
                    ++r;
                }
    return t;
}
__constant__ AlTables al_tab = al_make_tables();
static_assert(al_make_tables().cand[0] == AL_R * AL_D + AL_R && al_make_tables().rank[AL_NC - 1] == AL_NC - 1, "rank 0 is the start; (R, R) is last");

struct Level {
    int h, w, ty, tx;
    size_t lum_off, disp_off;                    // elements: into the pyramid, into the per-level displacement fields
};

// -> levels' geometry, or false when the arguments do not describe a pyramid
bool al_geometry(int N, int Hm, int Wm, int p, int levels, Level* lv, size_t* lum_elems, size_t* disp_elems) {
    if ((p != 2 && p != 6) || N < 2 || N > 256 || Hm < 1 || Wm < 1 || levels < 1 || levels > AL_MAXL) return false;
    if ((uint64_t)Hm * (uint64_t)Wm >= (1ull << 31)) return false;
    int h = Hm / p, w = Wm / p;
    size_t lo = 0, dofs = 0;
    for (int l = 0; l < levels; ++l) {
        if (h < AL_T || w < AL_T) return false;
        lv[l].h = h; lv[l].w = w;
        lv[l].ty = (h + AL_T - 1) / AL_T; lv[l].tx = (w + AL_T - 1) / AL_T;
        lv[l].lum_off = lo; lv[l].disp_off = dofs;
        lo += (size_t)N * h * w;
        if (l > 0) dofs += (size_t)N * lv[l].ty * lv[l].tx * 2;
        h = (h + 1) / 2; w = (w + 1) / 2;
    }
    *lum_elems = lo; *disp_elems = dofs;
    return true;
}

// ---- luma and pyramid ------------------------------------------------------------------------------------------------------------------------
template <int P, bool W32>
__global__ __launch_bounds__(256) void luma_kernel(const uint16_t* __restrict__ frames, uint16_t* __restrict__ out, int Hm, int Wm, int Wl, uint32_t cells,
                                                   FastDiv dwl) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cells) return;
    const uint32_t Y = fdiv_u32(i, dwl), X = i - Y * (uint32_t)Wl;
    const uint16_t* src = frames + (size_t)blockIdx.y * ((size_t)Hm * Wm) + (size_t)(Y * P) * Wm + X * P;       // Y P + P - 1 < Hm, X P + P - 1 < Wm
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < P; ++r) {
        if constexpr (W32) {                                     // frames 4-byte aligned, Wm and P even: every cell row starts on a word
            const uint32_t* q = reinterpret_cast<const uint32_t*>(src + (size_t)r * Wm);
#pragma unroll
            for (int c = 0; c < P / 2; ++c) { const uint32_t v = q[c]; s += (v & 0xFFFFu) + (v >> 16); }
        } else {
#pragma unroll
            for (int c = 0; c < P; ++c) s += src[(size_t)r * Wm + c];
        }
    }
    out[(size_t)blockIdx.y * cells + i] = (uint16_t)((s + P * P / 2) / (P * P));
}

__global__ __launch_bounds__(256) void down_kernel(const uint16_t* __restrict__ in, uint16_t* __restrict__ out, int h, int w, int w2, uint32_t cells,
                                                   FastDiv dw2) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cells) return;
    const uint32_t Y = fdiv_u32(i, dw2), X = i - Y * (uint32_t)w2;
    const uint16_t* src = in + (size_t)blockIdx.y * ((size_t)h * w);
    const int ya = 2 * (int)Y, yb = min(ya + 1, h - 1), xa = 2 * (int)X, xb = min(xa + 1, w - 1);     // 2 Y <= h - 1: Y < (h + 1) / 2
    const uint32_t s = (uint32_t)src[(size_t)ya * w + xa] + src[(size_t)ya * w + xb] + src[(size_t)yb * w + xa] + src[(size_t)yb * w + xb];
    out[(size_t)blockIdx.y * cells + i] = (uint16_t)((s + 2u) >> 2);
}

int al_pyramid(const uint16_t* frames, int N, int Hm, int Wm, int p, int levels, const Level* lv, uint16_t* out, hipStream_t s) {
    const uint32_t cells = (uint32_t)lv[0].h * (uint32_t)lv[0].w;
    const dim3 g0((cells + 255) / 256, N);
    const bool w32 = !((uintptr_t)frames & 3u) && Wm % 2 == 0;
    const FastDiv d0 = make_fastdiv((uint32_t)lv[0].w);
    if (p == 2) {
        if (w32) ELD_LAUNCH((luma_kernel<2, true>), g0, dim3(256), 0, s, frames, out, Hm, Wm, lv[0].w, cells, d0);
        else ELD_LAUNCH((luma_kernel<2, false>), g0, dim3(256), 0, s, frames, out, Hm, Wm, lv[0].w, cells, d0);
    } else {
        if (w32) ELD_LAUNCH((luma_kernel<6, true>), g0, dim3(256), 0, s, frames, out, Hm, Wm, lv[0].w, cells, d0);
        else ELD_LAUNCH((luma_kernel<6, false>), g0, dim3(256), 0, s, frames, out, Hm, Wm, lv[0].w, cells, d0);
    }
    ELD_LAUNCH_CHECK();
    for (int l = 1; l < levels; ++l) {
        const uint32_t c = (uint32_t)lv[l].h * (uint32_t)lv[l].w;
        ELD_LAUNCH(down_kernel, dim3((c + 255) / 256, N), dim3(256), 0, s, (const uint16_t*)(out + lv[l - 1].lum_off), out + lv[l].lum_off, lv[l - 1].h,
                   lv[l - 1].w, lv[l].w, c, make_fastdiv((uint32_t)lv[l].w));
        ELD_LAUNCH_CHECK();
    }
    return 0;
}

// ---- the search ------------------------------------------------------------------------------------------------------------------------------
struct SearchArgs {
    const uint16_t* lum;                         // this level's luma [N][h][w]
    const int16_t* up;                           // the level above's field [N][tyu][txu][2], or null at the coarsest level
    int16_t* disp;                               // [N][ty][tx][2]
    uint32_t* cost;                              // [N][ty][tx], or null
    int ref, h, w, ty, tx, tyu, txu;
    uint32_t tiles, items;                       // ty * tx, (N - 1) * tiles
    FastDiv dtiles, dtx;
};

__device__ __forceinline__ uint32_t sad2(uint32_t a, uint32_t b, uint32_t acc) {
#if __has_builtin(__builtin_amdgcn_sad_u16)
    return __builtin_amdgcn_sad_u16(a, b, acc);                  // |a.lo - b.lo| + |a.hi - b.hi| + acc
#else
    const int lo = (int)(a & 0xFFFFu) - (int)(b & 0xFFFFu), hi = (int)(a >> 16) - (int)(b >> 16);
    return acc + (uint32_t)(lo < 0 ? -lo : lo) + (uint32_t)(hi < 0 ? -hi : hi);
#endif
}

// the minimum over the wave, all 64 lanes active: rotations within each row of 16 lanes (DPP row_ror 8, 4, 2, 1), then one lane of each row
__device__ __forceinline__ int wave_min(int k) {
    k = min(k, __builtin_amdgcn_update_dpp(k, k, 0x128, 0xF, 0xF, false));
    k = min(k, __builtin_amdgcn_update_dpp(k, k, 0x124, 0xF, 0xF, false));
    k = min(k, __builtin_amdgcn_update_dpp(k, k, 0x122, 0xF, 0xF, false));
    k = min(k, __builtin_amdgcn_update_dpp(k, k, 0x121, 0xF, 0xF, false));
    return min(min(__builtin_amdgcn_readlane(k, 0), __builtin_amdgcn_readlane(k, 16)), min(__builtin_amdgcn_readlane(k, 32), __builtin_amdgcn_readlane(k, 48)));
}

__global__ __launch_bounds__(BT) void search_kernel(SearchArgs a) {
    __shared__ uint32_t s_ref[AL_WAVES][AL_T * AL_T / 2];
    __shared__ uint32_t s_alt[AL_WAVES][2][AL_WIN * AL_S];       // [0] the window, [1] the window one pixel to the left
    __shared__ uint32_t s_part[AL_WAVES][AL_TURNS * ELD_WAVE];
    const int wv = threadIdx.x / ELD_WAVE, lane = threadIdx.x % ELD_WAVE;
    const uint32_t item = blockIdx.x * (uint32_t)AL_WAVES + wv;
    const bool live = item < a.items;                            // wave-uniform; every wave reaches the barriers
    int frame = 0, ty = 0, tx = 0, y0 = 0, x0 = 0, sy = 0, sx = 0;
    if (live) {
        const uint32_t fi = fdiv_u32(item, a.dtiles), t = item - fi * a.tiles;
        frame = (int)fi + ((int)fi >= a.ref ? 1 : 0);
        ty = (int)fdiv_u32(t, a.dtx);
        tx = (int)t - ty * a.tx;
        y0 = min(ty * AL_T, a.h - AL_T);
        x0 = min(tx * AL_T, a.w - AL_T);
        if (a.up) {
            const int py = min(((y0 + AL_T / 2) >> 1) / AL_T, a.tyu - 1), px = min(((x0 + AL_T / 2) >> 1) / AL_T, a.txu - 1);
            const int16_t* q = a.up + (((size_t)frame * a.tyu + py) * a.txu + px) * 2;
            sy = 2 * q[0];
            sx = 2 * q[1];
        }
        const size_t hw = (size_t)a.h * a.w;
        const uint16_t* rp = a.lum + (size_t)a.ref * hw;
        const uint16_t* ap = a.lum + (size_t)frame * hw;
        uint16_t* r16 = reinterpret_cast<uint16_t*>(s_ref[wv]);
        uint16_t* a16 = reinterpret_cast<uint16_t*>(s_alt[wv][0]);
        uint16_t* b16 = reinterpret_cast<uint16_t*>(s_alt[wv][1]);
#pragma unroll
        for (int k = 0; k < AL_T * AL_T / ELD_WAVE; ++k) {
            const int i = k * ELD_WAVE + lane, y = i / AL_T, x = i % AL_T;
            r16[i] = rp[(size_t)(y0 + y) * a.w + (x0 + x)];      // the tile lies inside the level
        }
#pragma unroll
        for (int k = 0; k < AL_WIN * AL_WIN / ELD_WAVE; ++k) {
            const int i = k * ELD_WAVE + lane, wy = i / AL_WIN, wx = i % AL_WIN;
            const int gy = min(max(y0 + sy + wy - AL_R, 0), a.h - 1), gx = min(max(x0 + sx + wx - AL_R, 0), a.w - 1);
            const uint16_t v = ap[(size_t)gy * a.w + gx];
            a16[wy * 2 * AL_S + wx] = v;
            if (wx) b16[wy * 2 * AL_S + wx - 1] = v;
        }
    }
    static_assert(AL_T * AL_T % ELD_WAVE == 0 && AL_WIN * AL_WIN % ELD_WAVE == 0, "whole turns of the wave");
    __syncthreads();
    if (live) {
#pragma unroll
        for (int turn = 0; turn < AL_TURNS; ++turn) {
            const int it = turn * ELD_WAVE + lane;
            uint32_t acc = 0;
            if (it < AL_ITEMS) {
                const int c = it >> 1, half = it & 1, vr = c / AL_D, o = c % AL_D;     // the candidate's window row and column, 0..8
                // a row of 16 pixels from column o: words o / 2 .. of the window when o is even, words (o - 1) / 2 .. of its shifted copy when odd
                const uint32_t* al = s_alt[wv][o & 1] + (half * (AL_T / 2) + vr) * AL_S + (o >> 1);
                const uint32_t* rf = s_ref[wv] + half * (AL_T / 2) * (AL_T / 2);
#pragma unroll
                for (int y = 0; y < AL_T / 2; ++y)
#pragma unroll
                    for (int j = 0; j < AL_T / 2; ++j) acc = sad2(rf[y * (AL_T / 2) + j], al[y * AL_S + j], acc);
            }
            s_part[wv][it] = acc;
        }
    }
    __syncthreads();
    if (live) {
        const uint32_t* pt = s_part[wv];
        int key = (int)(((pt[2 * lane] + pt[2 * lane + 1]) << 7) | al_tab.rank[lane]);
        if (lane + ELD_WAVE < AL_NC) {
            const int c = lane + ELD_WAVE;
            key = min(key, (int)(((pt[2 * c] + pt[2 * c + 1]) << 7) | al_tab.rank[c]));
        }
        key = wave_min(key);
        if (lane == 0) {
            const int c = al_tab.cand[key & 127];
            const size_t o = ((size_t)frame * a.ty + ty) * a.tx + tx;
            a.disp[2 * o] = (int16_t)(sy + c / AL_D - AL_R);
            a.disp[2 * o + 1] = (int16_t)(sx + c % AL_D - AL_R);
            if (a.cost) a.cost[o] = (uint32_t)key >> 7;
        }
    }
}

// ---- the aligned stack -----------------------------------------------------------------------------------------------------------------------
constexpr int AS_UNITS = BT * 8;                 // units per workgroup
constexpr int AS_DEPTH = 4;                      // frames whose loads are in flight

struct AlignedArgs {
    const uint16_t* frames;
    const uint32_t* bitmap;
    const int16_t* disp;
    uint16_t* mean;
    uint8_t* kept;
    uint8_t* present;
    unsigned long long* ptc;
    int N, Hm, Wm, G, white, wpr, k2q, min_dev, ty, tx;
    uint32_t hw, upr, units;
    FastDiv dupr;
    int32_t tab[36];                             // cell -> black | (group + 1) << 16
};

__global__ __launch_bounds__(256) void disp_check_kernel(const int16_t* __restrict__ d, uint32_t n, int* __restrict__ flag) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u)
        if (d[i] > AL_MAXD || d[i] < -AL_MAXD) atomicOr(flag, 1);
}

template <int P, int CW>
__global__ __launch_bounds__(BT) void stack_aligned_kernel(AlignedArgs a) {
    static_assert(CW == 1 || CW == 2, "one site or one 32-bit word");
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
    const size_t fstride = (size_t)a.ty * a.tx * 2;              // one frame's field
    Run run[2];
    run_clear(run[0]);
    run_clear(run[1]);

    const uint32_t u0 = blockIdx.x * (uint32_t)AS_UNITS;
    const uint32_t u1 = min(u0 + (uint32_t)AS_UNITS, a.units);
    for (uint32_t u = u0 + threadIdx.x; u < u1; u += BT) {
        const uint32_t y = fdiv_u32(u, a.dupr);
        const uint32_t x0 = (u - y * a.upr) * (uint32_t)CW;
        const int tyi = min((int)(y / (uint32_t)(P * AL_T)), a.ty - 1), txi = min((int)(x0 / (uint32_t)(P * AL_T)), a.tx - 1);
        const int16_t* dp = a.disp + ((size_t)tyi * a.tx + txi) * 2;
        // frame f's sample: where it is, and whether that is inside the frame (CW = 2: x0, p dx and Wm are even, so both sites or neither)
        auto fetch = [&](int f, bool& in) __attribute__((always_inline)) -> uint32_t {
            const int sy = (int)y + P * dp[(size_t)f * fstride], sx = (int)x0 + P * dp[(size_t)f * fstride + 1];
            in = (uint32_t)sy < (uint32_t)a.Hm && (uint32_t)sx < (uint32_t)a.Wm;
            const uint16_t* q = a.frames + (size_t)f * a.hw + (in ? (size_t)sy * a.Wm + sx : (size_t)y * a.Wm + x0);
            if constexpr (CW == 2) return *reinterpret_cast<const uint32_t*>(q);
            else return *q;
        };
        uint32_t S1[CW], mn[CW], mx[CW], M = 0;
        unsigned long long S2[CW];
#pragma unroll
        for (int j = 0; j < CW; ++j) { S1[j] = 0; S2[j] = 0; mn[j] = 65535u; mx[j] = 0; }
        auto take = [&](uint32_t w, bool in) __attribute__((always_inline)) {
            if (in) {
                M += 1;
#pragma unroll
                for (int j = 0; j < CW; ++j) {
                    const uint32_t x = (w >> (16 * j)) & 0xFFFFu;
                    S1[j] += x; S2[j] += (unsigned long long)(x * x);
                    mn[j] = min(mn[j], x); mx[j] = max(mx[j], x);
                }
            }
        };
        int f = 0;
        for (; f + AS_DEPTH <= N; f += AS_DEPTH) {
            uint32_t w[AS_DEPTH];
            bool in[AS_DEPTH];
#pragma unroll
            for (int k = 0; k < AS_DEPTH; ++k) w[k] = fetch(f + k, in[k]);
#pragma unroll
            for (int k = 0; k < AS_DEPTH; ++k) take(w[k], in[k]);
        }
        for (; f < N; ++f) {
            bool in;
            const uint32_t w = fetch(f, in);
            take(w, in);
        }

        // the second look, for the sites whose furthest sample is rejected: the rule over the M present samples
        uint32_t Sk[CW], nk[CW];
        uint32_t need = 0;
#pragma unroll
        for (int j = 0; j < CW; ++j) { Sk[j] = S1[j]; nk[j] = M; }
        if (M >= 4 && a.k2q > 0) {
            const BurstRule rule((int)M, a.k2q, a.min_dev);
#pragma unroll
            for (int j = 0; j < CW; ++j)
                if (rule.rejected(mx[j], S1[j], S2[j]) || rule.rejected(mn[j], S1[j], S2[j])) need |= 1u << j;
            if (need) {
#pragma unroll
                for (int j = 0; j < CW; ++j)
                    if ((need >> j) & 1u) { Sk[j] = 0; nk[j] = 0; }
                for (int f2 = 0; f2 < N; ++f2) {
                    bool in;
                    const uint32_t w = fetch(f2, in);
                    if (in) {
#pragma unroll
                        for (int j = 0; j < CW; ++j)
                            if ((need >> j) & 1u) {
                                const uint32_t x = (w >> (16 * j)) & 0xFFFFu;
                                if (!rule.rejected(x, S1[j], S2[j])) { Sk[j] += x; nk[j] += 1; }
                            }
                    }
                }
            }
        }

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
                if (g >= 0 && !((bad >> j) & 1u) && M == (uint32_t)N && n == (uint32_t)N && (int)mx[j] < white && mn[j] > 0) {
                    const int key = g * PS_NB + bin_of((int)m[j], (int)m[j] - (t & 0xFFFF), white);
                    const unsigned long long v = (unsigned long long)(uint32_t)N * S2[j] - (unsigned long long)S1[j] * S1[j];     // < 2^46
                    run_add(tab, run[CW == 2 ? j : 0], key, S1[j], v);
                }
            }
        }
        const size_t i0 = (size_t)y * a.Wm + x0;
        if constexpr (CW == 2) {
            *reinterpret_cast<uint32_t*>(a.mean + i0) = m[0] | (m[1] << 16);
            if (a.kept) *reinterpret_cast<uint16_t*>(a.kept + i0) = (uint16_t)((nk[0] & 255u) | ((nk[1] & 255u) << 8));
            if (a.present) *reinterpret_cast<uint16_t*>(a.present + i0) = (uint16_t)((M & 255u) | ((M & 255u) << 8));
        } else {
            a.mean[i0] = (uint16_t)m[0];
            if (a.kept) a.kept[i0] = (uint8_t)nk[0];
            if (a.present) a.present[i0] = (uint8_t)M;
        }
    }
    if (!want_ptc) return;                                       // launch-uniform
    run_flush(tab, run[0]);
    run_flush(tab, run[1]);
    __syncthreads();
    ptc_merge(lds, a.ptc, a.G);
}

template <int P, int CW>
int launch_aligned(const AlignedArgs& a, hipStream_t s) {
    ELD_LAUNCH((stack_aligned_kernel<P, CW>), dim3((a.units + AS_UNITS - 1) / AS_UNITS), dim3(BT), 0, s, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

size_t al_round4(size_t bytes) { return (bytes + 3) & ~(size_t)3; }

}  // namespace

extern "C" size_t eld_burst_luma_pyramid_elems(int N, int Hm, int Wm, int p, int levels) {
    Level lv[AL_MAXL];
    size_t lum = 0, dsp = 0;
    return al_geometry(N, Hm, Wm, p, levels, lv, &lum, &dsp) ? lum : 0;
}

extern "C" int eld_burst_luma_pyramid_u16(const uint16_t* frames, int N, int Hm, int Wm, int p, int levels, uint16_t* out, void* stream) {
    Level lv[AL_MAXL];
    size_t lum = 0, dsp = 0;
    if (!al_geometry(N, Hm, Wm, p, levels, lv, &lum, &dsp)) return ELD_EINVAL;
    if (!frames || !out || ((uintptr_t)frames & 1u) || ((uintptr_t)out & 1u)) return ELD_EINVAL;
    return al_pyramid(frames, N, Hm, Wm, p, levels, lv, out, as_stream(stream));
}

extern "C" size_t eld_burst_align_workspace_bytes(int N, int Hm, int Wm, int p, int levels) {
    Level lv[AL_MAXL];
    size_t lum = 0, dsp = 0;
    if (!al_geometry(N, Hm, Wm, p, levels, lv, &lum, &dsp)) return 0;
    return al_round4(lum * 2) + dsp * 2;
}

extern "C" int eld_burst_align_u16(const uint16_t* frames, int N, int Hm, int Wm, int p, int ref, int levels, int16_t* disp, uint32_t* cost, void* ws,
                                   size_t ws_bytes, void* stream) {
    Level lv[AL_MAXL];
    size_t lum = 0, dsp = 0;
    if (!al_geometry(N, Hm, Wm, p, levels, lv, &lum, &dsp) || ref < 0 || ref >= N) return ELD_EINVAL;
    if (!frames || !disp || !ws || ((uintptr_t)frames & 1u) || ((uintptr_t)disp & 1u) || ((uintptr_t)cost & 3u) || ((uintptr_t)ws & 3u)) return ELD_EINVAL;
    if (ws_bytes < al_round4(lum * 2) + dsp * 2) return ELD_EWS;
    hipStream_t s = as_stream(stream);
    uint16_t* pyr = reinterpret_cast<uint16_t*>(ws);
    int16_t* fields = reinterpret_cast<int16_t*>(reinterpret_cast<char*>(ws) + al_round4(lum * 2));
    if (int rc = al_pyramid(frames, N, Hm, Wm, p, levels, lv, pyr, s)) return rc;
    // the reference frame's rows stay zero: the search visits the other frames only
    const size_t t0 = (size_t)lv[0].ty * lv[0].tx;
    if (hipMemsetAsync(disp + (size_t)ref * t0 * 2, 0, t0 * 2 * sizeof(int16_t), s) != hipSuccess) return ELD_EINVAL;
    if (cost && hipMemsetAsync(cost + (size_t)ref * t0, 0, t0 * sizeof(uint32_t), s) != hipSuccess) return ELD_EINVAL;
    for (int l = levels - 1; l >= 0; --l) {
        SearchArgs a;
        a.lum = pyr + lv[l].lum_off;
        a.up = l + 1 < levels ? fields + lv[l + 1].disp_off : nullptr;
        a.disp = l ? fields + lv[l].disp_off : disp;
        a.cost = l ? nullptr : cost;
        a.ref = ref; a.h = lv[l].h; a.w = lv[l].w; a.ty = lv[l].ty; a.tx = lv[l].tx;
        a.tyu = l + 1 < levels ? lv[l + 1].ty : 1; a.txu = l + 1 < levels ? lv[l + 1].tx : 1;
        a.tiles = (uint32_t)lv[l].ty * (uint32_t)lv[l].tx;
        a.items = (uint32_t)(N - 1) * a.tiles;                   // < 256 * 2^31 / (4 * 256) tiles: far below 2^32
        a.dtiles = make_fastdiv(a.tiles);
        a.dtx = make_fastdiv((uint32_t)lv[l].tx);
        ELD_LAUNCH(search_kernel, dim3((a.items + AL_WAVES - 1) / AL_WAVES), dim3(BT), 0, s, a);
        ELD_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" size_t eld_burst_stack_aligned_workspace_bytes(int N, int Hm, int Wm) {
    (void)N; (void)Hm; (void)Wm;
    return 4;                                                    // the flag of the displacement check
}

extern "C" int eld_burst_stack_aligned_u16(const uint16_t* frames, int N, int Hm, int Wm, int p, const int* group, int G, const int32_t* black, int white,
                                           const uint32_t* bitmap, int k2q, int min_dev, const int16_t* disp, int TY0, int TX0, uint16_t* mean,
                                           uint8_t* kept, uint8_t* present, int64_t* ptc, void* ws, size_t ws_bytes, void* stream) {
    Level lv[AL_MAXL];
    size_t lum = 0, dsp = 0;
    if (!al_geometry(N, Hm, Wm, p, 1, lv, &lum, &dsp) || G < 1 || G > 4) return ELD_EINVAL;
    if (TY0 != lv[0].ty || TX0 != lv[0].tx) return ELD_EINVAL;
    if (!cell_groups_ok(p, group, G, black, white)) return ELD_EINVAL;
    if (k2q < 0 || k2q > 256 || min_dev < 0 || min_dev > 65535) return ELD_EINVAL;
    if (!ws || ((uintptr_t)ws & 3u)) return ELD_EINVAL;
    if (ws_bytes < eld_burst_stack_aligned_workspace_bytes(N, Hm, Wm)) return ELD_EWS;
    if (!frames || !mean || !disp || ((uintptr_t)frames & 1u) || ((uintptr_t)mean & 1u) || ((uintptr_t)disp & 1u) || ((uintptr_t)bitmap & 3u) ||
        ((uintptr_t)ptc & 7u))
        return ELD_EINVAL;
    hipStream_t s = as_stream(stream);
    // a displacement beyond +-60 is refused before the stack runs (the field lives on the device: one flag comes back)
    int* flag = reinterpret_cast<int*>(ws);
    int bad = 0;
    const uint32_t nd = (uint32_t)N * (uint32_t)TY0 * (uint32_t)TX0 * 2u;
    if (hipMemsetAsync(flag, 0, sizeof(int), s) != hipSuccess) return ELD_EINVAL;
    ELD_LAUNCH(disp_check_kernel, dim3(min((nd + 255u) / 256u, 1024u)), dim3(256), 0, s, disp, nd, flag);
    ELD_LAUNCH_CHECK();
    if (hipMemcpyAsync(&bad, flag, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) return ELD_EINVAL;
    if (bad) return ELD_EINVAL;
    if (ptc)
        if (int rc = zero_u64(ptc, (size_t)G * PS_NB * 4, s)) return rc;
    AlignedArgs a;
    a.frames = frames; a.bitmap = bitmap; a.disp = disp; a.mean = mean; a.kept = kept; a.present = present; a.ptc = (unsigned long long*)ptc;
    a.N = N; a.Hm = Hm; a.Wm = Wm; a.G = G; a.white = white; a.wpr = bitmap_pitch(Wm); a.k2q = k2q; a.min_dev = min_dev; a.ty = TY0; a.tx = TX0;
    a.hw = (uint32_t)Hm * (uint32_t)Wm;
    pack_cell_tab(a.tab, p, group, black);
    const uintptr_t fm = (uintptr_t)frames | (uintptr_t)mean;
    const int cw = (!(fm & 3u) && !(((uintptr_t)kept | (uintptr_t)present) & 1u) && Wm % 2 == 0) ? 2 : 1;
    a.upr = (uint32_t)(Wm / cw);
    a.units = (uint32_t)Hm * a.upr;
    a.dupr = make_fastdiv(a.upr);
    if (p == 2) return cw == 2 ? launch_aligned<2, 2>(a, s) : launch_aligned<2, 1>(a, s);
    return cw == 2 ? launch_aligned<6, 2>(a, s) : launch_aligned<6, 1>(a, s);
}
