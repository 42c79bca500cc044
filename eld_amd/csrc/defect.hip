// defect.hip -- defective-pixel maps on uint16 sensor mosaics: the deviation of a stack sum from the lower median of
// its same-colour neighbours, the threshold into a bitmap, and the repair of flagged sites.  All integer: "equal" means equal bits.
//
//   class of (y, x)      pattern[(y % p) * p + x % p], p = 2 (Bayer: the four channel codes) or 6 (X-Trans: R 0, G 1, B 2)
//   N(y, x)              the sites != (y, x) inside the image with |dy| <= R, |dx| <= R and the class of (y, x); Bayer R = 2 (the offsets
//                        of +-2: 8 sites inside, 3 in a corner), X-Trans R = XT_DR below, derived from xtrans.h at compile time
//   lower median         of m >= 1 integers: rank (m - 1) / 2 in ascending order
//   S = sum_f u_f        exact in uint32 for F <= 4096;  D = int32(S - lower median of S over N)
//   flags                hot: D > T_hi; cold: -D > T_lo; bit x & 31 of word [y][x >> 5], ceil(Wm / 32) words per row, unused bits zero
//   repair               a clear site is copied; a flagged site becomes the lower median of u over the UNFLAGGED sites of N
//
// Repair in place (in == out) gives the bits of repair out of place: the gather reads unflagged sites only, and an unflagged site is
// written back with the code it held, so it does not matter whether a neighbour has been written yet.  A flagged site without an
// unflagged neighbour keeps its code (the Python layer refuses such a map before it reaches the device).
//
// No atomics, no LDS, no scratch; every site is computed by one lane from the same operands in the same order whatever the launch shape.
#include "mosaic_dev.h"
#include "xtrans.h"

namespace {

constexpr uint32_t PAD = 0xffffffffu;          // sorts after every stack sum (S <= 4096 * 65535 < 2^28) and every code

// ---- X-Trans tables, derived from the colour map of the cell (xtrans.h: XT.colour[6 * row + col]) ---------------------------------------------------
constexpr int XT_MAXR = 3;                     // a (2R + 1)^2 window mask fits 64 bits up to R = 3

// same-class taps of phase (py, px) in the (2R + 1)^2 window, centre excluded: bit = raster index (dy + R) * (2R + 1) + dx + R
constexpr uint64_t xt_same_mask(int py, int px, int R) {
    uint64_t m = 0;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx)
            if ((dy || dx) && XT.colour[6 * ((py + dy + 12) % 6) + (px + dx + 12) % 6] == XT.colour[6 * py + px])
                m |= 1ull << ((dy + R) * (2 * R + 1) + dx + R);
    return m;
}
// A window reaches a sites up / left and b sites down / right of its centre (0 <= a, b <= R).  Which (phase, a, b) occur along one axis
// of a mosaic of side >= 6 that starts at phase 0: a < R only at coordinate a (phase a); a < R and b < R only when the side a + b + 1 >= 6.
constexpr bool xt_axis_occurs(int phase, int a, int b, int R) {
    if (a < R && phase != a) return false;
    if (a < R && b < R && a + b + 1 < 6) return false;
    return true;
}
constexpr int popc64(uint64_t m) { int n = 0; for (; m; m &= m - 1) ++n; return n; }
constexpr uint64_t xt_rect_mask(int a, int b, int l, int r, int R) {
    uint64_t m = 0;
    for (int dy = -a; dy <= b; ++dy)
        for (int dx = -l; dx <= r; ++dx) m |= 1ull << ((dy + R) * (2 * R + 1) + dx + R);
    return m;
}
// fewest neighbours over every phase and every clipped window that occurs
constexpr int xt_min_neighbours(int R) {
    int best = 1 << 30;
    for (int a = 0; a <= R; ++a)
        for (int b = 0; b <= R; ++b)
            for (int l = 0; l <= R; ++l)
                for (int r = 0; r <= R; ++r) {
                    const uint64_t rect = xt_rect_mask(a, b, l, r, R);
                    for (int py = 0; py < 6; ++py) {
                        if (!xt_axis_occurs(py, a, b, R)) continue;
                        for (int px = 0; px < 6; ++px) {
                            if (!xt_axis_occurs(px, l, r, R)) continue;
                            const int n = popc64(xt_same_mask(py, px, R) & rect);
                            if (n < best) best = n;
                        }
                    }
                }
    return best;
}
constexpr int xt_defect_radius() {
    for (int R = 1; R <= XT_MAXR; ++R)
        if (xt_min_neighbours(R) >= 3) return R;
    return 0;
}
constexpr int XT_DR = xt_defect_radius();
static_assert(XT_DR >= 1 && XT_DR <= XT_MAXR, "no window radius up to 3 gives every X-Trans site 3 same-colour neighbours");
static_assert(xt_min_neighbours(XT_DR) >= 3 && (XT_DR == 1 || xt_min_neighbours(XT_DR - 1) < 3), "XT_DR is the smallest such radius");
constexpr int XT_DW = 2 * XT_DR + 1;

struct XtTaps { uint64_t mask[6][6]; int count[6][6]; signed char dy[6][6][XT_DW * XT_DW], dx[6][6][XT_DW * XT_DW]; int max_count; };
constexpr XtTaps make_xt_taps() {
    XtTaps t{};
    for (int py = 0; py < 6; ++py)
        for (int px = 0; px < 6; ++px) {
            t.mask[py][px] = xt_same_mask(py, px, XT_DR);
            int k = 0;
            for (int i = 0; i < XT_DW * XT_DW; ++i)
                if ((t.mask[py][px] >> i) & 1) {
                    t.dy[py][px][k] = (signed char)(i / XT_DW - XT_DR);
                    t.dx[py][px][k] = (signed char)(i % XT_DW - XT_DR);
                    ++k;
                }
            t.count[py][px] = k;
            if (k > t.max_count) t.max_count = k;
        }
    return t;
}
constexpr XtTaps XT_TAPS = make_xt_taps();

// ---- pass 1: the stack sum, two sites per lane -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void defect_sum_kernel(const uint32_t* __restrict__ u2, int F, size_t words, uint2* __restrict__ S2) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) {
        uint32_t lo = 0, hi = 0;
        for (int f = 0; f < F; ++f) {
            const uint32_t w = u2[(size_t)f * words + i];
            lo += w & 0xffffu;
            hi += w >> 16;
        }
        S2[i] = make_uint2(lo, hi);
    }
}

// ---- pass 2, Bayer: the lower median of the (up to) 8 sites at offsets of +-2 ------------------------------------------------------------
__device__ __forceinline__ void cx(uint32_t& a, uint32_t& b) {
    const uint32_t lo = min(a, b), hi = max(a, b);
    a = lo; b = hi;
}
// 19 compare-exchanges, 6 layers: sorts 8 values ascending
__device__ __forceinline__ void sort8(uint32_t* v) {
    cx(v[0], v[2]); cx(v[1], v[3]); cx(v[4], v[6]); cx(v[5], v[7]);
    cx(v[0], v[4]); cx(v[1], v[5]); cx(v[2], v[6]); cx(v[3], v[7]);
    cx(v[0], v[1]); cx(v[2], v[3]); cx(v[4], v[5]); cx(v[6], v[7]);
    cx(v[2], v[4]); cx(v[3], v[5]);
    cx(v[1], v[4]); cx(v[3], v[6]);
    cx(v[1], v[2]); cx(v[3], v[4]); cx(v[5], v[6]);
}

__global__ __launch_bounds__(256) void defect_dev_bayer_kernel(const uint32_t* __restrict__ S, int Hm, int Wm, int32_t* __restrict__ D) {
    for (int y = blockIdx.y; y < Hm; y += gridDim.y)
        for (int x = blockIdx.x * 256 + threadIdx.x; x < Wm; x += gridDim.x * 256) {
            uint32_t v[8];
            int m = 0, k = 0;
#pragma unroll
            for (int dy = -2; dy <= 2; dy += 2)
#pragma unroll
                for (int dx = -2; dx <= 2; dx += 2) {
                    if (!dy && !dx) continue;
                    const int yy = y + dy, xx = x + dx;
                    const bool ok = (unsigned)yy < (unsigned)Hm && (unsigned)xx < (unsigned)Wm;
                    const uint32_t s = S[ok ? (size_t)yy * Wm + xx : (size_t)y * Wm + x];        // never outside the plane
                    v[k++] = ok ? s : PAD;
                    m += ok;
                }
            sort8(v);                                   // the pads sort last: the first m entries are the neighbours, ascending
            const int r = (m - 1) >> 1;                 // m >= 1 needs a side >= 3; m == 0 (a 2 x 2 frame): the site's own sum
            const uint32_t own = S[(size_t)y * Wm + x];
            const uint32_t med = m == 0 ? own : r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : v[3];
            D[(size_t)y * Wm + x] = (int32_t)own - (int32_t)med;
        }
}

// ---- pass 2, X-Trans: compile-time tap list per phase; a lane owns the six sites of one row of a 6x6 cell ------------------------------
// rank (m - 1) / 2 by counting: the rank of candidate i is the number of candidates below it, ties broken by index
template <int K>
__device__ __forceinline__ uint32_t lower_median_padded(const uint32_t* v, int m) {
    const int target = (m - 1) >> 1;
    uint32_t med = PAD;
#pragma unroll
    for (int i = 0; i < K; ++i) {
        int r = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) r += (v[j] < v[i]) || (v[j] == v[i] && j < i);
        med = r == target ? v[i] : med;
    }
    return med;
}

template <int PY, int PX>
__device__ __forceinline__ void xt_dev_site(const uint32_t* __restrict__ S, int Hm, int Wm, int y, int x, int32_t* __restrict__ D) {
    constexpr int K = XT_TAPS.count[PY][PX];
    uint32_t v[K];
    int m = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int yy = y + XT_TAPS.dy[PY][PX][k], xx = x + XT_TAPS.dx[PY][PX][k];
        const bool ok = (unsigned)yy < (unsigned)Hm && (unsigned)xx < (unsigned)Wm;
        const uint32_t s = S[ok ? (size_t)yy * Wm + xx : (size_t)y * Wm + x];
        v[k] = ok ? s : PAD;
        m += ok;
    }
    const uint32_t own = S[(size_t)y * Wm + x];
    const uint32_t med = m == 0 ? own : lower_median_padded<K>(v, m);
    D[(size_t)y * Wm + x] = (int32_t)own - (int32_t)med;
}

template <int PY>
__device__ __forceinline__ void xt_dev_row(const uint32_t* __restrict__ S, int Hm, int Wm, int y, int x0, int32_t* __restrict__ D) {
    if (x0 + 0 < Wm) xt_dev_site<PY, 0>(S, Hm, Wm, y, x0 + 0, D);
    if (x0 + 1 < Wm) xt_dev_site<PY, 1>(S, Hm, Wm, y, x0 + 1, D);
    if (x0 + 2 < Wm) xt_dev_site<PY, 2>(S, Hm, Wm, y, x0 + 2, D);
    if (x0 + 3 < Wm) xt_dev_site<PY, 3>(S, Hm, Wm, y, x0 + 3, D);
    if (x0 + 4 < Wm) xt_dev_site<PY, 4>(S, Hm, Wm, y, x0 + 4, D);
    if (x0 + 5 < Wm) xt_dev_site<PY, 5>(S, Hm, Wm, y, x0 + 5, D);
}

__global__ __launch_bounds__(256) void defect_dev_xtrans_kernel(const uint32_t* __restrict__ S, int Hm, int Wm, int32_t* __restrict__ D) {
    const int cells = (Wm + 5) / 6;
    for (int y = blockIdx.y; y < Hm; y += gridDim.y) {
        const int py = y % 6;                                   // uniform over the block
        for (int c = blockIdx.x * 256 + threadIdx.x; c < cells; c += gridDim.x * 256) {
            const int x0 = 6 * c;
            switch (py) {
                case 0: xt_dev_row<0>(S, Hm, Wm, y, x0, D); break;
                case 1: xt_dev_row<1>(S, Hm, Wm, y, x0, D); break;
                case 2: xt_dev_row<2>(S, Hm, Wm, y, x0, D); break;
                case 3: xt_dev_row<3>(S, Hm, Wm, y, x0, D); break;
                case 4: xt_dev_row<4>(S, Hm, Wm, y, x0, D); break;
                default: xt_dev_row<5>(S, Hm, Wm, y, x0, D); break;
            }
        }
    }
}

// ---- flags: one ballot per wave, 64 bits = two words, written by lane 0 -------------------------------------------------------------------
__global__ __launch_bounds__(256) void defect_flags_kernel(const int32_t* __restrict__ D, int Hm, int Wm, int32_t T_hi, int32_t T_lo, int pitch,
                                                           uint32_t* __restrict__ bitmap) {
    const int spans = (Wm + 255) / 256;                         // the trip counts are uniform over the block: every lane reaches the ballot
    for (int y = blockIdx.y; y < Hm; y += gridDim.y)
        for (int sp = blockIdx.x; sp < spans; sp += gridDim.x) {
            const int x = sp * 256 + threadIdx.x;
            bool flag = false;
            if (x < Wm) {
                const int32_t d = D[(size_t)y * Wm + x];
                flag = d > T_hi || (int64_t)(-(int64_t)d) > (int64_t)T_lo;
            }
            const unsigned long long bits = __ballot(flag);     // lanes beyond the row vote 0: the pad bits stay zero
            if ((threadIdx.x & 63) == 0) {
                const int w = x >> 5;                           // x is a multiple of 64 here
                if (w < pitch) bitmap[(size_t)y * pitch + w] = (uint32_t)bits;
                if (w + 1 < pitch) bitmap[(size_t)y * pitch + w + 1] = (uint32_t)(bits >> 32);
            }
        }
}

// ---- repair -----------------------------------------------------------------------------------------------------------------------------------
struct ClassTable { uint64_t lo, hi; int p, R, step; };        // 2 bits per cell of the p x p pattern; window radius; 2 for Bayer (offsets of +-2 only)
__device__ __forceinline__ int class_of(const ClassTable& t, int y, int x) {
    const int k = (y % t.p) * t.p + x % t.p;
    return (int)((k < 32 ? t.lo >> (2 * k) : t.hi >> (2 * (k - 32))) & 3u);
}

// the rare path: lower median of the unflagged same-class sites of the window, by rank counting over at most |N| candidates
__device__ __noinline__ uint32_t repair_gather(const uint16_t* f, const uint32_t* __restrict__ bitmap, int pitch, int Hm, int Wm, ClassTable t,
                                               int y, int x) {
    const int cls = class_of(t, y, x), W = 2 * t.R + 1;
    uint64_t cand = 0;                                          // bit = raster index of the tap in the window
    for (int dy = -t.R; dy <= t.R; dy += t.step)
        for (int dx = -t.R; dx <= t.R; dx += t.step) {
            const int yy = y + dy, xx = x + dx;
            if ((!dy && !dx) || (unsigned)yy >= (unsigned)Hm || (unsigned)xx >= (unsigned)Wm) continue;
            if (class_of(t, yy, xx) != cls || defect_bit(bitmap, pitch, yy, xx)) continue;
            cand |= 1ull << ((dy + t.R) * W + dx + t.R);
        }
    const uint32_t own = f[(size_t)y * Wm + x];
    if (!cand) return own;
    const int target = (__popcll(cand) - 1) >> 1;
    uint32_t med = own;
    for (uint64_t a = cand; a; a &= a - 1) {
        const int i = __ffsll((unsigned long long)a) - 1;
        const uint32_t vi = f[(size_t)(y + i / W - t.R) * Wm + (x + i % W - t.R)];
        int r = 0;
        for (uint64_t b = cand; b; b &= b - 1) {
            const int j = __ffsll((unsigned long long)b) - 1;
            const uint32_t vj = f[(size_t)(y + j / W - t.R) * Wm + (x + j % W - t.R)];
            r += (vj < vi) || (vj == vi && j < i);
        }
        if (r == target) med = vi;
    }
    return med;
}

// A lane owns the 8 sites of one bitmap byte.  Per row (uniform over the block): 16-byte loads and stores when both row pointers allow
// them, 4-byte ones when they are 4-byte aligned, 2-byte ones otherwise and for the last, partial group of a row.
__global__ __launch_bounds__(256) void defect_repair_kernel(const uint16_t* in, uint16_t* out, int N, int Hm, int Wm, ClassTable t,
                                                            const uint32_t* __restrict__ bitmap, int pitch) {
    const int groups = (Wm + 7) / 8;
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(bitmap);
    const bool same = in == out;
    for (int row = blockIdx.y; row < N * Hm; row += gridDim.y) {
        const int y = row % Hm;
        const uint16_t* frame = in + (size_t)(row - y) * Wm;    // the frame's first site: the gather reads the INPUT frame
        const uint16_t* src = in + (size_t)row * Wm;
        uint16_t* dst = out + (size_t)row * Wm;
        const uintptr_t al = (uintptr_t)src | (uintptr_t)dst;
        const int mode = (al & 15) == 0 ? 2 : (al & 3) == 0 ? 1 : 0;
        for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
            const int x0 = 8 * g, nv = min(8, Wm - x0);
            const uint32_t b = bytes[(size_t)y * pitch * 4 + g];
            if (same && !b) continue;                           // in place: nothing to change in this group
            uint32_t c[8];
            const int m = nv == 8 ? mode : 0;
            if (m == 2) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + x0);
                c[0] = v.x & 0xffffu; c[1] = v.x >> 16; c[2] = v.y & 0xffffu; c[3] = v.y >> 16;
                c[4] = v.z & 0xffffu; c[5] = v.z >> 16; c[6] = v.w & 0xffffu; c[7] = v.w >> 16;
            } else if (m == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t w = reinterpret_cast<const uint32_t*>(src + x0)[q];
                    c[2 * q] = w & 0xffffu; c[2 * q + 1] = w >> 16;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q) c[q] = q < nv ? src[x0 + q] : 0u;
            }
            if (b) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (((b >> q) & 1u) && q < nv) c[q] = repair_gather(frame, bitmap, pitch, Hm, Wm, t, y, x0 + q);
            }
            if (m == 2) {
                *reinterpret_cast<uint4*>(dst + x0) = make_uint4(c[0] | (c[1] << 16), c[2] | (c[3] << 16), c[4] | (c[5] << 16), c[6] | (c[7] << 16));
            } else if (m == 1) {
#pragma unroll
                for (int q = 0; q < 4; ++q) reinterpret_cast<uint32_t*>(dst + x0)[q] = c[2 * q] | (c[2 * q + 1] << 16);
            } else {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (q < nv) dst[x0 + q] = (uint16_t)c[q];
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------
// pattern: p * p class codes.  Bayer: a permutation of 0..3.  X-Trans: rawpy's colour codes (1 and 3 both G) of the cell xtrans.h packs.
bool class_table(int period, const int* pattern, ClassTable* t) {
    if (!pattern || (period != 2 && period != 6)) return false;
    t->lo = t->hi = 0; t->p = period;
    if (period == 2) {
        if (!bayer_permutation(pattern)) return false;
        for (int i = 0; i < 4; ++i) t->lo |= (uint64_t)pattern[i] << (2 * i);
        t->R = 2; t->step = 2;
        return true;
    }
    for (int i = 0; i < 36; ++i) {
        const int k = pattern[i];
        if (k < 0 || k > 3) return false;
        const int col = k == 3 ? 1 : k;
        if (col != XT.colour[i]) return false;
        (i < 32 ? t->lo : t->hi) |= (uint64_t)col << (2 * (i < 32 ? i : i - 32));
    }
    t->R = XT_DR; t->step = 1;
    return true;
}

bool sides_ok(int Hm, int Wm, int period) {
    if (Hm < 1 || Wm < 1 || (size_t)Hm * (size_t)Wm > (size_t)0x7fffffff) return false;
    return period == 2 || (Hm >= 6 && Wm >= 6);
}

unsigned rows_grid(int rows) { return (unsigned)min(rows, 65535); }

}  // namespace

extern "C" size_t eld_defect_deviation_workspace_bytes(int Hm, int Wm) {
    if (Hm < 1 || Wm < 1) return 0;
    return (size_t)Hm * (size_t)Wm * sizeof(uint32_t);
}

extern "C" int eld_defect_deviation(const uint16_t* stack, int F, int Hm, int Wm, int period, const int* pattern, int32_t* D, void* ws,
                                    size_t ws_bytes, void* stream) {
    ClassTable t;
    if (!stack || !D || !ws || F < 1 || F > 4096 || !class_table(period, pattern, &t) || !sides_ok(Hm, Wm, period) || (Wm & 1)) return ELD_EINVAL;
    if (((uintptr_t)stack & 3) || ((uintptr_t)D & 3) || ((uintptr_t)ws & 7)) return ELD_EINVAL;
    if (ws_bytes < eld_defect_deviation_workspace_bytes(Hm, Wm)) return ELD_EWS;
    const size_t words = (size_t)Hm * Wm / 2;
    uint32_t* S = static_cast<uint32_t*>(ws);
    ELD_LAUNCH(defect_sum_kernel, dim3((unsigned)min((words + 255) / 256, (size_t)8192)), dim3(256), 0, as_stream(stream),
               reinterpret_cast<const uint32_t*>(stack), F, words, reinterpret_cast<uint2*>(ws));
    ELD_LAUNCH_CHECK();
    if (period == 2) {
        ELD_LAUNCH(defect_dev_bayer_kernel, dim3((unsigned)min((Wm + 255) / 256, 64), rows_grid(Hm)), dim3(256), 0, as_stream(stream), S, Hm, Wm, D);
    } else {
        const int cells = (Wm + 5) / 6;
        ELD_LAUNCH(defect_dev_xtrans_kernel, dim3((unsigned)min((cells + 255) / 256, 64), rows_grid(Hm)), dim3(256), 0, as_stream(stream), S, Hm, Wm, D);
    }
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_defect_flags(const int32_t* D, int Hm, int Wm, int32_t T_hi, int32_t T_lo, uint32_t* bitmap, void* stream) {
    if (!D || !bitmap || !sides_ok(Hm, Wm, 2) || ((uintptr_t)D & 3) || ((uintptr_t)bitmap & 3)) return ELD_EINVAL;
    const int pitch = bitmap_pitch(Wm);
    ELD_LAUNCH(defect_flags_kernel, dim3((unsigned)min((Wm + 255) / 256, 64), rows_grid(Hm)), dim3(256), 0, as_stream(stream), D, Hm, Wm, T_hi, T_lo,
               pitch, bitmap);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_defect_repair_u16(const uint16_t* in, uint16_t* out, int N, int Hm, int Wm, int period, const int* pattern, const uint32_t* bitmap,
                                     void* stream) {
    ClassTable t;
    if (!in || !out || !bitmap || N < 1 || !class_table(period, pattern, &t) || !sides_ok(Hm, Wm, period)) return ELD_EINVAL;
    if ((size_t)N * (size_t)Hm > (size_t)0x7fffffff) return ELD_EINVAL;
    if (((uintptr_t)in & 1) || ((uintptr_t)out & 1) || ((uintptr_t)bitmap & 3)) return ELD_EINVAL;
    if (in != out) {                                            // partial overlap would read sites another lane has already replaced
        const uintptr_t a = (uintptr_t)in, b = (uintptr_t)out, n = (uintptr_t)N * Hm * Wm * 2;
        if (a < b + n && b < a + n) return ELD_EINVAL;
    }
    const int groups = (Wm + 7) / 8, pitch = bitmap_pitch(Wm);
    ELD_LAUNCH(defect_repair_kernel, dim3((unsigned)min((groups + 255) / 256, 64), rows_grid(N * Hm)), dim3(256), 0, as_stream(stream), in, out, N, Hm,
               Wm, t, bitmap, pitch);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_debug_xtrans_defect_tables(int* out, int n) {
    if (!out || n < 1 + 36 * 4) return ELD_EINVAL;
    out[0] = XT_DR;
    for (int py = 0; py < 6; ++py)
        for (int px = 0; px < 6; ++px) {
            int* o = out + 1 + 4 * (6 * py + px);
            o[0] = XT.colour[6 * py + px];
            o[1] = XT_TAPS.count[py][px];
            o[2] = (int)(uint32_t)XT_TAPS.mask[py][px];
            o[3] = (int)(uint32_t)(XT_TAPS.mask[py][px] >> 32);
        }
    return 0;
}
