// mosaic_dev.h -- the device counterpart of eld_amd/mosaic.py: what the raw-frame kernels share when they walk a uint16 mosaic [Hm,Wm] with a
// CFA cell of period 2 (Bayer) or 6 (X-Trans).  The cell phase of a row or column, the per-cell table in LDS, 8 / 2 / 1 codes of a row as
// 32-bit words, the defect bitmap's word, the wave butterfly sum, the zero fill of 64-bit sums
// and the host-side checks of the per-cell arguments.  The packed-plane map of noise.hip, pack_raw.hip and demosaic.hip is xtrans.h's.
#pragma once
#include "common.h"

// ---- the cell phase -----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t mod6(uint32_t v) { return v - 6u * (__umulhi(v, 0xAAAAAAABu) >> 2); }

template <int P>
__device__ __forceinline__ uint32_t cell_phase(uint32_t v) { return P == 2 ? (v & 1u) : mod6(v); }

// ---- the cell table in LDS ----------------------------------------------------------------------------------------------------------------------
// A lane owns up to 8 adjacent columns from x0 on, and x0 % P is 0 or 1 (P == 2) or 0..5 (P == 6; 0, 2 or 4 for an even x0): with 12 entries per
// row phase, entry k = cell (r, k % P), the lane's cells are the CONSECUTIVE entries x0 % P + j, j < 8 -- one pointer, compile-time offsets.
constexpr int CELL_ROW = 12;

template <int P, typename T>
__device__ __forceinline__ void fill_cell_rows(T* s, const T* cell) {       // s[P * CELL_ROW] in LDS; the caller's barrier follows
    if (threadIdx.x < P * CELL_ROW) s[threadIdx.x] = cell[(threadIdx.x / CELL_ROW) * P + (threadIdx.x % CELL_ROW) % P];
}

// the lane's row of the table: row y, first column x0 (x0 % P + the lane's columns - 1 < CELL_ROW)
template <int P, typename T>
__device__ __forceinline__ const T* cell_row(const T* s, uint32_t y, uint32_t x0) { return s + cell_phase<P>(y) * CELL_ROW + cell_phase<P>(x0); }

// ---- codes of a row as 32-bit words -------------------------------------------------------------------------------------------------------------
// CW = 8: one 16-byte load (p 16-byte aligned); 2: one 32-bit word (p 4-byte aligned); 1: one code
template <int CW>
__device__ __forceinline__ void load_codes(const uint16_t* __restrict__ p, uint32_t (&w)[(CW + 1) / 2]) {
    if constexpr (CW == 8) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else if constexpr (CW == 2) {
        w[0] = *reinterpret_cast<const uint32_t*>(p);
    } else {
        w[0] = *p;
    }
}

// 8 codes from column x0 of a row of Wm (even) codes.  VEC: one 16-byte load; otherwise one word per column pair that lies inside the row
// (the others read as 0)
template <bool VEC>
__device__ __forceinline__ void load_codes8(const uint16_t* p, int x0, int Wm, uint32_t (&w)[4]) {
    if (VEC) {
        const uint4 q = *reinterpret_cast<const uint4*>(p);
        w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = x0 + 2 * k < Wm ? *reinterpret_cast<const uint32_t*>(p + 2 * k) : 0u;
    }
}

__device__ __forceinline__ uint32_t code_of(const uint32_t* w, int j) { return (w[j / 2] >> (16 * (j & 1))) & 0xFFFFu; }

// ---- the defect bitmap (pack_bitmap's layout: bit x & 31 of word [y][x >> 5], wpr = bitmap_pitch(Wm) words per row) -----------------------------
// The row's word shifted to x0: bit j is site (y, x0 + j).  A lane's CW columns start at a multiple of CW and CW divides 32, so its CW bits
// lie in this one word.  The bitmap is not null here: a caller whose bitmap is optional asks first.
template <typename I>
__device__ __forceinline__ uint32_t defect_bits(const uint32_t* bitmap, int wpr, I y, I x0) {
    return bitmap[(size_t)y * wpr + (x0 >> 5)] >> (x0 & 31);
}

template <typename I>
__device__ __forceinline__ bool defect_bit(const uint32_t* bitmap, int wpr, I y, I x) { return defect_bits(bitmap, wpr, y, x) & 1u; }

// ---- the sum over the 64 lanes: an xor butterfly from 32 down to 1, the same order of additions on every run --------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = ELD_WAVE / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, ELD_WAVE);
    return v;
}

// ---- the 8-column passes over a frame pool (shading.hip, flatfield.hip) -----------------------------------------------------------------------
constexpr int ROW_NPX = 8;                       // columns per lane
constexpr int POOL_U = 4;                        // frames in flight per lane

// ---- zero fill of 64-bit sums that a later kernel of the same call adds to ------------------------------------------------------------------------
// T: a 64-bit integer type (templates, so that only the files that zero something carry the kernel)
template <typename T>
__global__ __launch_bounds__(256) void zero_u64_kernel(T* __restrict__ p, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0;
}

// n words from p on the stream; 0 or the launch error
template <typename T>
int zero_u64(T* p, size_t n, hipStream_t s) {
    static_assert(sizeof(T) == 8, "64-bit sums");
    if (n == 0) return 0;
    const size_t nb = (n + 255) / 256;
    ELD_LAUNCH(zero_u64_kernel<T>, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, s, p, n);
    ELD_LAUNCH_CHECK();
    return 0;
}

// ---- host: the per-cell arguments ---------------------------------------------------------------------------------------------------------------
// words per row of the defect bitmap
static inline int bitmap_pitch(int Wm) { return (Wm + 31) / 32; }

// group[k] in [-1, G) and black[k] a code for the p * p cells (p is 2 or 6: the caller has checked), white in [1, 65536]
static inline bool cell_groups_ok(int p, const int* group, int G, const int32_t* black, int white) {
    if (!group || !black || white < 1 || white > 65536) return false;
    for (int k = 0; k < p * p; ++k)
        if (group[k] < -1 || group[k] >= G || black[k] < 0 || black[k] > 65535) return false;
    return true;
}

// cell -> black | (group + 1) << 16; the entries beyond p * p are 0
static inline void pack_cell_tab(int32_t (&tab)[36], int p, const int* group, const int32_t* black) {
    for (int k = 0; k < 36; ++k) tab[k] = k < p * p ? (black[k] | ((group[k] + 1) << 16)) : 0;
}
