// pack_raw.hip -- the raw input stage of inference and evaluation: uint16 sensor mosaic -> packed, normalised planes, one pass
// (pack_raw_bayer / the X-Trans branch of the dataset pack, dataset/sid_dataset.py:172-239, and the evaluation input stage, :398-409).
// Per site m of plane k, float32 throughout as NumPy evaluates it (uint16 -> float32 exact, one rounding per op, true division):
//   b = float(u) - black[k]
//   b = b - (a[m] + b_map[m] * t)        SHADE: the dark-shading map (shading.hip fits it)
//   v = (b * gain[m]) / denom[k]         FLAT: the PRNU plane (flatfield.hip fits it); otherwise v = b / denom[k], denom = white - black
//   o = min(max(v, 0), 1)
//   o = max(min(o * ratio[n], 1), 0)     with ratios: np.maximum(np.minimum(o * np.float32(ratio), 1), 0)
// One kernel per CFA, templated on the planes it reads and on the ratio step; an instantiation without a plane neither loads it nor spends an
// operation on it.  RATIO is compile time as well: decided in the kernel from ratios != nullptr, the same bits came out 14 % (Bayer, no planes,
// no ratios) and 4 % (Bayer, no planes, ratios) slower than with the step compiled in or out, on 8 frames of 2848 x 4256.  Eight entry points
// state their preconditions and share one launcher per CFA.  The library is built with -ffp-contract=off; the pragma says so for this file.
// 2 B read + 4 B written per site, plus 4 B per plane read.
#include <utility>

#include "common.h"
#include "xtrans.h"

#pragma clang fp contract(off)

namespace {

struct PackRawArgs { int oy[4], ox[4]; float black[4], denom[4]; };     // per colour code k: its position in the 2x2 cell and its constants

// the per-site planes and the per-frame ratios; a pointer the entry point does not have is nullptr
struct PackRawPlanes { const float* ratios; const float* ma; const float* mb; float t; const float* gain; };

__device__ __forceinline__ float apply_ratio(float v, float ratio) { return fmaxf(fminf(v * ratio, 1.f), 0.f); }

// Bayer: out[k][y][x] from im[2y + oy_k][2x + ox_k], k = R, G1, B, G2 = raw_pattern codes 0..3.  A lane handles two horizontally adjacent
// packed positions of all four planes: per mosaic row one 8-byte read of codes (the row pitch is a multiple of 4 sites) and one 16-byte read of
// each plane (VMAP: the planes are 16-byte aligned as well).  Sites beyond the row read as code 0, map 0, gain 1 and are not written.
template <bool SHADE, bool FLAT, bool VMAP, bool RATIO>
__global__ __launch_bounds__(256) void pack_raw_bayer_kernel(const uint16_t* __restrict__ im, float* __restrict__ out, int h, int w, PackRawArgs p,
                                                             const float* __restrict__ ratios, const float* __restrict__ ma,
                                                             const float* __restrict__ mb, float t, const float* __restrict__ gain) {
    const int n = blockIdx.y;
    const float ratio = RATIO ? ratios[n] : 1.f;
    const size_t hw = (size_t)h * w, W2 = 2 * (size_t)w;
    const uint16_t* src = im + (size_t)n * 4 * hw;
    float* dst = out + (size_t)n * 4 * hw;
    const int wp = (w + 1) / 2;                                     // position pairs per packed row
    const size_t total = (size_t)h * wp;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int y = (int)(i / wp), x = 2 * (int)(i - (size_t)y * wp);
        const bool two = x + 1 < w;
        uint16_t q[2][4];                                           // q[row][col] of the 2 x 4 mosaic block
        float ds[2][4], gn[2][4];                                   // a + b t and the gain of the same sites
        const size_t m0 = (size_t)(2 * y) * W2 + 2 * x;
        const uint16_t* r0 = src + m0;
        if (two && ((W2 & 3) == 0)) {
            const ushort4 a = *reinterpret_cast<const ushort4*>(r0), b = *reinterpret_cast<const ushort4*>(r0 + W2);
            q[0][0] = a.x; q[0][1] = a.y; q[0][2] = a.z; q[0][3] = a.w; q[1][0] = b.x; q[1][1] = b.y; q[1][2] = b.z; q[1][3] = b.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) { const bool ok = c < 2 || two; q[0][c] = ok ? r0[c] : 0; q[1][c] = ok ? r0[W2 + c] : 0; }
        }
        if (VMAP && two) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                if (FLAT) {
                    const float4 vg = *reinterpret_cast<const float4*>(gain + m0 + r * W2);
                    gn[r][0] = vg.x; gn[r][1] = vg.y; gn[r][2] = vg.z; gn[r][3] = vg.w;
                }
                if (SHADE) {
                    const float4 va = *reinterpret_cast<const float4*>(ma + m0 + r * W2), vb = *reinterpret_cast<const float4*>(mb + m0 + r * W2);
                    ds[r][0] = va.x + vb.x * t; ds[r][1] = va.y + vb.y * t; ds[r][2] = va.z + vb.z * t; ds[r][3] = va.w + vb.w * t;
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool ok = c < 2 || two;
                    if (FLAT) gn[r][c] = ok ? gain[m0 + r * W2 + c] : 1.f;
                    if (SHADE) ds[r][c] = ok ? ma[m0 + r * W2 + c] + mb[m0 + r * W2 + c] * t : 0.f;
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float b0 = (float)q[p.oy[k]][p.ox[k]] - p.black[k], b1 = (float)q[p.oy[k]][2 + p.ox[k]] - p.black[k];
            if (SHADE) { b0 = b0 - ds[p.oy[k]][p.ox[k]]; b1 = b1 - ds[p.oy[k]][2 + p.ox[k]]; }
            if (FLAT) { b0 = b0 * gn[p.oy[k]][p.ox[k]]; b1 = b1 * gn[p.oy[k]][2 + p.ox[k]]; }
            const float v0 = b0 / p.denom[k], v1 = b1 / p.denom[k];
            float* o = dst + (size_t)k * hw + (size_t)y * w + x;
            float o0 = fminf(fmaxf(v0, 0.f), 1.f), o1 = fminf(fmaxf(v1, 0.f), 1.f);
            if (RATIO) { o0 = apply_ratio(o0, ratio); o1 = apply_ratio(o1, ratio); }
            o[0] = o0;
            if (two) o[1] = o1;
        }
    }
}

// X-Trans: out[c][i][j] from im[row][col], (row, col) the index map of xtrans.h (as xtrans_kernel of noise.hip); one black level.  One thread per
// packed element: the packed side is the coalesced one.
template <bool SHADE, bool FLAT, bool RATIO>
__global__ __launch_bounds__(256) void pack_raw_xtrans_kernel(const uint16_t* __restrict__ im, float* __restrict__ out, int h, int w, int Hm, int Wm,
                                                              float black, float denom, const float* __restrict__ ratios,
                                                              const float* __restrict__ ma, const float* __restrict__ mb, float t,
                                                              const float* __restrict__ gain) {
    const int n = blockIdx.y;
    const float ratio = RATIO ? ratios[n] : 1.f;
    const size_t hw = (size_t)h * w, total = 9 * hw;
    const uint16_t* s = im + (size_t)n * Hm * Wm;
    float* d = out + (size_t)n * total;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
        const int c = (int)(e / hw);
        const int r = (int)(e - (size_t)c * hw);
        const int i = r / w, j = r - i * w;
        int row, col;
        if (c < 5) { row = 6 * (i >> 1) + XT_RC[c][i & 1][j & 1][0]; col = 6 * (j >> 1) + XT_RC[c][i & 1][j & 1][1]; }
        else { row = 3 * i + XT_RC3[c - 5][0]; col = 3 * j + XT_RC3[c - 5][1]; }
        const size_t m = (size_t)row * Wm + col;
        float b = (float)s[m] - black;
        if (SHADE) b = b - (ma[m] + mb[m] * t);
        if (FLAT) b = b * gain[m];
        const float v = b / denom;
        const float o = fminf(fmaxf(v, 0.f), 1.f);
        d[e] = RATIO ? apply_ratio(o, ratio) : o;
    }
}

// the instantiation whose template arguments are the bits of `bits` (SHADE the highest, RATIO the lowest)
template <size_t... I>
auto bayer_kernel(unsigned bits, std::index_sequence<I...>) {
    static constexpr decltype(&pack_raw_bayer_kernel<false, false, false, false>) table[] = {
        pack_raw_bayer_kernel<(I & 8) != 0, (I & 4) != 0, (I & 2) != 0, (I & 1) != 0>...};
    return table[bits];
}

template <size_t... I>
auto xtrans_kernel(unsigned bits, std::index_sequence<I...>) {
    static constexpr decltype(&pack_raw_xtrans_kernel<false, false, false>) table[] = {
        pack_raw_xtrans_kernel<(I & 4) != 0, (I & 2) != 0, (I & 1) != 0>...};
    return table[bits];
}

bool misaligned4(const void* p) { return ((uintptr_t)p & 3u) != 0; }

dim3 pack_grid(size_t total, int N) { return dim3((unsigned)min((total + 255) / 256, (size_t)4096), N); }

// The shared part of the Bayer entry points.  SHADE = there is a map, FLAT = there is a gain plane; the caller has checked what it requires of them.
int pack_raw_bayer_launch(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern, const float* black_level,
                          float white_point, const PackRawPlanes& pl, void* stream) {
    if (N < 0 || h < 0 || w < 0 || !raw_pattern || !black_level) return ELD_EINVAL;
    if (N == 0 || h == 0 || w == 0) return 0;
    if (!mosaic || !packed || !bayer_permutation(raw_pattern)) return ELD_EINVAL;
    PackRawArgs p;
    for (int i = 0; i < 4; ++i) { p.oy[raw_pattern[i]] = i >> 1; p.ox[raw_pattern[i]] = i & 1; }   // np.where(raw_pattern == k)
    for (int k = 0; k < 4; ++k) { p.black[k] = black_level[k]; p.denom[k] = white_point - black_level[k]; }
    const bool shade = pl.ma != nullptr, flat = pl.gain != nullptr;
    // a lane's first site of a row is (2 y') * 2w + 4 x': a multiple of 4 sites when 2w is; N frames share the planes
    const bool vmap = (shade || flat) && (2 * (size_t)w) % 4 == 0 && !(((uintptr_t)pl.ma | (uintptr_t)pl.mb | (uintptr_t)pl.gain) & 15u);
    const auto kern = bayer_kernel(shade << 3 | flat << 2 | vmap << 1 | (pl.ratios != nullptr), std::make_index_sequence<16>{});
    ELD_LAUNCH(kern, pack_grid((size_t)h * ((w + 1) / 2), N), dim3(256), 0, as_stream(stream), mosaic, packed, h, w, p, pl.ratios, pl.ma, pl.mb, pl.t,
               pl.gain);
    ELD_LAUNCH_CHECK();
    return 0;
}

// uint16 mosaic [N, Hm, Wm] -> packed float32 [N, 9, 2*(Hm/6), 2*(Wm/6)] (sides truncated to whole 6x6 cells, as eld_pack_xtrans)
int pack_raw_xtrans_launch(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point, const PackRawPlanes& pl,
                           void* stream) {
    if (N < 0 || Hm < 0 || Wm < 0 || !(white_point > black_level)) return ELD_EINVAL;
    const int h = 2 * (Hm / 6), w = 2 * (Wm / 6);
    const size_t total = (size_t)9 * h * w;
    if (N == 0 || total == 0) return 0;
    if (!mosaic || !packed) return ELD_EINVAL;
    const auto kern = xtrans_kernel((pl.ma != nullptr) << 2 | (pl.gain != nullptr) << 1 | (pl.ratios != nullptr), std::make_index_sequence<8>{});
    ELD_LAUNCH(kern, pack_grid(total, N), dim3(256), 0, as_stream(stream), mosaic, packed, h, w, Hm, Wm, black_level, white_point - black_level, pl.ratios,
               pl.ma, pl.mb, pl.t, pl.gain);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

// Each entry point states what it requires beyond the launcher's checks.  A null pointer is required only where there is work (Bayer: N, h, w > 0;
// X-Trans: N > 0 and at least one whole cell); a misaligned plane is refused even where there is none.
extern "C" int eld_pack_raw_bayer_u16(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern, const float* black_level,
                                      float white_point, void* stream) {
    return pack_raw_bayer_launch(mosaic, packed, N, h, w, raw_pattern, black_level, white_point, {nullptr, nullptr, nullptr, 0.f, nullptr}, stream);
}

extern "C" int eld_pack_raw_bayer_u16_gain(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern, const float* black_level,
                                           float white_point, const float* ratios, void* stream) {
    if (N > 0 && h > 0 && w > 0 && !ratios) return ELD_EINVAL;
    return pack_raw_bayer_launch(mosaic, packed, N, h, w, raw_pattern, black_level, white_point, {ratios, nullptr, nullptr, 0.f, nullptr}, stream);
}

extern "C" int eld_pack_raw_bayer_u16_shaded(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern,
                                             const float* black_level, float white_point, const float* ratios, const float* ma, const float* mb,
                                             float t, void* stream) {
    if (misaligned4(ma) || misaligned4(mb)) return ELD_EINVAL;
    if (N > 0 && h > 0 && w > 0 && (!ratios || !ma || !mb)) return ELD_EINVAL;
    return pack_raw_bayer_launch(mosaic, packed, N, h, w, raw_pattern, black_level, white_point, {ratios, ma, mb, t, nullptr}, stream);
}

extern "C" int eld_pack_raw_bayer_u16_flat(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern,
                                           const float* black_level, float white_point, const float* ratios, const float* ma, const float* mb,
                                           float t, const float* gain, void* stream) {
    if (misaligned4(ma) || misaligned4(mb) || misaligned4(gain) || (ma == nullptr) != (mb == nullptr)) return ELD_EINVAL;
    if (N > 0 && h > 0 && w > 0 && !gain) return ELD_EINVAL;
    return pack_raw_bayer_launch(mosaic, packed, N, h, w, raw_pattern, black_level, white_point, {ratios, ma, mb, t, gain}, stream);
}

extern "C" int eld_pack_raw_xtrans_u16(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point, void* stream) {
    return pack_raw_xtrans_launch(mosaic, packed, N, Hm, Wm, black_level, white_point, {nullptr, nullptr, nullptr, 0.f, nullptr}, stream);
}

extern "C" int eld_pack_raw_xtrans_u16_gain(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point,
                                            const float* ratios, void* stream) {
    if (N > 0 && Hm >= 6 && Wm >= 6 && !ratios) return ELD_EINVAL;
    return pack_raw_xtrans_launch(mosaic, packed, N, Hm, Wm, black_level, white_point, {ratios, nullptr, nullptr, 0.f, nullptr}, stream);
}

extern "C" int eld_pack_raw_xtrans_u16_shaded(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point,
                                              const float* ratios, const float* ma, const float* mb, float t, void* stream) {
    if (misaligned4(ma) || misaligned4(mb)) return ELD_EINVAL;
    if (N > 0 && Hm >= 6 && Wm >= 6 && (!ratios || !ma || !mb)) return ELD_EINVAL;
    return pack_raw_xtrans_launch(mosaic, packed, N, Hm, Wm, black_level, white_point, {ratios, ma, mb, t, nullptr}, stream);
}

extern "C" int eld_pack_raw_xtrans_u16_flat(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point,
                                            const float* ratios, const float* ma, const float* mb, float t, const float* gain, void* stream) {
    if (misaligned4(ma) || misaligned4(mb) || misaligned4(gain) || (ma == nullptr) != (mb == nullptr)) return ELD_EINVAL;
    if (N > 0 && Hm >= 6 && Wm >= 6 && !gain) return ELD_EINVAL;
    return pack_raw_xtrans_launch(mosaic, packed, N, Hm, Wm, black_level, white_point, {ratios, ma, mb, t, gain}, stream);
}
