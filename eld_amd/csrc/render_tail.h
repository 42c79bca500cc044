// render_tail.h -- what the full-resolution outputs share behind their resampling (demosaic.hip eld_render_*, warp.hip eld_warp_rgb_f32):
// one site's camera RGB -> the value an output mode writes, the CCM load, the choice of the tail variant and the tail's argument rules.
// Include inside the translation unit's anonymous namespace, as isp_tail.h (which this includes).
#pragma once
#include "isp_tail.h"

// one site's camera RGB -> the values the output modes write: o[c] = linear RGB after the CCM (ELD_RENDER_LINEAR_F32) or the 8-bit code
// as a float (ELD_RENDER_SRGB8: isp_rgb_out writes k / 255; k = rint(255 * (k / 255)) exactly, as eld_amd.denoise recovers it).
// TAIL is a template parameter of the kernels so that the default render (gamma 2.2: the threshold table) does not carry the double-precision
// pow and the CRF search of the other two at every unrolled site: isp_rgb_out is called with constant selectors and folds to one branch.
// Args: the kernel's argument record; inv_gamma, crf_E, crf_f and crf_n are read from it.
constexpr int TAIL_LINEAR = 0, TAIL_TABLE = 1, TAIL_GENERAL = 2;
template <int TAIL, class Args>
__device__ __forceinline__ void site_out(float r, float g, float b, const float (&m)[9], bool has_ccm, const Args& a, double ig,
                                         const unsigned* s_t, float (&o)[3]) {
    if (TAIL == TAIL_LINEAR) {
        if (has_ccm) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = r * m[3 * c];
                v = v + g * m[3 * c + 1];
                v = v + b * m[3 * c + 2];
                o[c] = v;
            }
        } else {
            o[0] = r; o[1] = g; o[2] = b;
        }
    } else {
        float t[3];
        if (TAIL == TAIL_TABLE) isp_rgb_out(r, g, b, m, t, 0, 1, a.inv_gamma, ig, nullptr, nullptr, 0, 1, s_t);
        else isp_rgb_out(r, g, b, m, t, 0, 1, a.inv_gamma, ig, a.crf_E, a.crf_f, a.crf_n, 0, s_t);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = rintf(t[c] * 255.0f);
    }
}

__device__ __forceinline__ void load_ccm(const float* ccms, int n, float (&m)[9]) {
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = ccms ? ccms[9 * n + i] : ((i & 3) == 0 ? 1.f : 0.f);      // identity: r * 1 + g * 0 + b * 0 == r
}

// the tail's own arguments: what every entry point with an out_mode refuses before any launch
inline int tail_args_bad(const void* ccms, int out_mode, float gamma, const float* crf_E, const float* crf_f, int crf_n) {
    if ((uintptr_t)ccms & 3) return 1;
    if (out_mode != ELD_RENDER_SRGB8 && out_mode != ELD_RENDER_LINEAR_F32) return 1;
    if (!(gamma > 0.f)) return 1;
    if (crf_n < 0 || crf_n == 1) return 1;
    if (crf_n >= 2 && (!crf_E || !crf_f || ((uintptr_t)crf_E & 3) || ((uintptr_t)crf_f & 3))) return 1;
    return 0;
}
inline int render_tail(int out_mode, float gamma, int crf_n) {
    return out_mode == ELD_RENDER_LINEAR_F32 ? TAIL_LINEAR : (crf_n == 0 && gamma == 2.2f) ? TAIL_TABLE : TAIL_GENERAL;      // the table: as eld_isp_process picks it
}
