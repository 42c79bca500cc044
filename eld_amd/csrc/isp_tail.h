// isp_tail.h -- the tail every sRGB render shares (eval.hip eld_isp_process / eld_isp_process_xtrans, demosaic.hip eld_render_*):
// linear camera RGB of one pixel -> 3x3 CCM (j ascending) -> clamp -> gamma compression / camera response -> truncating 8-bit quantiser
// (util/process.py:22-39, 71-83).  Include inside the translation unit's anonymous namespace (the table below has internal linkage there).
#pragma once
#include "gamma22_table.h"
__device__ __forceinline__ float isp_quant(float v) {
    int q = (int)(v * 255.0f);                                     // .int(): truncation toward zero
    q = q < 0 ? 0 : (q > 255 ? 255 : q);
    return (float)q / 255.0f;
}

// the tail both ISP kernels share: linear RGB of one pixel -> CCM -> clamp -> gamma / CRF -> 8-bit code / 255 into dst[c * hw + i]
__device__ __forceinline__ void isp_rgb_out(float r, float g, float b, const float (&m)[9], float* __restrict__ dst, size_t i, size_t hw,
                                            float inv_gamma, double ig, const float* __restrict__ crf_E, const float* __restrict__ crf_f,
                                            int crf_n, int gtab, const unsigned* s_t) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = r * m[3 * c];
        v = v + g * m[3 * c + 1];
        v = v + b * m[3 * c + 2];
        v = fminf(fmaxf(v, 0.f), 1.f);
        float o;
        if (crf_n > 0) {
            int lo = 0, hi = crf_n;                              // searchsorted(E, v, 'left') - 1, clamped to [0, n-2]
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (crf_E[mid] < v) lo = mid + 1; else hi = mid; }
            int ind = lo - 1;
            ind = ind < 0 ? 0 : (ind > crf_n - 2 ? crf_n - 2 : ind);
            const float slope = (crf_f[ind + 1] - crf_f[ind]) / (crf_E[ind + 1] - crf_E[ind]);
            o = crf_f[ind] + slope * (v - crf_E[ind]);
        } else if (gtab) {                                      // exact: code = #{c : bits(max(v,1e-8)) >= T[c]}, found from a hardware-pow guess
            const float vm = fmaxf(v, 1e-8f);
            const unsigned vb = __float_as_uint(vm);
            int q = (int)(__builtin_amdgcn_exp2f(__builtin_amdgcn_logf(vm) * inv_gamma) * 255.0f);
            q = q < 0 ? 0 : (q > 255 ? 255 : q);
            while (q < 255 && vb >= s_t[q + 1]) ++q;
            while (q > 0 && vb < s_t[q]) --q;
            dst[c * hw + i] = (float)q / 255.0f;
            continue;
        } else {
            o = (float)pow((double)fmaxf(v, 1e-8f), ig);
        }
        dst[c * hw + i] = isp_quant(o);
    }
}
