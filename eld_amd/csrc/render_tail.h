// render_tail.h -- what the full-resolution outputs share behind their resampling (the four renders of demosaic*.hip, warp.hip eld_warp_rgb_f32):
// the tail's argument record and rules, one site's camera RGB -> the value an output mode writes, the CCM load, the gamma table's staging, and
// the choice of the tail variant with its dispatch.  What only the four demosaic renders share is render_args.h.
// Include inside the translation unit's anonymous namespace, as isp_tail.h (which this includes).
#pragma once
#include "isp_tail.h"

// the tail's part of every kernel argument record
struct TailArgs {
    const float* ccms;                 // NULL: no matrix (linear mode: the resampled camera RGB; sRGB mode: the identity)
    float inv_gamma;
    const float* crf_E;
    const float* crf_f;
    int crf_n;
};
inline TailArgs tail_args(const float* ccms, float gamma, const float* crf_E, const float* crf_f, int crf_n) {
    return TailArgs{ccms, (float)(1.0 / (double)gamma), crf_E, crf_f, crf_n};
}

// one site's camera RGB -> the values the output modes write: o[c] = linear RGB after the CCM (ELD_RENDER_LINEAR_F32) or the 8-bit code
// as a float (ELD_RENDER_SRGB8: isp_rgb_out writes k / 255; k = rint(255 * (k / 255)) exactly, as eld_amd.denoise recovers it).
// TAIL is a template parameter of the kernels so that the default render (gamma 2.2: the threshold table) does not carry the double-precision
// pow and the CRF search of the other two at every unrolled site: isp_rgb_out is called with constant selectors and folds to one branch.
constexpr int TAIL_LINEAR = 0, TAIL_TABLE = 1, TAIL_GENERAL = 2;
template <int TAIL>
__device__ __forceinline__ void site_out(float r, float g, float b, const float (&m)[9], const TailArgs& a, double ig, const unsigned* s_t,
                                         float (&o)[3]) {
    if (TAIL == TAIL_LINEAR) {
        if (a.ccms != nullptr) {
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

// the 256-entry threshold table of gamma 2.2 into LDS, by a workgroup of THREADS lanes; the caller's next barrier publishes it
template <int TAIL, int THREADS>
__device__ __forceinline__ void stage_gamma_table(unsigned* s_t) {
    if (TAIL != TAIL_TABLE) return;
    if (THREADS == 256) s_t[threadIdx.x] = ELD_GAMMA22_T[threadIdx.x];
    else
        for (int i = threadIdx.x; i < 256; i += THREADS) s_t[i] = ELD_GAMMA22_T[i];
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

// the run-time tail as a template argument: f(TailTag<TAIL>{}) for the one TAIL that `tail` is; f's int is the entry point's return value
template <int TAIL>
struct TailTag { static constexpr int value = TAIL; };
template <class F>
inline int with_tail(int tail, F&& f) {
    if (tail == TAIL_LINEAR) return f(TailTag<TAIL_LINEAR>{});
    if (tail == TAIL_TABLE) return f(TailTag<TAIL_TABLE>{});
    return f(TailTag<TAIL_GENERAL>{});
}
