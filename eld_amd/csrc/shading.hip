// shading.hip -- dark shading: per-site offset maps offset(y, x, iso) = a(y, x) + b(y, x) * (iso - x0), fitted to the bias frames of all
// sessions and subtracted from sensor codes (eld_amd/shading.py).
//
//   eld_shading_fit_u16                bias frames of S sessions in a frame pool -> two float32 planes a, b [Hm,Wm]
//   eld_shading_apply_u16              uint16 codes [N,Hm,Wm] -> clamp(u - rint(a + b t), 0, 65535)
// The input stage that subtracts the maps in float32 (eld_pack_raw_*_u16_shaded) is in pack_raw.hip.
// Every output is a function of its own site: no atomics, no cross-lane sums, and the order of the floating-point operations is the one the
// header states, so two calls give the same bits and tests/shading_ref.py restates them operation for operation.  The library is built
// with -ffp-contract=off; the pragma below says so for this file whatever the flags.
//
// Fit and apply: a lane owns 8 consecutive columns of one row (x0 = a multiple of 8): one 16-byte load of codes where the row pitch and
// the frame's start allow it, else one 32-bit word per column pair (Wm is even, frames start at even elements).  The 8 bits of the defect
// bitmap lie in one word.  The fit walks the frames of a session four at a time (four loads in flight per lane), keeps eight uint32 sums
// for the session in turn and folds them into the float64 pair (A, B) before the next session starts.  Grids are sized from eld_num_cus().
#include "mosaic_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int SH_T = 256;                        // threads per workgroup
constexpr int SH_MAX_S = 16;                     // sessions per call (they travel as kernel arguments)
constexpr int SH_MAX_COUNT = 65536;              // frames per session: 65536 * 65535 < 2^32 keeps the uint32 sums exact

struct FitArgs {
    const uint16_t* pool;
    size_t pool_elems;
    const EldPoolFrame* frames;
    const uint32_t* bitmap;
    float* out_a;
    float* out_b;
    int Hm, Wm, wpr, lpr, S, vec_in, vec_out;    // lpr = lanes per row = ceil(Wm / 8); vec_in: row pitch and pool base allow 16-byte loads
    int first[SH_MAX_S], count[SH_MAX_S];
    double alpha[SH_MAX_S], beta[SH_MAX_S];
    int32_t cen[36];
};

struct ApplyArgs {
    const uint16_t* in;
    uint16_t* out;
    const float* a;
    const float* b;
    const uint32_t* bitmap;
    float t;
    int N, Hm, Wm, wpr, lpr;
};

template <int P>
__global__ __launch_bounds__(SH_T) void shading_fit_kernel(FitArgs a) {
    __shared__ int32_t s_cen[P * CELL_ROW];
    fill_cell_rows<P>(s_cen, a.cen);
    __syncthreads();
    const uint32_t units = (uint32_t)a.Hm * (uint32_t)a.lpr;             // Hm * Wm < 2^31
    const size_t fsz = (size_t)a.Hm * a.Wm;
    for (uint32_t i = blockIdx.x * SH_T + threadIdx.x; i < units; i += gridDim.x * SH_T) {
        const int y = (int)(i / (uint32_t)a.lpr), x0 = (int)(i - (uint32_t)y * (uint32_t)a.lpr) * ROW_NPX;
        const size_t site = (size_t)y * a.Wm + x0;
        const int32_t* cenl = s_cen + (y % P) * CELL_ROW + (P == 2 ? 0 : x0 % P);
        double A[ROW_NPX], B[ROW_NPX];
#pragma unroll
        for (int j = 0; j < ROW_NPX; ++j) A[j] = B[j] = 0.0;
        for (int s = 0; s < a.S; ++s) {
            const int first = a.first[s], cnt = a.count[s];
            uint32_t T[ROW_NPX];
#pragma unroll
            for (int j = 0; j < ROW_NPX; ++j) T[j] = 0u;
            for (int f0 = 0; f0 < cnt; f0 += POOL_U) {
                const uint16_t* src[POOL_U];
                bool ok[POOL_U], wide = a.vec_in;
#pragma unroll
                for (int u = 0; u < POOL_U; ++u) {                       // launch-uniform: the table entry decides, not the lane
                    ok[u] = f0 + u < cnt;
                    src[u] = a.pool;
                    if (ok[u]) {
                        const EldPoolFrame e = a.frames[first + f0 + u];
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
                for (int u = 0; u < POOL_U; ++u)
#pragma unroll
                    for (int j = 0; j < ROW_NPX; ++j) T[j] += code_of(w[u], j);
            }
            const double c = (double)cnt, al = a.alpha[s], be = a.beta[s];
#pragma unroll
            for (int j = 0; j < ROW_NPX; ++j) {
                const double ys = ((double)T[j] - c * (double)cenl[j]) / c;      // product and difference exact: one rounding
                A[j] = A[j] + al * ys;
                B[j] = B[j] + be * ys;
            }
        }
        const uint32_t bad = a.bitmap ? defect_bits(a.bitmap, a.wpr, y, x0) : 0u;
        float oa[ROW_NPX], ob[ROW_NPX];
#pragma unroll
        for (int j = 0; j < ROW_NPX; ++j) {
            const bool flagged = (bad >> j) & 1u;
            oa[j] = flagged ? 0.f : (float)A[j];
            ob[j] = flagged ? 0.f : (float)B[j];
        }
        if (a.vec_out) {
            float4* pa = reinterpret_cast<float4*>(a.out_a + site);
            float4* pb = reinterpret_cast<float4*>(a.out_b + site);
            pa[0] = make_float4(oa[0], oa[1], oa[2], oa[3]); pa[1] = make_float4(oa[4], oa[5], oa[6], oa[7]);
            pb[0] = make_float4(ob[0], ob[1], ob[2], ob[3]); pb[1] = make_float4(ob[4], ob[5], ob[6], ob[7]);
        } else {
#pragma unroll
            for (int j = 0; j < ROW_NPX; ++j)
                if (x0 + j < a.Wm) { a.out_a[site + j] = oa[j]; a.out_b[site + j] = ob[j]; }
        }
    }
}

// the integer the apply pass subtracts: rint(a + b t), ties to even.  Kept inside +-65536 before the conversion: with a code in [0, 65535] the
// clamped difference is the same, and the conversion stays defined for any map.
__device__ __forceinline__ int shading_step(float a, float b, float t) {
    const float ds = a + b * t;
    return (int)fminf(fmaxf(rintf(ds), -65536.f), 65536.f);
}

// in and out may be the same buffer: a lane reads its own 8 codes of a frame before it writes them, and touches no others
template <bool VEC>
__global__ __launch_bounds__(SH_T) void shading_apply_kernel(ApplyArgs a) {
    const uint32_t units = (uint32_t)a.Hm * (uint32_t)a.lpr;
    const size_t fsz = (size_t)a.Hm * a.Wm;
    for (uint32_t i = blockIdx.x * SH_T + threadIdx.x; i < units; i += gridDim.x * SH_T) {
        const int y = (int)(i / (uint32_t)a.lpr), x0 = (int)(i - (uint32_t)y * (uint32_t)a.lpr) * ROW_NPX;
        const size_t site = (size_t)y * a.Wm + x0;
        float fa[ROW_NPX], fb[ROW_NPX];
        if (VEC) {
            const float4 a0 = reinterpret_cast<const float4*>(a.a + site)[0], a1 = reinterpret_cast<const float4*>(a.a + site)[1];
            const float4 b0 = reinterpret_cast<const float4*>(a.b + site)[0], b1 = reinterpret_cast<const float4*>(a.b + site)[1];
            fa[0] = a0.x; fa[1] = a0.y; fa[2] = a0.z; fa[3] = a0.w; fa[4] = a1.x; fa[5] = a1.y; fa[6] = a1.z; fa[7] = a1.w;
            fb[0] = b0.x; fb[1] = b0.y; fb[2] = b0.z; fb[3] = b0.w; fb[4] = b1.x; fb[5] = b1.y; fb[6] = b1.z; fb[7] = b1.w;
        } else {
#pragma unroll
            for (int j = 0; j < ROW_NPX; ++j) {
                const bool in = x0 + j < a.Wm;
                fa[j] = in ? a.a[site + j] : 0.f;
                fb[j] = in ? a.b[site + j] : 0.f;
            }
        }
        const uint32_t bad = a.bitmap ? defect_bits(a.bitmap, a.wpr, y, x0) : 0u;
        int r[ROW_NPX];
#pragma unroll
        for (int j = 0; j < ROW_NPX; ++j) r[j] = ((bad >> j) & 1u) ? 0 : shading_step(fa[j], fb[j], a.t);   // a flagged site passes through
        for (int n = 0; n < a.N; ++n) {
            uint32_t w[4], o[4];
            load_codes8<VEC>(a.in + (size_t)n * fsz + site, x0, a.Wm, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int lo = min(max((int)code_of(w, 2 * k) - r[2 * k], 0), 65535);
                const int hi = min(max((int)code_of(w, 2 * k + 1) - r[2 * k + 1], 0), 65535);
                o[k] = (uint32_t)lo | ((uint32_t)hi << 16);
            }
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

}  // namespace

extern "C" int eld_shading_fit_u16(const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int Hm, int Wm, const int32_t* sessions,
                                   int S, const double* alpha, const double* beta, const int32_t* centre, int period, const uint32_t* bitmap,
                                   float* out_a, float* out_b, void* stream) {
    if ((period != 2 && period != 6) || bad_shape(Hm, Wm) || F < 0 || S < 1 || S > SH_MAX_S) return ELD_EINVAL;
    if (!sessions || !alpha || !beta || !centre) return ELD_EINVAL;
    for (int s = 0; s < S; ++s) {
        const int first = sessions[2 * s], count = sessions[2 * s + 1];
        if (count < 1 || count > SH_MAX_COUNT || first < 0 || first > F - count) return ELD_EINVAL;
    }
    for (int k = 0; k < period * period; ++k)
        if (centre[k] < 0 || centre[k] > 65535) return ELD_EINVAL;
    if (((uintptr_t)pool & 3u) || ((uintptr_t)bitmap & 3u) || ((uintptr_t)frames & 7u) || ((uintptr_t)out_a & 3u) || ((uintptr_t)out_b & 3u)) return ELD_EINVAL;
    if (Hm == 0 || Wm == 0) return 0;
    if (!pool || !frames || !out_a || !out_b) return ELD_EINVAL;
    FitArgs a;
    a.pool = pool; a.pool_elems = pool_elems; a.frames = frames; a.bitmap = bitmap; a.out_a = out_a; a.out_b = out_b;
    a.Hm = Hm; a.Wm = Wm; a.wpr = bitmap_pitch(Wm); a.lpr = (Wm + ROW_NPX - 1) / ROW_NPX; a.S = S;
    a.vec_in = Wm % ROW_NPX == 0 && !((uintptr_t)pool & 15u);
    a.vec_out = Wm % ROW_NPX == 0 && !(((uintptr_t)out_a | (uintptr_t)out_b) & 15u);
    for (int s = 0; s < SH_MAX_S; ++s) {
        a.first[s] = s < S ? sessions[2 * s] : 0; a.count[s] = s < S ? sessions[2 * s + 1] : 0;
        a.alpha[s] = s < S ? alpha[s] : 0.0; a.beta[s] = s < S ? beta[s] : 0.0;
    }
    for (int k = 0; k < 36; ++k) a.cen[k] = k < period * period ? centre[k] : 0;
    const dim3 grid(stride_grid((uint32_t)Hm * (uint32_t)a.lpr, SH_T));
    if (period == 2) ELD_LAUNCH(shading_fit_kernel<2>, grid, dim3(SH_T), 0, as_stream(stream), a);
    else ELD_LAUNCH(shading_fit_kernel<6>, grid, dim3(SH_T), 0, as_stream(stream), a);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_shading_apply_u16(const uint16_t* in, uint16_t* out, int N, int Hm, int Wm, const float* ma, const float* mb, float t,
                                     const uint32_t* bitmap, void* stream) {
    if (bad_shape(Hm, Wm) || N < 0) return ELD_EINVAL;
    if (((uintptr_t)in & 3u) || ((uintptr_t)out & 3u) || ((uintptr_t)bitmap & 3u) || ((uintptr_t)ma & 3u) || ((uintptr_t)mb & 3u)) return ELD_EINVAL;
    if (N == 0 || Hm == 0 || Wm == 0) return 0;
    if (!in || !out || !ma || !mb) return ELD_EINVAL;
    ApplyArgs a;
    a.in = in; a.out = out; a.a = ma; a.b = mb; a.bitmap = bitmap; a.t = t;
    a.N = N; a.Hm = Hm; a.Wm = Wm; a.wpr = bitmap_pitch(Wm); a.lpr = (Wm + ROW_NPX - 1) / ROW_NPX;
    // Wm % 8 == 0 makes a frame a multiple of 16 bytes: every frame of an aligned stack is aligned
    const bool vec = Wm % ROW_NPX == 0 && !(((uintptr_t)in | (uintptr_t)out | (uintptr_t)ma | (uintptr_t)mb) & 15u);
    const dim3 grid(stride_grid((uint32_t)Hm * (uint32_t)a.lpr, SH_T));
    if (vec) ELD_LAUNCH(shading_apply_kernel<true>, grid, dim3(SH_T), 0, as_stream(stream), a);
    else ELD_LAUNCH(shading_apply_kernel<false>, grid, dim3(SH_T), 0, as_stream(stream), a);
    ELD_LAUNCH_CHECK();
    return 0;
}
