// warp.hip -- DNG WarpRectilinear on demosaiced camera RGB: every output pixel of every plane is a 4 x 4 Catmull-Rom
// sample of its plane at the coordinate the lens polynomial gives, and the three samples of a pixel go through the renders' tail
// (render_tail.h: CCM, gamma table / pow / CRF, quantiser).  The per-pixel arithmetic is warp_dev.h, which a host compiler takes too; the
// kernel here is the tiling around it.
//
// One workgroup of 512 lanes owns a tile of 32 rows x 64 columns of output pixels; a wave owns 4 consecutive rows, a lane one column of them
// (256 lanes with 8 rows each need 160 to 256 registers and are slower: DESIGN.md sec. 30).
//   1. every lane evaluates the map of its 4 pixels, once per coefficient set (one set: once for the three planes);
//   2. the workgroup reduces the minimum and maximum of i0 and j0 per set over the tile's pixels: the exact bounding box of what the tile
//      samples, whatever the polynomial does inside the tile;
//   3. if the three planes' boxes with their -1 / +2 halo fit the LDS budget they are staged with coalesced row loads, the edge clamp applied
//      on the way in (the box is kept in unclamped coordinates: LDS holds the replicated edge), and the 16 taps of a sample are LDS reads;
//      otherwise the taps are read from global memory through the clamp (warp_tap).  Both paths feed the same values to the same sum.
// Reading the taps from global memory is the faster of the two on the MI355X (sec. 30: 414 against 582 us on 24 MP), so it is the default:
// without an LDS budget the kernel is instantiated without steps 2 and 3.
// The record travels as a kernel argument (184 bytes); its fields are wave-uniform, so they are scalar loads.
#include "common.h"
#include "warp_dev.h"

namespace {
#include "render_tail.h"

constexpr int WT = 512;                          // lanes of a workgroup
constexpr int WTX = 64, WTY = 32;                // the tile
constexpr int WWAVES = WT / ELD_WAVE;            // 8
constexpr int WROWS = WTY / WWAVES;              // rows of a lane
constexpr int WARP_DEFAULT_LDS = 0;              // lds_bytes < 0: no staging (measured faster); 40 KiB would hold the widest boxes of sec. 30's lenses
constexpr int WARP_MAX_LDS = 64 << 10;
static_assert(WTX == ELD_WAVE, "a wave spans the tile's columns: a row of a wave's loads and stores is one line of 64 pixels");

struct WarpArgs {
    const float* rgb;
    void* out;
    TailArgs t;
    int Hm, Wm;
    int lds_floats;                              // the staging budget in floats (0: the direct path everywhere)
    EldWarp w;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// STAGE: the launch has an LDS budget (steps 2 and 3); without one no box is reduced and every tile reads global memory
template <int TAIL, int NSETS, bool STAGE>
__global__ __launch_bounds__(WT) void warp_kernel(WarpArgs a) {
    extern __shared__ __align__(16) float warp_lds[];
    __shared__ int s_box[WWAVES][NSETS][4];          // per wave and set: min i0, max i0, min j0, max j0 of its pixels inside the image
    __shared__ unsigned s_t[256];
    const int tid = threadIdx.x, lane = tid & (ELD_WAVE - 1), wave = tid / ELD_WAVE;
    stage_gamma_table<TAIL, WT>(s_t);
    const int n = blockIdx.z, Hm = a.Hm, Wm = a.Wm;
    const int x = blockIdx.x * WTX + lane, y0 = blockIdx.y * WTY + wave * WROWS;
    const bool x_in = x < Wm;

    // 1. the map
    WarpSite site[NSETS][WROWS];
    int box[NSETS][4];
#pragma unroll
    for (int s = 0; s < NSETS; ++s) {
        box[s][0] = box[s][2] = 0x7fffffff;
        box[s][1] = box[s][3] = -0x7fffffff - 1;
#pragma unroll
        for (int r = 0; r < WROWS; ++r) {
            site[s][r] = warp_site(a.w.k[s], a.w.cxp, a.w.cyp, a.w.m, a.w.m2, x, y0 + r, Hm, Wm);
            if (STAGE && x_in && y0 + r < Hm) {
                box[s][0] = min(box[s][0], site[s][r].i0); box[s][1] = max(box[s][1], site[s][r].i0);
                box[s][2] = min(box[s][2], site[s][r].j0); box[s][3] = max(box[s][3], site[s][r].j0);
            }
        }
    }
    // 2. the boxes of the tile: across the wave, then across the waves (a wave without a pixel inside the image leaves the identities)
#pragma unroll
    for (int s = 0; STAGE && s < NSETS; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int v = box[s][q];
#pragma unroll
            for (int d = ELD_WAVE / 2; d >= 1; d >>= 1) {
                const int o = __shfl_xor(v, d, ELD_WAVE);
                v = (q & 1) ? max(v, o) : min(v, o);
            }
            if (STAGE && lane == 0) s_box[wave][s][q] = v;
        }
    __syncthreads();                                                 // s_box, and s_t
    int top[NSETS], left[NSETS], bh[NSETS], bw[NSETS];
    size_t need = 0;
#pragma unroll
    for (int s = 0; s < NSETS; ++s) {
        if (!STAGE) { top[s] = left[s] = bh[s] = bw[s] = 0; continue; }
        int lo_i = s_box[0][s][0], hi_i = s_box[0][s][1], lo_j = s_box[0][s][2], hi_j = s_box[0][s][3];
#pragma unroll
        for (int wv = 1; wv < WWAVES; ++wv) {
            lo_i = min(lo_i, s_box[wv][s][0]); hi_i = max(hi_i, s_box[wv][s][1]);
            lo_j = min(lo_j, s_box[wv][s][2]); hi_j = max(hi_j, s_box[wv][s][3]);
        }
        // the tile's first pixel is inside the image, so lo <= hi, both in [-1, L]: the box is i0 - 1 .. i0 + 2 over them, at most L + 5 lines
        top[s] = lo_i - 1; bh[s] = hi_i - lo_i + 4;
        left[s] = lo_j - 1; bw[s] = hi_j - lo_j + 4;
        need += (size_t)bh[s] * (size_t)bw[s] * (size_t)(NSETS == 1 ? 3 : 1);
    }
    const bool staged = STAGE && need <= (size_t)a.lds_floats;       // uniform over the workgroup
    const size_t plane = (size_t)Hm * (size_t)Wm;
    const float* src = a.rgb + (size_t)n * 3 * plane;
    int off[3];                                                      // where plane c's box starts in LDS (staged: the products are small)
    off[0] = 0;
    off[1] = staged ? bh[0] * bw[0] : 0;
    off[2] = staged ? off[1] + bh[NSETS == 1 ? 0 : 1] * bw[NSETS == 1 ? 0 : 1] : 0;
    // 3. staging: the lanes take consecutive elements of a box, row-major (a row of the box is a run of one image row: coalesced); row and
    // column are clamped to the image here
    if (staged) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = NSETS == 1 ? 0 : c;
            float* dst = warp_lds + off[c];
            const float* pl = src + (size_t)c * plane;
            const int cnt = bh[s] * bw[s];
#pragma unroll 4
            for (int e = tid; e < cnt; e += WT) {                    // independent loads: several in flight per lane
                const int r = e / bw[s], q = e - r * bw[s];
                dst[e] = pl[(size_t)clampi(top[s] + r, 0, Hm - 1) * (size_t)Wm + (size_t)clampi(left[s] + q, 0, Wm - 1)];
            }
        }
    }
    if (STAGE) __syncthreads();

    float m[9];
    load_ccm(a.t.ccms, n, m);
    const double ig = (double)a.t.inv_gamma;
    if (!x_in) return;
#pragma unroll
    for (int r = 0; r < WROWS; ++r) {
        const int y = y0 + r;
        if (y >= Hm) break;
        float val[3];
        float wx[NSETS][4], wy[NSETS][4];
#pragma unroll
        for (int s = 0; s < NSETS; ++s) {
            warp_weights(site[s][r].tx, wx[s]);
            warp_weights(site[s][r].ty, wy[s]);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = NSETS == 1 ? 0 : c;
            const WarpSite& t = site[s][r];
            float p[4][4];
            if (staged) {                                            // inside the box by construction: top <= i0 - 1, i0 + 2 < top + bh
                const int b = off[c] + (t.i0 - 1 - top[s]) * bw[s] + (t.j0 - 1 - left[s]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[i][j] = warp_lds[b + i * bw[s] + j];
            } else {
                int cols[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) cols[j] = warp_tap(t.j0, j, Wm);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float* row = src + (size_t)c * plane + (size_t)warp_tap(t.i0, i, Hm) * (size_t)Wm;
#pragma unroll
                    for (int j = 0; j < 4; ++j) p[i][j] = row[cols[j]];
                }
            }
            val[c] = warp_sum16(p, wx[s], wy[s]);
        }
        float o[3];
        site_out<TAIL>(val[0], val[1], val[2], m, a.t, ig, s_t, o);
        const size_t e = (size_t)n * 3 * plane + (size_t)y * (size_t)Wm + (size_t)x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (TAIL == TAIL_LINEAR) ((float*)a.out)[e + c * plane] = o[c];
            else ((unsigned char*)a.out)[e + c * plane] = (unsigned char)o[c];
        }
    }
}

template <int TAIL, int NSETS, bool STAGE>
int warp_launch(const WarpArgs& a, dim3 grid, size_t lds, hipStream_t st) {
    auto kern = warp_kernel<TAIL, NSETS, STAGE>;
    if (lds > (48u << 10)) {                                         // more dynamic LDS than a launch gets by default
        static EldAttrOnce once;
        const int e = once.ensure(kern, WARP_MAX_LDS);
        if (e) return e;
    }
    ELD_LAUNCH(kern, grid, dim3(WT), lds, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int eld_warp_rgb_f32(const float* rgb, void* out, int out_mode, int N, int Hm, int Wm, const EldWarp* warp, const float* ccms, float gamma,
                                const float* crf_E, const float* crf_f, int crf_n, int lds_bytes, void* stream) {
    if (!rgb || !out || !warp) return ELD_EINVAL;
    if (tail_args_bad(ccms, out_mode, gamma, crf_E, crf_f, crf_n)) return ELD_EINVAL;
    if (((uintptr_t)rgb & 15u) || (out_mode == ELD_RENDER_LINEAR_F32 && ((uintptr_t)out & 3u))) return ELD_EINVAL;
    if (N < 0 || N > 65535 || Hm < 1 || Wm < 1 || (uint64_t)Hm * (uint64_t)Wm >= (1ull << 31)) return ELD_EINVAL;
    if (!warp_record_ok(*warp) || lds_bytes > WARP_MAX_LDS) return ELD_EINVAL;
    const dim3 grid((unsigned)((Wm + WTX - 1) / WTX), (unsigned)((Hm + WTY - 1) / WTY), (unsigned)N);
    if (grid.y > 65535u) return ELD_EINVAL;
    {
        const uintptr_t a0 = (uintptr_t)rgb, b0 = (uintptr_t)out, elems = (uintptr_t)N * 3u * (uintptr_t)Hm * (uintptr_t)Wm;
        const uintptr_t na = elems * sizeof(float), nb = elems * (out_mode == ELD_RENDER_LINEAR_F32 ? sizeof(float) : 1u);
        if (a0 < b0 + nb && b0 < a0 + na) return ELD_EINVAL;
    }
    if (N == 0) return 0;
    WarpArgs a = {};
    a.rgb = rgb; a.out = out; a.Hm = Hm; a.Wm = Wm;
    const size_t lds = (size_t)(lds_bytes < 0 ? WARP_DEFAULT_LDS : lds_bytes) & ~(size_t)3;
    a.lds_floats = (int)(lds / sizeof(float));
    a.t = tail_args(ccms, gamma, crf_E, crf_f, crf_n);
    a.w = *warp;
    hipStream_t st = as_stream(stream);
    return with_tail(render_tail(out_mode, gamma, crf_n), [&](auto T) {
        constexpr int TAIL = decltype(T)::value;
        if (lds > 0) return a.w.nsets == 1 ? warp_launch<TAIL, 1, true>(a, grid, lds, st) : warp_launch<TAIL, 3, true>(a, grid, lds, st);
        return a.w.nsets == 1 ? warp_launch<TAIL, 1, false>(a, grid, 0, st) : warp_launch<TAIL, 3, false>(a, grid, 0, st);
    });
}
