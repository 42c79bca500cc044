// demosaic_xdir.hip -- eld_render_xtrans_dir: the full-resolution X-Trans render of demosaic.hip with a directional demosaic in place of the
// isotropic normalised convolution: gains -> clamp -> four dependent stencil stages -> the tail of render_tail.h, planar
// (N,3,Hm,Wm) as 8-bit sRGB codes or float32 linear RGB.  The per-site arithmetic is demosaic_xdir_dev.h's; the evaluation order of every
// float32 expression is the contract of include/eld_amd.h and tests/demosaic_xdir_ref.py restates it operation by operation (the build passes
// -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt).
//
// One workgroup of 384 threads owns a tile of XD_CH x XD_CW whole cells (24 x 96 sites).  The stages reach 6 sites, one cell, so the
// intermediate images go through LDS:
//     v          tile + 6   gain and clamp, gathered from the nine packed planes through the extension's index map (xdir_ext_row / _col):
//                           from here on the frame's border and its interior run the same code with full windows
//     G0         tile + 5   stage A
//     d_h, d_v   tile + 3   stage B's gradients (the 3x3 sums are taken where stage C needs them)
//     G^         tile + 2   stage C, at the R and B sites (a G site's G^ is its v); written over G0, which is dead behind stage B's barrier
//     output     tile       stage D, the matrix and the tone curve, stored from registers
// with a barrier between the stages.  The six waves are the six rows of the cell: wave R runs row R of every cell, a lane one cell's six sites
// of that row, so every site's phase is a compile-time constant and the tap lists of demosaic_xdir_dev.h fold into the code.  Stage B has no
// phase and runs flat over its region.  No atomics, no scratch.
#include "common.h"
#include "demosaic_xdir_dev.h"

namespace {
#include "render_args.h"                   // RenderArgs, gain_clamp, store_sites; with render_tail.h: site_out, load_ccm, TAIL_*, with_tail

constexpr int XD_CH = 4, XD_CW = 16, XD_THREADS = 384;
constexpr int XD_TH = 6 * XD_CH, XD_TW = 6 * XD_CW;
constexpr int XV_H = XD_TH + 2 * XDIR_HALO, XV_W = XD_TW + 2 * XDIR_HALO;     // v: tile + 6 = the tile's cells and one cell around them
constexpr int XG_H = XD_TH + 10, XG_W = XD_TW + 10;                           // G0, then G^: tile + 5
constexpr int XB_H = XD_TH + 6, XB_W = XD_TW + 6;                             // d_h, d_v: tile + 3
constexpr int XE_CH = XD_CH + 2, XE_CW = XD_CW + 2;                           // the cells of v
constexpr int XDIR_LDS_BYTES = (XV_H * XV_W + XG_H * XG_W + 2 * XB_H * XB_W + 256) * 4;
static_assert(XD_THREADS == 6 * ELD_WAVE && XD_CH * XD_CW == ELD_WAVE, "a wave per cell row, a lane per cell of the tile");
static_assert(XV_H == 6 * XE_CH && XV_W == 6 * XE_CW, "v is whole cells");
static_assert(XDIR_LDS_BYTES <= 64 * 1024 && 2 * XDIR_LDS_BYTES <= 160 * 1024, "static LDS; two workgroups per CU");

// stage A, row R of the cell whose first site is (ly0, lx0) of v: G0 at its sites that lie in tile + 5
template <int R>
__device__ __forceinline__ void xd_stage_a(const float* sv, float* sg, int ly0, int lx0) {
    const int ly = ly0 + R;
    if (ly < 1 || ly >= XV_H - 1) return;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const int lx = lx0 + c;
        if (lx < 1 || lx >= XV_W - 1) continue;
        const float* s = sv + ly * XV_W + lx;
        sg[(ly - 1) * XG_W + lx - 1] = XT.colour[6 * R + c] == 1 ? s[0] : xdir_green0(s, XV_W, 6 * R + c);
    }
}

// stage C, row R of that cell: G^ at its R and B sites that lie in tile + 2
template <int R>
__device__ __forceinline__ void xd_stage_c(const float* sv, const float* sdh, const float* sdv, float* sg, int ly0, int lx0) {
    const int ly = ly0 + R;
    if (ly < 4 || ly >= XV_H - 4) return;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        if (XT.colour[6 * R + c] == 1) continue;
        const int lx = lx0 + c;
        if (lx < 4 || lx >= XV_W - 4) continue;
        const int d = (ly - 3) * XB_W + lx - 3;
        sg[(ly - 1) * XG_W + lx - 1] = xdir_green(sv + ly * XV_W + lx, XV_W, sdh + d, sdv + d, XB_W, 6 * R + c);
    }
}

// stage D of row R of the lane's own cell (first site (ly0, lx0) of v): the camera RGB of its six sites
template <int R>
__device__ __forceinline__ void xd_stage_d(const float* sv, const float* sg, int ly0, int lx0, float (&cam)[3][6]) {
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        constexpr int r = R;
        const int ph = 6 * r + c;
        const float* s = sv + (ly0 + r) * XV_W + lx0 + c;
        const float* gp = sg + (ly0 + r - 1) * XG_W + lx0 + c - 1;
        const int col = XT.colour[ph];
        const float g = col == 1 ? s[0] : gp[0];
        cam[0][c] = col == 0 ? s[0] : g + xdir_chroma(s, XV_W, gp, XG_W, ph, 0);
        cam[1][c] = g;
        cam[2][c] = col == 2 ? s[0] : g + xdir_chroma(s, XV_W, gp, XG_W, ph, 1);
    }
}

// the tail of those six sites, stored as three 2-site vectors per colour plane.  Outside the switch over the cell's rows: the six waves share
// one copy of the matrix and the tone curve instead of running six.
template <int TAIL>
__device__ __forceinline__ void xd_row_out(const float (&cam)[3][6], const unsigned* s_t, const RenderArgs& a, const float (&m)[9], double ig, size_t e0,
                                           size_t plane) {
    float o[3][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        float t[3];
        site_out<TAIL>(cam[0][c], cam[1][c], cam[2][c], m, a.t, ig, s_t, t);
        o[0][c] = t[0]; o[1][c] = t[1]; o[2][c] = t[2];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int q = 0; q < 3; ++q) store_sites<TAIL, 2>(a.out, e0 + ch * plane + 2 * q, o[ch][2 * q], o[ch][2 * q + 1]);
}

// the wave's row of the cell as a template argument: wv is wave-uniform
#define XD_ROWS(wv, CALL) \
    switch (wv) {         \
        case 0: { constexpr int R = 0; CALL; } break; \
        case 1: { constexpr int R = 1; CALL; } break; \
        case 2: { constexpr int R = 2; CALL; } break; \
        case 3: { constexpr int R = 3; CALL; } break; \
        case 4: { constexpr int R = 4; CALL; } break; \
        default: { constexpr int R = 5; CALL; } break; \
    }

template <int TAIL>
__global__ __launch_bounds__(XD_THREADS) void render_xtrans_dir_kernel(RenderArgs a, int cells_y, int cells_x) {
    __shared__ float sv[XV_H * XV_W];
    __shared__ float sg[XG_H * XG_W];
    __shared__ float sdh[XB_H * XB_W];
    __shared__ float sdv[XB_H * XB_W];
    __shared__ unsigned s_t[256];
    const int tid = threadIdx.x;
    stage_gamma_table<TAIL, XD_THREADS>(s_t);
    const int n = blockIdx.z, h = a.h, w = a.w, Hm = 3 * h, Wm = 3 * w;
    const int y0 = 6 * XD_CH * blockIdx.y, x0 = 6 * XD_CW * blockIdx.x;              // the tile's first site
    const size_t hw = (size_t)h * w;
    const float* src = a.packed + (size_t)n * 9 * hw;
    const float wr = a.wbs[3 * n], wg = a.wbs[3 * n + 1], wb = a.wbs[3 * n + 2];

    // v on tile + 6, lanes along the row: site (Y, X) of the frame is packed pixel (Y / 3, X / 3) of the plane of its phase.  The frame + 6 goes
    // through the extension; a ragged tile's sites beyond that feed no output and hold zero.
    for (int it = tid; it < XV_H * XV_W; it += XD_THREADS) {
        const int ly = it / XV_W, lx = it - ly * XV_W;
        const int fy = y0 - XDIR_HALO + ly, fx = x0 - XDIR_HALO + lx;
        float v = 0.f;
        if (fy < Hm + XDIR_HALO && fx < Wm + XDIR_HALO) {
            const int Y = xdir_ext_row(fy, Hm), X = xdir_ext_col(fx, Wm);
            const int ph = 6 * (Y % 6) + X % 6;
            const int col = XT.colour[ph];
            v = gain_clamp(src[XT.plane[ph] * hw + (size_t)(Y / 3) * w + X / 3], col == 0 ? wr : col == 1 ? wg : wb);
        }
        sv[it] = v;
    }
    __syncthreads();

    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;

    // stage A on tile + 5: the wave's row of every cell of v
    for (int it = lane; it < XE_CH * XE_CW; it += ELD_WAVE) {
        const int er = it / XE_CW, ec = it - er * XE_CW;
        XD_ROWS(wv, xd_stage_a<R>(sv, sg, 6 * er, 6 * ec))
    }
    __syncthreads();

    // stage B's gradients on tile + 3
    for (int it = tid; it < XB_H * XB_W; it += XD_THREADS) {
        const int ry = it / XB_W, rx = it - ry * XB_W;
        float d_h, d_v;
        xdir_grad(sg + (ry + 2) * XG_W + rx + 2, XG_W, d_h, d_v);
        sdh[it] = d_h;
        sdv[it] = d_v;
    }
    __syncthreads();

    // stage C at the R and B sites of tile + 2, over G0
    for (int it = lane; it < XE_CH * XE_CW; it += ELD_WAVE) {
        const int er = it / XE_CW, ec = it - er * XE_CW;
        XD_ROWS(wv, xd_stage_c<R>(sv, sdh, sdv, sg, 6 * er, 6 * ec))
    }
    __syncthreads();

    // stage D and the tail: the wave's row of the lane's cell
    const int cr = lane / XD_CW, cc = lane - cr * XD_CW;
    const int cy = XD_CH * blockIdx.y + cr, cx = XD_CW * blockIdx.x + cc;
    if (cy >= cells_y || cx >= cells_x) return;
    float m[9];
    load_ccm(a.t.ccms, n, m);
    const double ig = (double)a.t.inv_gamma;
    const size_t plane = (size_t)9 * hw;
    const size_t e0 = (size_t)n * 3 * plane + (size_t)(6 * cy + wv) * Wm + 6 * cx;
    float cam[3][6];
    XD_ROWS(wv, xd_stage_d<R>(sv, sg, 6 * cr + 6, 6 * cc + 6, cam))
    xd_row_out<TAIL>(cam, s_t, a, m, ig, e0, plane);
}
#undef XD_ROWS
}  // namespace

extern "C" int eld_render_xtrans_dir(const float* packed, const float* wbs, const float* ccms, void* out, int out_mode, int N, int h, int w,
                                     float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream) {
    if (render_args_bad(packed, wbs, ccms, out, out_mode, N, gamma, crf_E, crf_f, crf_n) || h < 2 || w < 2 || (h & 1) || (w & 1)) return ELD_EINVAL;
    if (h > (1 << 28) || w > (1 << 28)) return ELD_EINVAL;                 // xdir_ext_row's 2 (3h - 1) is an int
    const int cells_y = h / 2, cells_x = w / 2;
    const unsigned gy = (unsigned)((cells_y + XD_CH - 1) / XD_CH);
    if (gy > 65535u) return ELD_EINVAL;
    const RenderArgs a{packed, wbs, tail_args(ccms, gamma, crf_E, crf_f, crf_n), out, h, w};
    const dim3 grid((unsigned)((cells_x + XD_CW - 1) / XD_CW), gy, N), block(XD_THREADS);
    hipStream_t st = as_stream(stream);
    return with_tail(render_tail(out_mode, gamma, crf_n), [&](auto T) {
        ELD_LAUNCH(render_xtrans_dir_kernel<decltype(T)::value>, grid, block, 0, st, a, cells_y, cells_x);
        ELD_LAUNCH_CHECK();
        return 0;
    });
}

// HOST, no device work: the tile of one workgroup in mosaic sites and the LDS it declares
extern "C" int eld_render_xtrans_dir_tile(int* tile_h, int* tile_w, int* lds_bytes) {
    if (!tile_h || !tile_w) return ELD_EINVAL;
    *tile_h = XD_TH;
    *tile_w = XD_TW;
    if (lds_bytes) *lds_bytes = XDIR_LDS_BYTES;
    return 0;
}
