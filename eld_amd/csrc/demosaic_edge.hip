// demosaic_edge.hip -- eld_render_bayer_edge: the full-resolution Bayer render of demosaic.hip with an edge-directed demosaic in place of
// Malvar-He-Cutler: gains -> clamp -> four dependent stencil stages -> the tail of render_tail.h, planar (N,3,Hm,Wm) as
// 8-bit sRGB codes or float32 linear RGB.  The per-site arithmetic is demosaic_edge_dev.h's; the evaluation order of every float32 expression
// is the contract of include/eld_amd.h and tests/demosaic_edge_ref.py restates it operation by operation (the build passes
// -ffp-contract=off and -fhip-fp32-correctly-rounded-divide-sqrt).
//
// One workgroup of 256 threads owns a tile of EDGE_TH x EDGE_TW mosaic sites.  The stages reach 4 sites, so, unlike the direct MHC kernel, the
// intermediate images go through LDS:
//     v          tile + 4   gain and clamp, gathered from the four packed planes through mirrored indices (edge_reflect): from here on the
//                           frame's border and its interior run the same code
//     d_h, d_v   tile + 2   stage A
//     G^         tile + 1   stages B and C, at the R and B sites (a G site's G^ is its v)
//     output     tile       stage D, the matrix and the tone curve, stored from registers
// with a barrier between the stages.  a_h, a_v (stage C) and delta = v - G^ (stage D) are recomputed from LDS with stage A's / the contract's own
// instructions instead of stored.  Pitches are odd: the lanes of stage D own 4 adjacent sites of a row (stride 4 dwords) and a 32-lane group
// spans two rows of one parity, which an odd pitch puts on different banks.
#include "common.h"
#include "mosaic_dev.h"
#include "demosaic_edge_dev.h"

namespace {
#include "render_args.h"                   // RenderArgs, BayerCell, gain_clamp, store_sites; with render_tail.h: site_out, load_ccm, TAIL_*, with_tail

constexpr int EDGE_TH = 16, EDGE_TW = 64, EDGE_THREADS = 256;
constexpr int EV_H = EDGE_TH + 2 * EDGE_HALO, EV_W = EDGE_TW + 2 * EDGE_HALO, EV_P = EV_W + 1;        // v: tile + 4
constexpr int ED_H = EDGE_TH + 4, ED_W = EDGE_TW + 4, ED_P = ED_W + 1;                                // d_h, d_v: tile + 2
constexpr int EG_H = EDGE_TH + 2, EG_W = EDGE_TW + 2, EG_P = EG_W + 1;                                // G^: tile + 1
constexpr int EDGE_LDS_BYTES = (EV_H * EV_P + 2 * ED_H * ED_P + EG_H * EG_P + 256) * 4;
static_assert(EDGE_TH % 2 == 0 && EDGE_TW % 4 == 0 && EDGE_THREADS == EDGE_TH * (EDGE_TW / 4), "a lane of stage D owns 4 sites of one row");
static_assert(EDGE_THREADS / ELD_WAVE == 4 && EDGE_TW / 4 == 16 && EDGE_TH == 16, "stage D's lane map: 4 waves of 4 rows x 16 lanes");
static_assert(EV_P % 2 == 1 && ED_P % 2 == 1 && EG_P % 2 == 1, "odd pitches");
static_assert(2 * EDGE_LDS_BYTES <= 160 * 1024, "at least two workgroups per CU");

// stage D and the tail of the lane's 4 sites (row ty of the tile, columns tx .. tx + 3, tx % 4 == 0); OY: the row's parity
template <bool G00, int TAIL, int OY>
__device__ __forceinline__ void edge_row_out(const float* sv, const float* sg, const unsigned* s_t, const TailArgs& a, int r_row, const float (&m)[9],
                                             double ig, int ty, int tx, float (&o)[3][4]) {
    const bool r_in_row = r_row == OY;                           // launch-uniform
#pragma unroll
    for (int ox = 0; ox < 4; ++ox) {
        const float* c = sv + (ty + EDGE_HALO) * EV_P + tx + ox + EDGE_HALO;
        const float* g = sg + (ty + 1) * EG_P + tx + ox + 1;
        float r, gg, b;
        if ((((OY ^ ox) & 1) == 0) == G00) {                       // G site
            float hor, ver;
            edge_rb_at_g(c, EV_P, g, EG_P, hor, ver);
            gg = c[0];
            r = r_in_row ? hor : ver;
            b = r_in_row ? ver : hor;
        } else {                                                   // R or B site
            const float other = edge_other_at_rb(c, EV_P, g, EG_P);
            gg = g[0];
            r = r_in_row ? c[0] : other;
            b = r_in_row ? other : c[0];
        }
        float t[3];
        site_out<TAIL>(r, gg, b, m, a, ig, s_t, t);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[ch][ox] = t[ch];
    }
}

template <bool G00, int TAIL>
__global__ __launch_bounds__(EDGE_THREADS) void render_bayer_edge_kernel(BayerArgs ba, int wide) {
    const RenderArgs& a = ba.r;
    const BayerCell& cell = ba.cell;
    __shared__ float sv[EV_H * EV_P];
    __shared__ float sdh[ED_H * ED_P];
    __shared__ float sdv[ED_H * ED_P];
    __shared__ float sg[EG_H * EG_P];
    __shared__ unsigned s_t[256];
    const int tid = threadIdx.x;
    stage_gamma_table<TAIL, EDGE_THREADS>(s_t);
    const int n = blockIdx.z, h = a.h, w = a.w, Hm = 2 * h, Wm = 2 * w;
    const int y0 = blockIdx.y * EDGE_TH, x0 = blockIdx.x * EDGE_TW;           // the tile's first site; both even
    const size_t hw = (size_t)h * w;
    const float* src = a.packed + (size_t)n * 4 * hw;

    // v on tile + 4: per cell position a (EV_H / 2) x (EV_W / 2) block of one packed plane, lanes along the packed row.  The extension keeps
    // parity, so the site at cell position (sy, sx) of the extended tile is packed pixel (Y >> 1, X >> 1) of that position's plane.
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float* plane = src + (size_t)cell.pos[s] * hw;
        const float gain = a.wbs[4 * n + cell.pos[s]];
        for (int it = tid; it < (EV_H / 2) * (EV_W / 2); it += EDGE_THREADS) {
            const int pr = it / (EV_W / 2), pc = it - pr * (EV_W / 2);
            const int ly = 2 * pr + (s >> 1), lx = 2 * pc + (s & 1);
            const int Y = edge_reflect(y0 - EDGE_HALO + ly, Hm), X = edge_reflect(x0 - EDGE_HALO + lx, Wm);
            sv[ly * EV_P + lx] = gain_clamp(plane[(size_t)(Y >> 1) * w + (X >> 1)], gain);
        }
    }
    __syncthreads();

    // stage A on tile + 2
    for (int it = tid; it < ED_H * ED_W; it += EDGE_THREADS) {
        const int ry = it / ED_W, rx = it - ry * ED_W;
        float d_h, d_v;
        edge_grad(sv + (ry + 2) * EV_P + rx + 2, EV_P, d_h, d_v);
        sdh[ry * ED_P + rx] = d_h;
        sdv[ry * ED_P + rx] = d_v;
    }
    __syncthreads();

    // stages B and C at the R and B sites of tile + 1: every other site of a row.  Row ry, column rx of tile + 1 is site (y0 - 1 + ry,
    // x0 - 1 + rx): a G site when ((ry ^ rx) & 1) == 0 is G00.
    for (int it = tid; it < EG_H * (EG_W / 2); it += EDGE_THREADS) {
        const int ry = it / (EG_W / 2), k = it - ry * (EG_W / 2);
        const int rx = 2 * k + ((int)cell_phase<2>((uint32_t)ry) ^ (G00 ? 1 : 0));
        sg[ry * EG_P + rx] = edge_green(sv + (ry + 3) * EV_P + rx + 3, EV_P, sdh + (ry + 1) * ED_P + rx + 1, sdv + (ry + 1) * ED_P + rx + 1, ED_P);
    }
    __syncthreads();

    // stage D and the tail: a wave owns 4 rows of one parity (waves 0, 1: rows 0 .. 7 of the tile, waves 2, 3: rows 8 .. 15), 16 lanes per row
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int ty = (wv >> 1) * 8 + 2 * (lane >> 4) + (wv & 1), tx = 4 * (lane & 15);
    const int Y = y0 + ty, X = x0 + tx;
    if (Y >= Hm || X >= Wm) return;
    float m[9];
    load_ccm(a.t.ccms, n, m);
    const double ig = (double)a.t.inv_gamma;
    float o[3][4];
    if (wv & 1) edge_row_out<G00, TAIL, 1>(sv, sg, s_t, a.t, cell.r_row, m, ig, ty, tx, o);
    else edge_row_out<G00, TAIL, 0>(sv, sg, s_t, a.t, cell.r_row, m, ig, ty, tx, o);

    // Wm is even and X a multiple of 4: a lane's sites are 4, or the 2 in front of the right edge of a frame with Wm % 4 == 2
    const size_t plane = (size_t)4 * hw;                           // Hm * Wm, a multiple of 4
    const bool pair2 = X + 2 < Wm;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const size_t e = ((size_t)n * 3 + ch) * plane + (size_t)Y * Wm + X;
        const float(&v)[4] = o[ch];
        if (wide) {
            store_sites<TAIL, 4>(a.out, e, v[0], v[1], v[2], v[3]);
        } else {
            store_sites<TAIL, 2>(a.out, e, v[0], v[1]);
            if (pair2) store_sites<TAIL, 2>(a.out, e + 2, v[2], v[3]);
        }
    }
}
}  // namespace

extern "C" int eld_render_bayer_edge(const float* packed, const int* raw_pattern, const float* wbs, const float* ccms, void* out, int out_mode,
                                     int N, int h, int w, float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream) {
    BayerArgs a{{packed, wbs, tail_args(ccms, gamma, crf_E, crf_f, crf_n), out, h, w}, {}};
    if (render_args_bad(packed, wbs, ccms, out, out_mode, N, gamma, crf_E, crf_f, crf_n) || h < 1 || w < 1) return ELD_EINVAL;
    if (h > (1 << 28) || w > (1 << 28)) return ELD_EINVAL;                 // edge_reflect's period 2 (2h - 1) is an int
    if (!bayer_cell(raw_pattern, &a.cell)) return ELD_EINVAL;
    const long long gx = (2LL * w + EDGE_TW - 1) / EDGE_TW, gy = (2LL * h + EDGE_TH - 1) / EDGE_TH;
    if (gy > 65535 || gx > 0x7fffffffLL) return ELD_EINVAL;
    const int wide = w % 2 == 0;           // Wm % 4 == 0: every lane's 4 sites exist and start 16-byte (float32) / 4-byte (codes) aligned
    const dim3 grid((unsigned)gx, (unsigned)gy, N), block(EDGE_THREADS);
    hipStream_t st = as_stream(stream);
    return with_tail(render_tail(out_mode, gamma, crf_n), [&](auto T) {
        constexpr int TAIL = decltype(T)::value;
        auto kern = a.cell.g00 ? render_bayer_edge_kernel<true, TAIL> : render_bayer_edge_kernel<false, TAIL>;
        ELD_LAUNCH(kern, grid, block, 0, st, a, wide);
        ELD_LAUNCH_CHECK();
        return 0;
    });
}

// HOST, no device work: the tile of one workgroup in mosaic sites and the LDS it declares
extern "C" int eld_render_bayer_edge_tile(int* tile_h, int* tile_w, int* lds_bytes) {
    if (!tile_h || !tile_w) return ELD_EINVAL;
    *tile_h = EDGE_TH;
    *tile_w = EDGE_TW;
    if (lds_bytes) *lds_bytes = EDGE_LDS_BYTES;
    return 0;
}
