// demosaic.hip -- full-resolution renders of the packed network output: gains -> clamp -> demosaic -> the tail of
// eld_isp_process (isp_tail.h), at MOSAIC resolution, planar (N,3,Hm,Wm) as 8-bit sRGB codes or as float32 linear RGB after the CCM.
//   * eld_render_bayer:  Malvar-He-Cutler (2004), 5x5 linear, coefficients in eighths, borders mirrored without repeating the edge.
//   * eld_render_xtrans: two-stage normalised convolution on colour differences, windows clipped to the image.
// Both are single streaming passes (4 B read, 3 B or 12 B written per mosaic site); the evaluation order of every float32 expression is
// the contract of include/eld_amd.h and tests/demosaic_ref.py restates it operation by operation (the build passes -ffp-contract=off
// and -fhip-fp32-correctly-rounded-divide-sqrt).
#include "common.h"
#include "xtrans.h"

namespace {
#include "render_args.h"                   // RenderArgs, BayerCell, gain_clamp, store_sites; with render_tail.h: site_out, load_ccm, TAIL_*, with_tail

// ---- Bayer ---------------------------------------------------------------------------------------------------------------------------
// A lane owns BAY_RUN consecutive packed columns of one packed row = a 2 x 8 block of mosaic sites, and reads the 3 x 6 packed
// neighbourhood of its run (the +-2 mosaic halo is +-1 packed) straight from the cache hierarchy: neighbouring lanes and rows re-read the
// same lines, HBM sees each packed value once.
constexpr int BAY_RUN = 4;

__device__ __forceinline__ int mirror(int x, int L) {           // -1 -> 1, -2 -> 2, L -> L - 2; then clamped (only sites nobody uses get clamped)
    x = x < 0 ? -x : x;
    x = x >= L ? 2 * L - 2 - x : x;
    return x < 0 ? 0 : (x > L - 1 ? L - 1 : x);
}

template <bool G00, bool VEC, int TAIL>
__global__ __launch_bounds__(256) void render_bayer_kernel(BayerArgs ba, int groups) {
    const RenderArgs& a = ba.r;
    const BayerCell& cell = ba.cell;
    __shared__ unsigned s_t[256];
    stage_gamma_table<TAIL, 256>(s_t);
    __syncthreads();
    const int n = blockIdx.y, h = a.h, w = a.w;
    const unsigned idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= (unsigned)h * (unsigned)groups) return;
    const int j = idx / groups, i = idx - j * groups;
    const size_t hw = (size_t)h * w;
    const float* src = a.packed + (size_t)n * 4 * hw;
    float gains[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) gains[k] = a.wbs[4 * n + cell.pos[k]];
    float m[9];
    load_ccm(a.t.ccms, n, m);
    const double ig = (double)a.t.inv_gamma;

    // p[dj][sy][sx][q]: the packed value at packed row j - 1 + dj, cell position (sy, sx), packed column 4i - 1 + q (mirrored at the borders),
    // after gain and clamp.  Mosaic site (2j - 2 + y, 8i - 2 + x) of the 6 x 12 window is p[y >> 1][y & 1][x & 1][x >> 1].
    float p[3][2][2][BAY_RUN + 2];
    const int c0 = BAY_RUN * i;
    if (VEC && j >= 1 && j <= h - 2 && i >= 1 && c0 + BAY_RUN <= w - 1) {
#pragma unroll
        for (int dj = 0; dj < 3; ++dj)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* row = src + (size_t)cell.pos[s] * hw + (size_t)(j - 1 + dj) * w + c0;
                const float4 v = *reinterpret_cast<const float4*>(row);
                const float g = gains[s];
                p[dj][s >> 1][s & 1][0] = gain_clamp(row[-1], g);
                p[dj][s >> 1][s & 1][1] = gain_clamp(v.x, g);
                p[dj][s >> 1][s & 1][2] = gain_clamp(v.y, g);
                p[dj][s >> 1][s & 1][3] = gain_clamp(v.z, g);
                p[dj][s >> 1][s & 1][4] = gain_clamp(v.w, g);
                p[dj][s >> 1][s & 1][5] = gain_clamp(row[BAY_RUN], g);
            }
    } else {
#pragma unroll
        for (int dj = 0; dj < 3; ++dj)
#pragma unroll
            for (int sy = 0; sy < 2; ++sy) {
                const int pr = mirror(2 * (j - 1 + dj) + sy, 2 * h) >> 1;
#pragma unroll
                for (int sx = 0; sx < 2; ++sx) {
                    const float* row = src + (size_t)cell.pos[2 * sy + sx] * hw + (size_t)pr * w;
#pragma unroll
                    for (int q = 0; q < BAY_RUN + 2; ++q) {
                        const int pc = mirror(2 * (c0 - 1 + q) + sx, 2 * w) >> 1;
                        p[dj][sy][sx][q] = gain_clamp(row[pc], gains[2 * sy + sx]);
                    }
                }
            }
    }
    auto M = [&](int y, int x) -> float { return p[y >> 1][y & 1][x & 1][x >> 1]; };

    float o[3][2][2 * BAY_RUN];
#pragma unroll
    for (int oy = 0; oy < 2; ++oy)
#pragma unroll
        for (int ox = 0; ox < 2 * BAY_RUN; ++ox) {
            const int y = 2 + oy, x = 2 + ox;
            const float c = M(y, x);
            const float n_s = M(y - 1, x) + M(y + 1, x), w_e = M(y, x - 1) + M(y, x + 1);
            const float nn_ss = M(y - 2, x) + M(y + 2, x), ww_ee = M(y, x - 2) + M(y, x + 2);
            const float D = (M(y - 1, x - 1) + M(y - 1, x + 1)) + (M(y + 1, x - 1) + M(y + 1, x + 1));
            float r, g, b;
            const bool r_in_row = cell.r_row == oy;                   // launch-uniform
            if ((((oy ^ ox) & 1) == 0) == G00) {                   // G site: R and B from the horizontal / vertical formula
                const float hor = (((5.f * c + 4.f * w_e) + 0.5f * nn_ss) - (D + ww_ee)) * 0.125f;
                const float ver = (((5.f * c + 4.f * n_s) + 0.5f * ww_ee) - (D + nn_ss)) * 0.125f;
                g = c;
                r = r_in_row ? hor : ver;
                b = r_in_row ? ver : hor;
            } else {                                               // R or B site
                const float S1 = n_s + w_e, S2 = nn_ss + ww_ee;
                g = ((4.f * c + 2.f * S1) - S2) * 0.125f;
                const float diag = ((6.f * c + 2.f * D) - 1.5f * S2) * 0.125f;
                r = r_in_row ? c : diag;
                b = r_in_row ? diag : c;
            }
            float t[3];
            site_out<TAIL>(r, g, b, m, a.t, ig, s_t, t);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) o[ch][oy][ox] = t[ch];
        }

    const int Wm = 2 * w;
    const size_t plane = (size_t)4 * hw;                           // Hm * Wm
    const int nv = w - c0 < BAY_RUN ? w - c0 : BAY_RUN;          // packed columns of this run that exist (ragged right edge)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int oy = 0; oy < 2; ++oy) {
            const size_t e = ((size_t)n * 3 + ch) * plane + (size_t)(2 * j + oy) * Wm + 2 * c0;
            const float(&v)[2 * BAY_RUN] = o[ch][oy];
            if (VEC) {
                store_sites<TAIL, 2 * BAY_RUN>(a.out, e, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
            } else {
#pragma unroll
                for (int q = 0; q < BAY_RUN; ++q)
                    if (q < nv) store_sites<TAIL, 2>(a.out, e + 2 * q, v[2 * q], v[2 * q + 1]);
            }
        }
}

// ---- X-Trans ---------------------------------------------------------------------------------------------------------------------------
// The per-phase tables of the 6 x 6 cell are xtrans.h's XT, with the checks of the index map and of the window coverage the kernel stands on.

// A workgroup of 128 threads owns a tile of XT_CH x XT_CW whole cells.  LDS holds v (after gain and clamp) of tile + halo 3 (= one
// packed pixel on every side; zero outside the image) and d = v - G^ at the R / B sites of tile + halo 2 (zero outside the image).
constexpr int XT_CH = 4, XT_CW = 32, XT_THREADS = XT_CH * XT_CW;
constexpr int XT_TH = 6 * XT_CH, XT_TW = 6 * XT_CW;
constexpr int XT_LH = XT_TH + 6, XT_LW = XT_TW + 6;
constexpr int XT_PH = XT_TH / 3 + 2, XT_PW = XT_TW / 3 + 2;       // packed pixels of tile + halo

// in-block position (row * XT_LW + col) of plane k in a packed pixel of block parity (pi, pj)
constexpr int xt_lds_off(int k, int pi, int pj) {
    return k < 5 ? (XT_RC[k][pi][pj][0] - 3 * pi) * XT_LW + (XT_RC[k][pi][pj][1] - 3 * pj) : XT_RC3[k - 5][0] * XT_LW + XT_RC3[k - 5][1];
}

// edge flags of a cell: bit 0 top, 1 bottom, 2 left, 3 right frame border
// weight of tap (dy, dx) of the site at cell position (r, c) if the tap lies inside the image, else 0: a compile-time constant unless the
// tap can leave the cell on a side where the frame may end
__device__ __forceinline__ int tap_weight(int r, int c, int dy, int dx, int wt, int edge) {
    bool out = false;
    if (r + dy < 0) out = out || (edge & 1);
    if (r + dy > 5) out = out || (edge & 2);
    if (c + dx < 0) out = out || (edge & 4);
    if (c + dx > 5) out = out || (edge & 8);
    return out ? 0 : wt;
}

// G^ of the non-G site at cell position (r, c); s points at the site's v in LDS.  Taps outside the image hold zero, which leaves the
// running sum as it is; only the weight sum knows them (the clipped window).
__device__ __forceinline__ float xt_green(const float* s, int r, int c, int edge) {
    float acc = 0.f;
    int ws = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
            if ((XT.gmask[6 * r + c] >> (3 * (dy + 1) + dx + 1)) & 1u) {
                const int wt = XT_W3[dy + 1] * XT_W3[dx + 1];
                acc = acc + (float)wt * s[dy * XT_LW + dx];
                ws += tap_weight(r, c, dy, dx, wt, edge);
            }
    return acc / (float)ws;
}

// stage 1 of cell row R of one cell: d = v - G^ at its R / B sites that lie in tile + halo 2 (zero for a cell outside the image)
template <int R>
__device__ __forceinline__ void xt_stage1_row(const float* sv, float* sd, int ly0, int lx0, bool inside, int edge) {
#pragma unroll
    for (int c = 0; c < 6; ++c)
        if (XT.colour[6 * R + c] != 1) {
            const int ly = ly0 + R, lx = lx0 + c;
            if (ly >= 1 && ly < XT_LH - 1 && lx >= 1 && lx < XT_LW - 1) {
                const float* s = sv + ly * XT_LW + lx;
                sd[ly * XT_LW + lx] = inside ? s[0] - xt_green(s, R, c, edge) : 0.f;
            }
        }
}

// stage 2 and the tail of cell row R of the lane's own cell: six sites, stored as three 2-site vectors per colour plane
template <int TAIL, int R>
__device__ __forceinline__ void xt_stage2_row(const float* sv, const float* sd, const unsigned* s_t, const RenderArgs& a, const float (&m)[9],
                                              double ig, int l0, size_t e0, size_t plane, int Wm, int edge) {
    float o[3][6];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        constexpr int r = R;
        const int ph = 6 * r + c;
        const int l = l0 + r * XT_LW + c;
        const float v = sv[l];
        const int col = XT.colour[ph];
        const float g = col == 1 ? v : xt_green(sv + l, r, c, edge);
        float rb[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (col == 2 * k) { rb[k] = v; continue; }
            float acc = 0.f;
            int ws = 0;
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx)
                    if ((XT.cmask[k][ph] >> (5 * (dy + 2) + dx + 2)) & 1u) {
                        const int wt = XT_W5[dy + 2] * XT_W5[dx + 2];
                        acc = acc + (float)wt * sd[l + dy * XT_LW + dx];
                        ws += tap_weight(r, c, dy, dx, wt, edge);
                    }
            rb[k] = g + acc / (float)ws;
        }
        float t[3];
        site_out<TAIL>(rb[0], g, rb[1], m, a.t, ig, s_t, t);
        o[0][c] = t[0]; o[1][c] = t[1]; o[2][c] = t[2];
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const size_t e = e0 + ch * plane + (size_t)R * Wm;
#pragma unroll
        for (int q = 0; q < 3; ++q) store_sites<TAIL, 2>(a.out, e + 2 * q, o[ch][2 * q], o[ch][2 * q + 1]);
    }
}

template <int TAIL>
__global__ __launch_bounds__(XT_THREADS) void render_xtrans_kernel(RenderArgs a, int cells_y, int cells_x) {
    __shared__ float sv[XT_LH * XT_LW];
    __shared__ float sd[XT_LH * XT_LW];
    __shared__ unsigned s_t[256];
    const int tid = threadIdx.x;
    stage_gamma_table<TAIL, XT_THREADS>(s_t);
    const int n = blockIdx.z, h = a.h, w = a.w;
    const int cy0 = blockIdx.y * XT_CH, cx0 = blockIdx.x * XT_CW;        // first cell of the tile
    const size_t hw = (size_t)h * w;
    const float* src = a.packed + (size_t)n * 9 * hw;
    const float wc[3] = {a.wbs[3 * n], a.wbs[3 * n + 1], a.wbs[3 * n + 2]};

    // gather: one packed pixel (nine planes) per lane and step -> its 3 x 3 block of v
    for (int it = tid; it < XT_PH * XT_PW; it += XT_THREADS) {
        const int pr = it / XT_PW, pc = it - pr * XT_PW;
        const int gy = 2 * cy0 - 1 + pr, gx = 2 * cx0 - 1 + pc;
        const bool ok = gy >= 0 && gy < h && gx >= 0 && gx < w;
        const int pi = gy & 1, pj = gx & 1;
        const float* q = src + (size_t)(ok ? gy : 0) * w + (ok ? gx : 0);
        float* d = sv + 3 * pr * XT_LW + 3 * pc;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const float v = ok ? gain_clamp(q[k * hw], wc[xt_colour(k)]) : 0.f;
            const int off = k < 5 ? (pi ? (pj ? xt_lds_off(k, 1, 1) : xt_lds_off(k, 1, 0)) : (pj ? xt_lds_off(k, 0, 1) : xt_lds_off(k, 0, 0)))
                                  : xt_lds_off(k, 0, 0);
            d[off] = v;
        }
    }
    __syncthreads();

    // stage 1 at the R / B sites of tile + halo 2: a lane takes one cell of the (XT_CH + 2) x (XT_CW + 2) cells around the tile
    for (int it = tid; it < (XT_CH + 2) * (XT_CW + 2); it += XT_THREADS) {
        const int er = it / (XT_CW + 2), ec = it - er * (XT_CW + 2);
        const int cy = cy0 - 1 + er, cx = cx0 - 1 + ec;
        const bool inside = cy >= 0 && cy < cells_y && cx >= 0 && cx < cells_x;
        const int edge = (cy == 0 ? 1 : 0) | (cy == cells_y - 1 ? 2 : 0) | (cx == 0 ? 4 : 0) | (cx == cells_x - 1 ? 8 : 0);
        const int ly0 = 6 * er - 3, lx0 = 6 * ec - 3;                      // LDS coordinates of the cell's first site
        xt_stage1_row<0>(sv, sd, ly0, lx0, inside, edge); xt_stage1_row<1>(sv, sd, ly0, lx0, inside, edge);
        xt_stage1_row<2>(sv, sd, ly0, lx0, inside, edge); xt_stage1_row<3>(sv, sd, ly0, lx0, inside, edge);
        xt_stage1_row<4>(sv, sd, ly0, lx0, inside, edge); xt_stage1_row<5>(sv, sd, ly0, lx0, inside, edge);
    }
    __syncthreads();

    // stage 2 and the tail: a lane owns one cell
    const int cr = tid / XT_CW, cc = tid - cr * XT_CW;
    const int cy = cy0 + cr, cx = cx0 + cc;
    if (cy >= cells_y || cx >= cells_x) return;
    const int edge = (cy == 0 ? 1 : 0) | (cy == cells_y - 1 ? 2 : 0) | (cx == 0 ? 4 : 0) | (cx == cells_x - 1 ? 8 : 0);
    float m[9];
    load_ccm(a.t.ccms, n, m);
    const double ig = (double)a.t.inv_gamma;
    const int Wm = 3 * w;
    const size_t plane = (size_t)9 * hw;
    const int l0 = (6 * cr + 3) * XT_LW + 6 * cc + 3;                     // the cell's first site in LDS
    const size_t e0 = (size_t)n * 3 * plane + (size_t)(6 * cy) * Wm + 6 * cx;
    xt_stage2_row<TAIL, 0>(sv, sd, s_t, a, m, ig, l0, e0, plane, Wm, edge); xt_stage2_row<TAIL, 1>(sv, sd, s_t, a, m, ig, l0, e0, plane, Wm, edge);
    xt_stage2_row<TAIL, 2>(sv, sd, s_t, a, m, ig, l0, e0, plane, Wm, edge); xt_stage2_row<TAIL, 3>(sv, sd, s_t, a, m, ig, l0, e0, plane, Wm, edge);
    xt_stage2_row<TAIL, 4>(sv, sd, s_t, a, m, ig, l0, e0, plane, Wm, edge); xt_stage2_row<TAIL, 5>(sv, sd, s_t, a, m, ig, l0, e0, plane, Wm, edge);
}

}  // namespace

extern "C" int eld_render_bayer(const float* packed, const int* raw_pattern, const float* wbs, const float* ccms, void* out, int out_mode,
                                int N, int h, int w, float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream) {
    BayerArgs a{{packed, wbs, tail_args(ccms, gamma, crf_E, crf_f, crf_n), out, h, w}, {}};
    if (render_args_bad(packed, wbs, ccms, out, out_mode, N, gamma, crf_E, crf_f, crf_n) || h < 2 || w < 2) return ELD_EINVAL;
    if (!bayer_cell(raw_pattern, &a.cell)) return ELD_EINVAL;
    const int groups = (w + BAY_RUN - 1) / BAY_RUN;
    if ((long long)h * groups > 0x7fffffffLL - 256) return ELD_EINVAL;
    const bool vec = w % BAY_RUN == 0;                                     // then every run is whole and every row of every plane 16-byte aligned
    const dim3 grid((unsigned)(((long long)h * groups + 255) / 256), N), block(256);
    hipStream_t st = as_stream(stream);
    return with_tail(render_tail(out_mode, gamma, crf_n), [&](auto T) {
        constexpr int TAIL = decltype(T)::value;
        auto kern = a.cell.g00 ? (vec ? render_bayer_kernel<true, true, TAIL> : render_bayer_kernel<true, false, TAIL>)
                        : (vec ? render_bayer_kernel<false, true, TAIL> : render_bayer_kernel<false, false, TAIL>);
        ELD_LAUNCH(kern, grid, block, 0, st, a, groups);
        ELD_LAUNCH_CHECK();
        return 0;
    });
}

extern "C" int eld_render_xtrans(const float* packed, const float* wbs, const float* ccms, void* out, int out_mode, int N, int h, int w,
                                 float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream) {
    if (render_args_bad(packed, wbs, ccms, out, out_mode, N, gamma, crf_E, crf_f, crf_n) || h < 2 || w < 2 || (h & 1) || (w & 1)) return ELD_EINVAL;
    const int cells_y = h / 2, cells_x = w / 2;
    const unsigned gy = (unsigned)((cells_y + XT_CH - 1) / XT_CH);
    if (gy > 65535u) return ELD_EINVAL;
    const RenderArgs a{packed, wbs, tail_args(ccms, gamma, crf_E, crf_f, crf_n), out, h, w};
    const dim3 grid((unsigned)((cells_x + XT_CW - 1) / XT_CW), gy, N), block(XT_THREADS);
    hipStream_t st = as_stream(stream);
    return with_tail(render_tail(out_mode, gamma, crf_n), [&](auto T) {
        ELD_LAUNCH(render_xtrans_kernel<decltype(T)::value>, grid, block, 0, st, a, cells_y, cells_x);
        ELD_LAUNCH_CHECK();
        return 0;
    });
}

// HOST, no device work: the 36 x 8 per-phase table rows (colour, plane, G mask, G weight sum, R mask, R weight sum, B mask, B weight sum)
extern "C" int eld_debug_xtrans_demosaic_tables(int* out, int n) {
    if (!out || n < 36 * 8) return ELD_EINVAL;
    for (int i = 0; i < 36; ++i) {
        int* o = out + 8 * i;
        o[0] = XT.colour[i]; o[1] = XT.plane[i]; o[2] = (int)XT.gmask[i]; o[3] = (int)XT.gsum[i];
        o[4] = (int)XT.cmask[0][i]; o[5] = (int)XT.csum[0][i]; o[6] = (int)XT.cmask[1][i]; o[7] = (int)XT.csum[1][i];
    }
    return 0;
}
