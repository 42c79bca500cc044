// eval.hip -- evaluation-side kernels of the path, all HBM-bound single passes:
//   * quality_assess: PSNR and multichannel SSIM of util/index.py:76-81 on the x255-clipped images of tensor2im
//     (models/ELD_model.py:23-38), i.e. skimage.metrics.peak_signal_noise_ratio / structural_similarity(data_range=255,
//     multichannel=True) with skimage's defaults (7x7 uniform window, K1 = 0.01, K2 = 0.03, sample covariance, windows
//     fully inside the image, channels averaged) -- the frames never leave the device;
//   * illuminance_correct: models/ELD_model.py:138-169, out = <p,s>/<p,p> * p over the elements with s != 1, p clamped
//     to [0,1], one scale per image.
// Sums are accumulated in double and reduced in a fixed order (run-to-run bit-stable, no atomics).
#include "mosaic_dev.h"
#include "xtrans.h"

int debug_kernel_mask(int set);      // conv_bfs.hip (eld_debug_kernel_mask): set < 0 only queries

namespace {

constexpr int QA_TW = 32, QA_TH = 8, WIN = 7, HALO = WIN - 1;
constexpr int RED_BLOCKS = 512;

// tensor2im (ELD_model.py:23-38): np.clip(x * 255, 0, 255).  mul = 255 for [0,1] inputs; mul = 1 (an exact no-op multiply) for values
// that are already images on the [0, range] scale (util/index.py's own callers)
__device__ __forceinline__ float to_im(float v, float mul, float range) { return fminf(fmaxf(v * mul, 0.f), range); }

// the same clip as one v_med3_f32 (finite values: median(v, 0, range) == min(max(v, 0), range))
__device__ __forceinline__ float to_im3(float v, float mul, float range) { return __builtin_amdgcn_fmed3f(v * mul, 0.f, range); }

__device__ __forceinline__ double block_sum(double v, double* sh) {       // 256 threads, fixed tree
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// one workgroup = one 32x8 tile of window positions of one (image, channel) plane; writes the tile's sum of S
__global__ __launch_bounds__(256) void ssim_kernel(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ part,
                                                   int H, int W, int tiles_x, int tiles_y, float mul, float scale) {
    __shared__ float lx[QA_TH + HALO][QA_TW + HALO], ly[QA_TH + HALO][QA_TW + HALO];
    __shared__ double hs[5][QA_TH + HALO][QA_TW];
    __shared__ double red[256];
    const int plane = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * QA_TH, x0 = tx * QA_TW;
    const int Ho = H - HALO, Wo = W - HALO;                       // window positions
    const float* px = est + (size_t)plane * H * W;
    const float* py = ref + (size_t)plane * H * W;
    for (int i = threadIdx.x; i < (QA_TH + HALO) * (QA_TW + HALO); i += 256) {
        const int r = i / (QA_TW + HALO), c = i - r * (QA_TW + HALO);
        const int gy = y0 + r, gx = x0 + c;
        const bool ok = gy < H && gx < W;
        lx[r][c] = ok ? to_im(px[(size_t)gy * W + gx], mul, scale) : 0.f;
        ly[r][c] = ok ? to_im(py[(size_t)gy * W + gx], mul, scale) : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (QA_TH + HALO) * QA_TW; i += 256) {      // horizontal 7-sums of x, y, xx, yy, xy
        const int r = i / QA_TW, c = i - r * QA_TW;
        double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int d = 0; d < WIN; ++d) {
            const double a = lx[r][c + d], b = ly[r][c + d];
            sx += a; sy += b; sxx += a * a; syy += b * b; sxy += a * b;
        }
        hs[0][r][c] = sx; hs[1][r][c] = sy; hs[2][r][c] = sxx; hs[3][r][c] = syy; hs[4][r][c] = sxy;
    }
    __syncthreads();
    const int r = threadIdx.x / QA_TW, c = threadIdx.x - r * QA_TW;
    double S = 0.0;
    if (y0 + r < Ho && x0 + c < Wo) {
        double s[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double a = 0;
#pragma unroll
            for (int d = 0; d < WIN; ++d) a += hs[q][r + d][c];
            s[q] = a * (1.0 / (WIN * WIN));
        }
        const double cov_norm = (double)(WIN * WIN) / (WIN * WIN - 1.0);
        const double ux = s[0], uy = s[1];
        const double vx = cov_norm * (s[2] - ux * ux), vy = cov_norm * (s[3] - uy * uy), vxy = cov_norm * (s[4] - ux * uy);
        const double C1 = (0.01 * (double)scale) * (0.01 * (double)scale), C2 = (0.03 * (double)scale) * (0.03 * (double)scale);
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
    }
    const double tot = block_sum(S, red);
    if (threadIdx.x == 0) part[(size_t)plane * tiles_x * tiles_y + blockIdx.x] = tot;
}

// squared error of the x255-clipped images: grid (RED_BLOCKS, N)
__global__ __launch_bounds__(256) void sqerr_kernel(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ part, size_t chw, float mul, float scale) {
    __shared__ double red[256];
    const float* a = est + (size_t)blockIdx.y * chw;
    const float* b = ref + (size_t)blockIdx.y * chw;
    double s = 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < chw; i += (size_t)RED_BLOCKS * 256) {
        const double d = (double)to_im(b[i], mul, scale) - (double)to_im(a[i], mul, scale);
        s += d * d;
    }
    const double tot = block_sum(s, red);
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * RED_BLOCKS + blockIdx.x] = tot;
}

// one workgroup per image: out[2n] = PSNR, out[2n+1] = SSIM
__global__ __launch_bounds__(256) void qa_final_kernel(const double* __restrict__ sq, const double* __restrict__ ss, double* __restrict__ out, int C,
                                                       int tiles, size_t chw, size_t windows, float scale) {
    __shared__ double red[256];
    const int n = blockIdx.x;
    double a = 0.0;
    for (int i = threadIdx.x; i < RED_BLOCKS; i += 256) a += sq[(size_t)n * RED_BLOCKS + i];
    const double err = block_sum(a, red) / (double)chw;
    double ssim = 0.0;
    for (int c = 0; c < C; ++c) {                      // mean over channels of the per-channel means (multichannel=True)
        double b = 0.0;
        for (int i = threadIdx.x; i < tiles; i += 256) b += ss[((size_t)n * C + c) * tiles + i];
        ssim += block_sum(b, red) / (double)windows;
    }
    if (threadIdx.x == 0) {
        out[2 * n] = 10.0 * log10((double)scale * (double)scale / err);
        out[2 * n + 1] = ssim / C;
    }
}

// ---- round 5: PSNR + SSIM in ONE pass, no LDS, no workgroup barriers -------------------------------------------------------------------
// The tile kernel above re-reads a 14 x 38 halo per 8 x 32 window positions (2.1x), runs three barriers plus a nine-barrier double-precision tree
// per 256 results and a second pass (sqerr_kernel) over both images: 0.25 ms for one 4 x 1424 x 2128 frame pair = 0.05 of HBM.
// Here one WAVE owns a strip of 64 * NC columns x QA_RH rows of one plane and slides down it: a lane owns NC adjacent window columns, forms the
// horizontal 7-sums of the four moments SSIM needs (sum a, sum b, sum (a^2 + b^2), sum ab -- var_x + var_y only ever appear added) for the input
// row that enters the window, keeps the last seven rows' sums in registers (ring indexed at compile time: the row loop is unrolled by 14 =
// lcm(7 ring slots, 2 load buffers)) and updates the vertical sum by adding the entering row and subtracting the leaving one.  With NC = 2 the two
// windows of a lane share their six common columns (5 + 2 adds per moment for two windows instead of 12) and every pixel is converted by four
// lanes instead of seven.  Every accumulation is double and every order is fixed (per lane: rows top to bottom; per wave: a butterfly; per image:
// qa_final2_kernel's strided sum + tree): run-to-run bit-stable.  Products of two float32 values are exact in double, so the fused multiply-adds
// below round exactly like a multiply followed by an add; and for identical images the result is exactly PSNR = inf / SSIM = 1: q = a^2 + b^2 is
// formed per pixel and summed in the same order as p = ab, so every partial sum of q is exactly twice that of p (and A1 == B1, A2 == B2 below).  Rows are loaded two ahead of
// their use (two register buffers); the shifted loads of a lane hit the lines its neighbours fetch (L1).  The squared error of PSNR rides along:
// a lane adds (b - a)^2 of its OWN columns for the rows its item owns (strips / chunks are cut over ALL columns / rows, so every pixel has an owner).
constexpr int QA_RH = 106, QA_ROWS = QA_RH + HALO;                  // 112 input rows per item = 8 x 14
static_assert(QA_ROWS % 14 == 0, "row loop unrolled by 14");

// EDGE = false: every column this wave reads exists (uniform row base + per-lane column + immediate k: no address arithmetic per load);
// EDGE = true (the last strip of a row of strips): column indices clamped to W - 1
template <int NC, bool EDGE>
__device__ __forceinline__ void qa_item(const float* __restrict__ px, const float* __restrict__ py, double* __restrict__ ss_out, double* __restrict__ sq_out,
                                        int H, int W, int y0, int c, int lane, float mul, float scale) {
    constexpr int NV = WIN + NC - 1;                                // input columns a lane reads per row
    const int Ho = H - HALO, Wo = W - HALO;
    // window outputs that do not exist (column >= Wo, row >= Ho) are computed from clamped addresses and discarded: an existing output only ever
    // reads in-range pixels, so no zero padding is needed -- only in-bounds addresses
    int idx[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) idx[k] = min(c + k, W - 1);
    float pa[2][NV], pb[2][NV];
    auto issue = [&](int i, float (&A)[NV], float (&B)[NV]) {       // loads of input row y0 + i (clamped)
        const size_t ro = (size_t)min(y0 + i, H - 1) * W;
        const float* rx = px + ro;
        const float* ry = py + ro;
#pragma unroll
        for (int k = 0; k < NV; ++k) { A[k] = rx[EDGE ? idx[k] : c + k]; B[k] = ry[EDGE ? idx[k] : c + k]; }
    };
    issue(0, pa[0], pb[0]);
    issue(1, pa[1], pb[1]);
    double ring[WIN][NC][4], vs[NC][4];
#pragma unroll
    for (int w = 0; w < NC; ++w)
#pragma unroll
        for (int q = 0; q < 4; ++q) vs[w][q] = 0.0;
    double S_acc = 0.0, sq = 0.0;
    const double NP = (double)(WIN * WIN), cov_norm = NP / (NP - 1.0);
    const double K1 = (0.01 * (double)scale) * (0.01 * (double)scale) * (NP * NP), K2 = (0.03 * (double)scale) * (0.03 * (double)scale) * (NP * NP);
#pragma unroll 1
    for (int u = 0; u < QA_ROWS / 14; ++u) {
#pragma unroll
        for (int j = 0; j < 14; ++j) {
            const int i = 14 * u + j;                               // input row of the item; ring slot j % 7, load buffer j % 2 (compile time)
            // one column at a time, summed as soon as it is converted (few live doubles: the kernel's registers are the ring); the NC windows share
            // columns NC-1 .. 6: one core sum per moment, then the private columns on either side (the same tree for all four moments)
            double h[NC][4];
            {
                const bool own_row = i < QA_RH && y0 + i < H;       // this item's own rows: squared error of this lane's own columns
                double e0[4], c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
#pragma unroll
                for (int k = 0; k < NV; ++k) {
                    const double ak = (double)to_im3(pa[j & 1][k], mul, scale), bk = (double)to_im3(pb[j & 1][k], mul, scale);
                    const double qk = __builtin_fma(bk, bk, ak * ak), pk = ak * bk;
                    if (k < NC && own_row && c + k < W) { const double d = bk - ak; sq = __builtin_fma(d, d, sq); }
                    if (NC == 2 && k == 0) { e0[0] = ak; e0[1] = bk; e0[2] = qk; e0[3] = pk; }
                    else if (k == NC - 1) { c0 = ak; c1 = bk; c2 = qk; c3 = pk; }
                    else if (k < WIN) { c0 = c0 + ak; c1 = c1 + bk; c2 = c2 + qk; c3 = c3 + pk; }
                    else if constexpr (NC == 2) { h[NC - 1][0] = c0 + ak; h[NC - 1][1] = c1 + bk; h[NC - 1][2] = c2 + qk; h[NC - 1][3] = c3 + pk; }      // k == WIN: the second window's last column
                }
                if constexpr (NC == 1) { h[0][0] = c0; h[0][1] = c1; h[0][2] = c2; h[0][3] = c3; (void)e0; }
                else { h[0][0] = e0[0] + c0; h[0][1] = e0[1] + c1; h[0][2] = e0[2] + c2; h[0][3] = e0[3] + c3; }
            }
            if (i + 2 < QA_ROWS) issue(i + 2, pa[j & 1], pb[j & 1]);      // the buffer is free: its values were consumed above
            const int leave = (j + 1) % WIN;                        // ring slot of row i - 6 ((i - 6) % 7 == (i + 1) % 7)
#pragma unroll
            for (int w = 0; w < NC; ++w) {
#pragma unroll
                for (int m = 0; m < 4; ++m) vs[w][m] = vs[w][m] + h[w][m];
                if (i >= HALO) {                                    // rows i-6 .. i are summed: the window of output row y0 + i - 6
                    if (c + w < Wo && y0 + i - HALO < Ho) {
                        // S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) with u = s / 49, v = cov_norm (s_2 / 49 - u u): both
                        // factors of numerator and denominator scaled by 49^2, so the window sums are used as they are
                        const double s0 = vs[w][0], s1 = vs[w][1];
                        const double t = s0 * s1, uu = s0 * s0 + s1 * s1;
                        const double A1 = __builtin_fma(2.0, t, K1), B1 = uu + K1;
                        const double A2 = __builtin_fma(2.0 * cov_norm, __builtin_fma(NP, vs[w][3], -t), K2);
                        const double B2 = __builtin_fma(cov_norm, __builtin_fma(NP, vs[w][2], -uu), K2);
                        S_acc = S_acc + (A1 * A2) / (B1 * B2);
                    }
#pragma unroll
                    for (int m = 0; m < 4; ++m) vs[w][m] = vs[w][m] - ring[leave][w][m];
                }
#pragma unroll
                for (int m = 0; m < 4; ++m) ring[j % WIN][w][m] = h[w][m];
            }
        }
    }
    const double Sw = wave_sum(S_acc), Qw = wave_sum(sq);
    if (lane == 0) { *ss_out = Sw; *sq_out = Qw; }
}

template <int NC>
__global__ __launch_bounds__(256) void qa_fused_kernel(const float* __restrict__ est, const float* __restrict__ ref, double* __restrict__ ss_part,
                                                       double* __restrict__ sq_part, int H, int W, int strips, int chunks, float mul, float scale) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blockIdx.x * 4 + wave;
    if (item >= strips * chunks) return;                            // (no barrier anywhere in this kernel)
    const int plane = blockIdx.y;
    const int chunk = item / strips, strip = item - chunk * strips;
    const int y0 = chunk * QA_RH, c = (strip * 64 + lane) * NC;
    const float* px = est + (size_t)plane * H * W;
    const float* py = ref + (size_t)plane * H * W;
    const size_t o = (size_t)plane * strips * chunks + item;
    if ((strip * 64 + 63) * NC + WIN + NC - 1 <= W) qa_item<NC, false>(px, py, ss_part + o, sq_part + o, H, W, y0, c, lane, mul, scale);      // wave-uniform
    else qa_item<NC, true>(px, py, ss_part + o, sq_part + o, H, W, y0, c, lane, mul, scale);
}

// one workgroup per image: out[2n] = PSNR, out[2n+1] = SSIM from the per-item partials of qa_fused_kernel ([plane][item])
__global__ __launch_bounds__(256) void qa_final2_kernel(const double* __restrict__ ss, const double* __restrict__ sq, double* __restrict__ out, int C,
                                                        int items, size_t chw, size_t windows, float scale) {
    __shared__ double red[256];
    const int n = blockIdx.x;
    double a = 0.0;
    for (int i = threadIdx.x; i < C * items; i += 256) a += sq[(size_t)n * C * items + i];
    const double err = block_sum(a, red) / (double)chw;
    double ssim = 0.0;
    for (int c = 0; c < C; ++c) {                      // mean over channels of the per-channel means (multichannel=True)
        double b = 0.0;
        for (int i = threadIdx.x; i < items; i += 256) b += ss[((size_t)n * C + c) * items + i];
        ssim += block_sum(b, red) / (double)windows;
    }
    if (threadIdx.x == 0) {
        out[2 * n] = 10.0 * log10((double)scale * (double)scale / err);
        out[2 * n + 1] = ssim / C;
    }
}

// illuminance correction, pass 1: per-block partial <p,s> and <p,p> over s != 1 (p clamped to [0,1]); grid (RED_BLOCKS, N).
// VEC: 16-byte loads (chw % 4 == 0 and 16-byte aligned planes: every frame of the path); the scalar form stays for odd sizes.
__device__ __forceinline__ void illum_acc(float pv_, float sv, double& num, double& den) {
    if (sv != 1.0f) {
        const double pv = fminf(fmaxf(pv_, 0.f), 1.f);
        num += pv * (double)sv; den += pv * pv;
    }
}
template <bool VEC>
__global__ __launch_bounds__(256) void illum_dot_kernel(const float* __restrict__ pred, const float* __restrict__ src, double* __restrict__ part, size_t chw,
                                                        size_t src_stride) {
    __shared__ double red[256];
    const float* p = pred + (size_t)blockIdx.y * chw;
    const float* s = src + (size_t)blockIdx.y * src_stride;
    double num = 0.0, den = 0.0;
    if (VEC) {
        const float4* p4 = reinterpret_cast<const float4*>(p);
        const float4* s4 = reinterpret_cast<const float4*>(s);
        const size_t n4 = chw >> 2;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)RED_BLOCKS * 256) {
            const float4 a = p4[i], b = s4[i];
            illum_acc(a.x, b.x, num, den); illum_acc(a.y, b.y, num, den); illum_acc(a.z, b.z, num, den); illum_acc(a.w, b.w, num, den);
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < chw; i += (size_t)RED_BLOCKS * 256) illum_acc(p[i], s[i], num, den);
    }
    const double tn = block_sum(num, red), td = block_sum(den, red);
    if (threadIdx.x == 0) { part[((size_t)blockIdx.y * RED_BLOCKS + blockIdx.x) * 2] = tn; part[((size_t)blockIdx.y * RED_BLOCKS + blockIdx.x) * 2 + 1] = td; }
}

__global__ __launch_bounds__(256) void illum_alpha_kernel(const double* __restrict__ part, float* __restrict__ alpha) {
    __shared__ double red[256];
    const int n = blockIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < RED_BLOCKS; i += 256) { a += part[((size_t)n * RED_BLOCKS + i) * 2]; b += part[((size_t)n * RED_BLOCKS + i) * 2 + 1]; }
    const double num = block_sum(a, red), den = block_sum(b, red);
    if (threadIdx.x == 0) alpha[n] = (float)num / (float)den;             // num / den as fp32 tensors (ELD_model.py:164-166)
}

template <bool VEC>
__global__ __launch_bounds__(256) void illum_scale_kernel(const float* __restrict__ pred, const float* __restrict__ alpha, float* __restrict__ out, size_t chw) {
    const float a = alpha[blockIdx.y];
    const size_t base = (size_t)blockIdx.y * chw;
    if (VEC) {
        const float4* p4 = reinterpret_cast<const float4*>(pred + base);
        float4* o4 = reinterpret_cast<float4*>(out + base);
        const size_t n4 = chw >> 2;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
            const float4 v = p4[i];
            o4[i] = make_float4(a * fminf(fmaxf(v.x, 0.f), 1.f), a * fminf(fmaxf(v.y, 0.f), 1.f), a * fminf(fmaxf(v.z, 0.f), 1.f), a * fminf(fmaxf(v.w, 0.f), 1.f));
        }
    } else {
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < chw; i += (size_t)gridDim.x * 256)
            out[base + i] = a * fminf(fmaxf(pred[base + i], 0.f), 1.f);
    }
}

// ---- raw -> sRGB ISP: util/process.py:52-68 `process`, one pass: 16 B read + 12 B written per RGBG position.
//      gains (15-19) -> clamp -> binning R, (G1+G2)/2, B (42-49) -> 3x3 CCM with j ascending (22-31) -> clamp -> gamma
//      compression max(x,1e-8)^(1/gamma) (34-39) or piecewise-linear camera response (71-83) -> truncating 8-bit quantiser.
//      gamma == 2.2 (the only value the reference passes): power + quantiser are ONE exact step function of the clamped input,
//      tabulated from torch's own float32 evaluation over every float32 in [0, 1] (gamma22_table.h, oracle/gen_gamma_table.py):
//      bit-exact 8-bit codes.  Other gammas: the power in double, rounded once (then +-1 code on isolated pixels is possible).
//      The tail (CCM -> clamp -> gamma / CRF -> quantiser) lives in isp_tail.h: the full-resolution renders (demosaic.hip) call the same function.
#include "isp_tail.h"

__global__ __launch_bounds__(256) void isp_kernel(const float* __restrict__ bayer, const float* __restrict__ wbs, const float* __restrict__ ccms,
                                                  float* __restrict__ out, size_t hw, float inv_gamma, const float* __restrict__ crf_E,
                                                  const float* __restrict__ crf_f, int crf_n, int gtab) {
    __shared__ unsigned s_t[256];
    if (gtab) s_t[threadIdx.x] = ELD_GAMMA22_T[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.y;
    const float* wb = wbs + 4 * n;
    const float* cm = ccms + 9 * n;
    const float w0 = wb[0], w1 = wb[1], w2 = wb[2], w3 = wb[3];
    float m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = cm[i];
    const float* src = bayer + (size_t)n * 4 * hw;
    float* dst = out + (size_t)n * 3 * hw;
    const double ig = (double)inv_gamma;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (size_t)gridDim.x * 256) {
        const float c0 = fminf(fmaxf(src[i] * w0, 0.f), 1.f), c1 = fminf(fmaxf(src[hw + i] * w1, 0.f), 1.f);
        const float c2 = fminf(fmaxf(src[2 * hw + i] * w2, 0.f), 1.f), c3 = fminf(fmaxf(src[3 * hw + i] * w3, 0.f), 1.f);
        const float r = c0, g = (c1 + c3) / 2.0f, b = c2;
        isp_rgb_out(r, g, b, m, dst, i, hw, inv_gamma, ig, crf_E, crf_f, crf_n, gtab, s_t);
    }
}

// X-Trans (eld_isp_process_xtrans): one packed pixel = one 3x3 mosaic block, nine planes.  Gains by plane colour (xtrans.h xt_colour)
// -> clamp -> per colour its planes summed in ascending plane order in float32 (R = p0 + p3, G = (((p1 + p5) + p6) + p7) + p8,
// B = p2 + p4) and divided by the plane count (2 / 5 / 2) -> the shared tail.  36 B read + 12 B written per packed pixel.
// planes of colour col among planes 0 .. k-1 (k = 9: the plane count of the colour)
__host__ __device__ constexpr int xt_planes_before(int k, uint32_t col) { return k == 0 ? 0 : xt_planes_before(k - 1, col) + (xt_colour(k - 1) == col ? 1 : 0); }

__global__ __launch_bounds__(256) void isp_xtrans_kernel(const float* __restrict__ packed, const float* __restrict__ wbs, const float* __restrict__ ccms,
                                                         float* __restrict__ out, size_t hw, float inv_gamma, const float* __restrict__ crf_E,
                                                         const float* __restrict__ crf_f, int crf_n, int gtab) {
    __shared__ unsigned s_t[256];
    if (gtab) s_t[threadIdx.x] = ELD_GAMMA22_T[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.y;
    const float wc[3] = {wbs[3 * n], wbs[3 * n + 1], wbs[3 * n + 2]};
    const float* cm = ccms + 9 * n;
    float m[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) m[i] = cm[i];
    const float* src = packed + (size_t)n * 9 * hw;
    float* dst = out + (size_t)n * 3 * hw;
    const double ig = (double)inv_gamma;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < hw; i += (size_t)gridDim.x * 256) {
        float sum[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const uint32_t col = xt_colour(k);
            const float v = fminf(fmaxf(src[k * hw + i] * wc[col], 0.f), 1.f);
            sum[col] = xt_planes_before(k, col) == 0 ? v : sum[col] + v;
        }
        const float r = sum[0] / (float)xt_planes_before(9, 0), g = sum[1] / (float)xt_planes_before(9, 1), b = sum[2] / (float)xt_planes_before(9, 2);
        isp_rgb_out(r, g, b, m, dst, i, hw, inv_gamma, ig, crf_E, crf_f, crf_n, gtab, s_t);
    }
}

inline size_t qa_tiles(int H, int W) { return (size_t)((W - HALO + QA_TW - 1) / QA_TW) * ((H - HALO + QA_TH - 1) / QA_TH); }
inline size_t qa_items(int H, int W) { return (size_t)((W + 63) / 64) * ((H + QA_RH - 1) / QA_RH); }      // upper bound (64-column strips); strips over ALL columns / rows: every pixel has an owner
// test / A-B hooks (eld_debug_kernel_mask, env ELD_DEBUG_KERNEL_MASK): bit 6 (64) = the round-2 tile kernels, bit 5 (32) = one window column per
// lane (64-column strips) instead of two -- tests/test_model_gpu.py runs the oracle comparison under all three
int qa_use_tiles() { return (debug_kernel_mask(-1) & 64) != 0; }
int qa_cols() { return (debug_kernel_mask(-1) & 32) ? 1 : 2; }
}  // namespace

extern "C" size_t eld_quality_assess_workspace_bytes(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || H < WIN || W < WIN) return 0;
    const size_t tiles = ((size_t)N * RED_BLOCKS + (size_t)N * C * qa_tiles(H, W)) * sizeof(double);      // tile kernels (ELD_QA_TILES=1)
    const size_t fused = (size_t)2 * N * C * qa_items(H, W) * sizeof(double);                                // qa_fused_kernel: S and squared-error partials
    return tiles > fused ? tiles : fused;
}

static int quality_assess_impl(const float* est, const float* ref, double* out, void* ws, size_t ws_bytes, int N, int C, int H, int W,
                               float mul, float data_range, void* stream) {
    if (N == 0) return 0;
    if (!est || !ref || !out || !ws || N < 0 || C < 1 || H < WIN || W < WIN || !(data_range > 0.f)) return ELD_EINVAL;
    if (ws_bytes < eld_quality_assess_workspace_bytes(N, C, H, W)) return ELD_EWS;
    hipStream_t st = as_stream(stream);
    const size_t chw_ = (size_t)C * H * W;
    if (!qa_use_tiles() && (long long)N * C <= 65535) {
        const int nc = qa_cols();
        const int strips = (W + 64 * nc - 1) / (64 * nc), chunks = (H + QA_RH - 1) / QA_RH;
        const size_t items = (size_t)strips * chunks;
        double* ssp = (double*)ws;
        double* sqp = ssp + (size_t)N * C * items;
        if (nc == 2) { ELD_LAUNCH(qa_fused_kernel<2>, dim3((unsigned)((items + 3) / 4), N * C), dim3(256), 0, st, est, ref, ssp, sqp, H, W, strips, chunks, mul, data_range); }
        else { ELD_LAUNCH(qa_fused_kernel<1>, dim3((unsigned)((items + 3) / 4), N * C), dim3(256), 0, st, est, ref, ssp, sqp, H, W, strips, chunks, mul, data_range); }
        ELD_LAUNCH_CHECK();
        ELD_LAUNCH(qa_final2_kernel, dim3(N), dim3(256), 0, st, ssp, sqp, out, C, (int)items, chw_, (size_t)(H - HALO) * (W - HALO), data_range);
        ELD_LAUNCH_CHECK();
        return 0;
    }
    double* sq = (double*)ws;
    double* ss = sq + (size_t)N * RED_BLOCKS;
    const int tiles_x = (W - HALO + QA_TW - 1) / QA_TW, tiles_y = (H - HALO + QA_TH - 1) / QA_TH;
    const size_t chw = (size_t)C * H * W;
    ELD_LAUNCH(sqerr_kernel, dim3(RED_BLOCKS, N), dim3(256), 0, st, est, ref, sq, chw, mul, data_range);
    ELD_LAUNCH_CHECK();
    ELD_LAUNCH(ssim_kernel, dim3(tiles_x * tiles_y, N * C), dim3(256), 0, st, est, ref, ss, H, W, tiles_x, tiles_y, mul, data_range);
    ELD_LAUNCH_CHECK();
    ELD_LAUNCH(qa_final_kernel, dim3(N), dim3(256), 0, st, sq, ss, out, C, tiles_x * tiles_y, chw, (size_t)(H - HALO) * (W - HALO), data_range);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_quality_assess(const float* est, const float* ref, double* out, void* ws, size_t ws_bytes, int N, int C, int H, int W,
                                  float data_range, void* stream) {
    return quality_assess_impl(est, ref, out, ws, ws_bytes, N, C, H, W, data_range, data_range, stream);
}

// the same on images that are ALREADY on the [0, data_range] scale (util/index.py:76-81 as its callers use it: quality_assess(X, Y) on
// tensor2im outputs): no x255 stage, values only clipped to [0, data_range] (a no-op for tensor2im outputs)
extern "C" int eld_quality_assess_images(const float* est, const float* ref, double* out, void* ws, size_t ws_bytes, int N, int C, int H, int W,
                                         float data_range, void* stream) {
    return quality_assess_impl(est, ref, out, ws, ws_bytes, N, C, H, W, 1.0f, data_range, stream);
}

extern "C" size_t eld_illuminance_correct_workspace_bytes(int N) { return N < 1 ? 0 : (size_t)N * RED_BLOCKS * 2 * sizeof(double) + (size_t)N * sizeof(float); }

extern "C" int eld_illuminance_correct(const float* predict, const float* source, float* out, void* ws, size_t ws_bytes, int N, int source_N,
                                       size_t chw, void* stream) {
    if (N == 0) return 0;
    if (!predict || !source || !out || !ws || N < 0 || chw == 0 || (source_N != N && source_N != 1)) return ELD_EINVAL;
    if (ws_bytes < eld_illuminance_correct_workspace_bytes(N)) return ELD_EWS;
    hipStream_t st = as_stream(stream);
    double* part = (double*)ws;
    float* alpha = (float*)(part + (size_t)N * RED_BLOCKS * 2);
    const bool vec = chw % 4 == 0 && (((uintptr_t)predict | (uintptr_t)source | (uintptr_t)out) & 15) == 0;      // (then every image plane is 16-byte aligned too)
    const size_t sstride = source_N == 1 ? (size_t)0 : chw;
    if (vec) { ELD_LAUNCH(illum_dot_kernel<true>, dim3(RED_BLOCKS, N), dim3(256), 0, st, predict, source, part, chw, sstride); }
    else { ELD_LAUNCH(illum_dot_kernel<false>, dim3(RED_BLOCKS, N), dim3(256), 0, st, predict, source, part, chw, sstride); }
    ELD_LAUNCH_CHECK();
    ELD_LAUNCH(illum_alpha_kernel, dim3(N), dim3(256), 0, st, part, alpha);
    ELD_LAUNCH_CHECK();
    if (vec) { ELD_LAUNCH(illum_scale_kernel<true>, dim3(1024, N), dim3(256), 0, st, predict, alpha, out, chw); }
    else { ELD_LAUNCH(illum_scale_kernel<false>, dim3(1024, N), dim3(256), 0, st, predict, alpha, out, chw); }
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_isp_process(const float* bayer, const float* wbs, const float* ccms, float* out, int N, int H, int W, float gamma,
                               const float* crf_E, const float* crf_f, int crf_n, void* stream) {
    if (N == 0) return 0;
    if (!bayer || !wbs || !ccms || !out || N < 0 || H < 1 || W < 1 || !(gamma > 0.f)) return ELD_EINVAL;
    if (crf_n != 0 && (crf_n < 2 || !crf_E || !crf_f)) return ELD_EINVAL;
    const size_t hw = (size_t)H * W;
    const unsigned bx = (unsigned)((hw + 255) / 256 < 2048 ? (hw + 255) / 256 : 2048);
    const int gtab = (crf_n == 0 && gamma == 2.2f) ? 1 : 0;
    ELD_LAUNCH(isp_kernel, dim3(bx, N), dim3(256), 0, as_stream(stream), bayer, wbs, ccms, out, hw, (float)(1.0 / (double)gamma), crf_E, crf_f, crf_n, gtab);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_isp_process_xtrans(const float* packed, const float* wbs, const float* ccms, float* out, int N, int H, int W, float gamma,
                                      const float* crf_E, const float* crf_f, int crf_n, void* stream) {
    if (N == 0) return 0;
    if (!packed || !wbs || !ccms || !out || N < 0 || H < 1 || W < 1 || !(gamma > 0.f)) return ELD_EINVAL;
    if (crf_n != 0 && (crf_n < 2 || !crf_E || !crf_f)) return ELD_EINVAL;
    const size_t hw = (size_t)H * W;
    const unsigned bx = (unsigned)((hw + 255) / 256 < 2048 ? (hw + 255) / 256 : 2048);
    const int gtab = (crf_n == 0 && gamma == 2.2f) ? 1 : 0;
    ELD_LAUNCH(isp_xtrans_kernel, dim3(bx, N), dim3(256), 0, as_stream(stream), packed, wbs, ccms, out, hw, (float)(1.0 / (double)gamma), crf_E, crf_f, crf_n,
               gtab);
    ELD_LAUNCH_CHECK();
    return 0;
}
