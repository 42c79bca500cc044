// unet_wide.hip -- the two ends of the U-Net for more than 4 planes (X-Trans: 9; burst inputs: 4 x num_burst), gfx950.
//   * conv10_1 (1x1, 32 -> OC) for 5 <= OC <= 16: forward, backward, the fused training head (output + L1 / MSE + head backward in one
//     pass) and the fixed-order reduction of its 33 * OC partial sums.  The OC <= 4 head (unet_misc.hip, one plane per lane of a quad)
//     is not touched: the launchers there hand OC > 4 to this file.
//   * the bf16 network's input for 5 <= Cin <= 16: NCHW fp32 planes -> NHWC 32-channel bf16 (zero padded), the operand of the generic
//     bf16 3x3 conv / weight gradient (their bf16 K granule is 32 channels).
// Reference ops: models/arch/Unet.py:46,88 (conv10_1), models/losses.py:30-34 (L1Loss / MSELoss), models/ELD_model.py:377-391
// (arch.unet(opt.channels, opt.channels): 9 -> 9 for X-Trans).
#include "unet_misc.h"

// ------------------------------------------------------------------------------------------------
// Wide head.  Eight lanes per pixel, four channels each (fp32: 16 B per lane; bf16: 8 B per lane -- four channels for bf16 too, so that
// w[o][4 channels] and dW[o][4 channels] of all OCP planes fit beside each other: 2 * 4 * OCP = 128 registers at OCP = 16).
// Forward: every lane forms the partial dot products of its 4 channels for all OCP planes (fma chains), then a REDUCE-SCATTER over the
// pixel's 8 lanes (xor 4, 2, 1: each step hands half of the values to the partner and adds the other half) leaves lane r with the full
// sums of planes PPL r .. PPL r + PPL - 1 (PPL = OCP / 8).  14 moves at OCP = 16 instead of the 48 of a butterfly per plane.
// Backward: lane r reads / derives the output gradient of its own planes; an ALL-GATHER (xor 1, 2, 4) hands every lane all OCP of them.
// Moves: xor 1 / xor 2 are quad-permute DPP (no LDS), xor 4 is ds_swizzle in bitmask mode (no LDS memory, no address register).
// The inference forward and the fused training forward run the same code for the output: same bits.
// OCP = 8 serves OC 5..8, OCP = 16 serves OC 9..16; planes >= OC have zero weights and are neither read nor written.
// ------------------------------------------------------------------------------------------------
#define HEAD_WIDE_BLOCKS 1024
enum { HW_FWD = 0, HW_L1 = 1, HW_MSE = 2, HW_BWD = 3 };

template <int M>
__device__ __forceinline__ float lane_xor(float v) {
    const int i = __float_as_int(v);
    if constexpr (M == 1) return __int_as_float(__builtin_amdgcn_update_dpp(0, i, 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]
    else if constexpr (M == 2) return __int_as_float(__builtin_amdgcn_update_dpp(0, i, 0x4E, 0xF, 0xF, true)); // quad_perm [2,3,0,1]
    else return __int_as_float(__builtin_amdgcn_ds_swizzle(i, 0x101F));                                       // and 0x1F, xor 4
}

// one reduce-scatter step: K values in v[0..K), partner = lane ^ M; afterwards v[0..K/2) = the half this lane keeps, summed
template <int K, int M>
__device__ __forceinline__ void rs_step(float* v, bool up) {
#pragma unroll
    for (int i = 0; i < K / 2; ++i) {
        const float send = up ? v[i] : v[i + K / 2];
        const float keep = up ? v[i + K / 2] : v[i];
        v[i] = keep + lane_xor<M>(send);
    }
}
// one all-gather step: K values in v[0..K) -> 2K values (the lower lane of the pair holds the lower half)
template <int K, int M>
__device__ __forceinline__ void ag_step(float* v, bool up) {
    float t[K];
#pragma unroll
    for (int i = 0; i < K; ++i) t[i] = lane_xor<M>(v[i]);
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float lo = up ? t[i] : v[i], hi = up ? v[i] : t[i];
        v[i] = lo; v[i + K] = hi;
    }
}

template <typename T>
__device__ __forceinline__ void head_wide_load(const T* act, size_t pc, int r, float (&av)[4]) {
    float4 a;
    if constexpr (sizeof(T) == 4) a = reinterpret_cast<const float4*>(act + pc * 32)[r];
    else a = unpack_bf4(reinterpret_cast<const uint2*>(act + pc * 32)[r]);
    av[0] = a.x; av[1] = a.y; av[2] = a.z; av[3] = a.w;
}

// MODE HW_FWD: out = head(act).  HW_L1 / HW_MSE: the fused training head (src = target): out, loss partials, g = d(loss)/d(conv9_2 pre-act),
// dW / db partials.  HW_BWD: src = dout (NCHW, OC planes) -> g, dW / db partials.
// Partials: part[block][33 OC] = dW[o][c] at 32 o + c, db[o] at 32 OC + o; lpart[block] = the block's loss sum (training).
template <typename T, int OCP, int MODE>
__global__ __launch_bounds__(256) void head_wide_kernel(const T* __restrict__ act, const float* __restrict__ w, const float* __restrict__ b,
                                                        const float* __restrict__ src, float* __restrict__ out, T* __restrict__ g,
                                                        float* __restrict__ part, float* __restrict__ lpart, int N, size_t HW, int OC, float gscale) {
    constexpr int PPL = OCP / 8;                       // planes per lane after the reduce-scatter
    constexpr bool FWD = MODE != HW_BWD, BWD = MODE != HW_FWD;
    __shared__ float red[BWD ? 4 : 1][BWD ? 33 * OCP + 1 : 1];
    const int tid = threadIdx.x, r = tid & 7;
    const bool u4 = r & 4, u2 = r & 2, u1 = r & 1;
    float wq[OCP][4];                                  // w[o][4r + j]
#pragma unroll
    for (int o = 0; o < OCP; ++o)
#pragma unroll
        for (int j = 0; j < 4; ++j) wq[o][j] = o < OC ? w[o * 32 + 4 * r + j] : 0.f;
    float bo[PPL];
#pragma unroll
    for (int k = 0; k < PPL; ++k) bo[k] = (FWD && PPL * r + k < OC) ? b[PPL * r + k] : 0.f;
    float dw[BWD ? OCP : 1][4];
    float db[PPL], ls = 0.f;
#pragma unroll
    for (int o = 0; o < (BWD ? OCP : 1); ++o)
#pragma unroll
        for (int j = 0; j < 4; ++j) dw[o][j] = 0.f;
#pragma unroll
    for (int k = 0; k < PPL; ++k) db[k] = 0.f;
    const size_t total = (size_t)N * HW;
    const size_t stride = (size_t)gridDim.x * 32;
    size_t p = (size_t)blockIdx.x * 32 + (tid >> 3);
    const size_t iters = (total + stride - 1) / stride;               // every lane of a pixel group runs the same trip count (the exchanges need its mates)
    for (size_t itn = 0; itn < iters; ++itn, p += stride) {
        const bool ok = p < total;
        const size_t pc = ok ? p : total - 1;
        const size_t n = pc / HW, q = pc - n * HW;
        float av[4];
        head_wide_load<T>(act, pc, r, av);
        float v[OCP];                                  // forward: partial sums -> own planes' outputs; backward: own planes' gradients -> all
        if constexpr (FWD) {
#pragma unroll
            for (int o = 0; o < OCP; ++o) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) s = fmaf(av[j], wq[o][j], s);
                v[o] = s;
            }
            rs_step<OCP, 4>(v, u4);
            rs_step<OCP / 2, 2>(v, u2);
            rs_step<OCP / 4, 1>(v, u1);
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                const int o = PPL * r + k;
                const float y = v[k] + bo[k];
                float dl = 0.f;
                if (ok && o < OC) {
                    const size_t idx = (n * OC + o) * HW + q;
                    out[idx] = y;
                    if constexpr (MODE != HW_FWD) {
                        const float diff = y - src[idx];
                        ls += MODE == HW_MSE ? diff * diff : fabsf(diff);
                        dl = MODE == HW_MSE ? 2.0f * diff * gscale : (diff > 0.f ? gscale : (diff < 0.f ? -gscale : 0.f));
                    }
                }
                v[k] = dl;
            }
        } else {
#pragma unroll
            for (int k = 0; k < PPL; ++k) {
                const int o = PPL * r + k;
                v[k] = (ok && o < OC) ? src[(n * OC + o) * HW + q] : 0.f;
            }
        }
        if constexpr (BWD) {
#pragma unroll
            for (int k = 0; k < PPL; ++k) db[k] += v[k];
            ag_step<PPL, 1>(v, u1);
            ag_step<2 * PPL, 2>(v, u2);
            ag_step<4 * PPL, 4>(v, u4);
            if (!ok) continue;
            float gv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float s = 0.f;
#pragma unroll
                for (int o = 0; o < OCP; ++o) { s = fmaf(wq[o][j], v[o], s); dw[o][j] = fmaf(v[o], av[j], dw[o][j]); }
                gv[j] = s * lrelu_slope(av[j]);
            }
            if constexpr (sizeof(T) == 4) reinterpret_cast<float4*>(g + pc * 32)[r] = make_float4(gv[0], gv[1], gv[2], gv[3]);
            else reinterpret_cast<uint2*>(g + pc * 32)[r] = pack_bf4(make_float4(gv[0], gv[1], gv[2], gv[3]));
        }
    }
    if constexpr (BWD) {
        // block reduction in a fixed order: lanes sharing r (the 8 pixel groups of a wave) by xor-shuffles, then the 4 waves through LDS
        const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int o = 0; o < OCP; ++o)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float x = dw[o][j];
                for (int off = 8; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
                if (lane < 8 && o < OC) red[wave][o * 32 + 4 * lane + j] = x;
            }
#pragma unroll
        for (int k = 0; k < PPL; ++k) {
            float x = db[k];
            for (int off = 8; off < 64; off <<= 1) x += __shfl_xor(x, off, 64);
            if (lane < 8 && PPL * lane + k < OC) red[wave][32 * OC + PPL * lane + k] = x;
        }
        if constexpr (MODE != HW_BWD) {
            float l = ls;
            for (int off = 1; off < 64; off <<= 1) l += __shfl_xor(l, off, 64);
            if (lane == 0) red[wave][33 * OC] = l;
        }
        __syncthreads();
        const int S = 33 * OC;
        for (int t = tid; t < S; t += 256) part[(size_t)blockIdx.x * S + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
        if (MODE != HW_BWD && tid == 0) lpart[blockIdx.x] = red[0][S] + red[1][S] + red[2][S] + red[3][S];
    }
}

// 33 OC outputs, 16 lanes each over the per-block partials (stride 33 OC); fixed shuffle tree
__global__ __launch_bounds__(256) void head_wide_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int nblocks, int OC) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int S = 33 * OC;
    const int t = (blockIdx.x * 4 + wave) * 4 + (lane & 3), slice = lane >> 2;
    float s = 0.f;
    if (t < S)
        for (int bk = slice; bk < nblocks; bk += 16) s += part[(size_t)bk * S + t];
#pragma unroll
    for (int off = 4; off < 64; off <<= 1) s += __shfl_xor(s, off, 64);
    if (slice != 0 || t >= S) return;
    if (t < 32 * OC) dw[t] = s; else db[t - 32 * OC] = s;
}

// loss = inv_n * sum of the per-block loss partials, in a fixed order (double accumulation, as l1_reduce_kernel)
__global__ __launch_bounds__(256) void head_wide_loss_kernel(const float* __restrict__ lpart, float* __restrict__ loss, int nblocks, float inv_n) {
    __shared__ double sh[256];
    double s = 0.0;
    for (int bk = threadIdx.x; bk < nblocks; bk += 256) s += (double)lpart[bk];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(sh[0] * (double)inv_n);
}

size_t head_wide_bwd_ws_floats(int OC) { return (size_t)HEAD_WIDE_BLOCKS * 33 * OC; }
size_t head_wide_train_ws_floats(int OC) { return (size_t)HEAD_WIDE_BLOCKS * (33 * OC + 1); }
static int head_wide_blocks(size_t total) { return (int)min((total + 31) / 32, (size_t)HEAD_WIDE_BLOCKS); }

template <typename T, int MODE>
static int launch_wide(int grid, const T* act, const float* w, const float* b, const float* src, float* out, T* g, float* part, float* lpart,
                       int N, size_t HW, int OC, float gs, hipStream_t st) {
    if (OC <= 8) { ELD_LAUNCH((head_wide_kernel<T, 8, MODE>), dim3(grid), dim3(256), 0, st, act, w, b, src, out, g, part, lpart, N, HW, OC, gs); }
    else { ELD_LAUNCH((head_wide_kernel<T, 16, MODE>), dim3(grid), dim3(256), 0, st, act, w, b, src, out, g, part, lpart, N, HW, OC, gs); }
    ELD_LAUNCH_CHECK();
    return 0;
}

static int launch_wide_reduce(const float* part, float* dw, float* db, int nb, int OC, hipStream_t st) {
    ELD_LAUNCH(head_wide_reduce_kernel, dim3((33 * OC + 15) / 16), dim3(256), 0, st, part, dw, db, nb, OC);
    ELD_LAUNCH_CHECK();
    return 0;
}

int launch_head_wide_fwd(const void* act, int bf16, const float* w, const float* b, float* out, int N, int H, int W, int OC, hipStream_t st) {
    if (OC <= 4 || OC > 16) return ELD_EINVAL;
    const size_t total = (size_t)N * H * W;
    if (!total) return 0;
    const int grid = (int)min((total + 31) / 32, (size_t)16384);
    if (bf16) return launch_wide<bf16_t, HW_FWD>(grid, (const bf16_t*)act, w, b, nullptr, out, nullptr, nullptr, nullptr, N, (size_t)H * W, OC, 0.f, st);
    return launch_wide<float, HW_FWD>(grid, (const float*)act, w, b, nullptr, out, nullptr, nullptr, nullptr, N, (size_t)H * W, OC, 0.f, st);
}

int launch_head_wide_bwd(const float* dout, const void* act, int bf16, const float* w, void* g, float* dw, float* db, float* part,
                         int N, int H, int W, int OC, hipStream_t st) {
    if (OC <= 4 || OC > 16) return ELD_EINVAL;
    const size_t total = (size_t)N * H * W;
    if (!total) return 0;
    const int nb = head_wide_blocks(total);
    const int rc = bf16 ? launch_wide<bf16_t, HW_BWD>(nb, (const bf16_t*)act, w, nullptr, dout, nullptr, (bf16_t*)g, part, nullptr, N, (size_t)H * W, OC, 0.f, st)
                        : launch_wide<float, HW_BWD>(nb, (const float*)act, w, nullptr, dout, nullptr, (float*)g, part, nullptr, N, (size_t)H * W, OC, 0.f, st);
    if (rc) return rc;
    return launch_wide_reduce(part, dw, db, nb, OC, st);
}

// part: head_wide_train_ws_floats(OC) floats that must survive until launch_head_wide_train_reduce (the backward) has run
int launch_head_wide_train(const void* act, int bf16, const float* w, const float* b, const float* tgt, float* out, void* g, float* part, float* loss,
                           int N, int H, int W, int OC, int mse, float grad_scale, hipStream_t st) {
    if (OC <= 4 || OC > 16) return ELD_EINVAL;
    const size_t total = (size_t)N * H * W;
    if (!total) return ELD_EINVAL;
    const int nb = head_wide_blocks(total);
    float* lpart = part + (size_t)HEAD_WIDE_BLOCKS * 33 * OC;
    const float n = (float)(total * (size_t)OC);
    const float gs = grad_scale / n;
    const size_t HW = (size_t)H * W;
    int rc;
    if (bf16) rc = mse ? launch_wide<bf16_t, HW_MSE>(nb, (const bf16_t*)act, w, b, tgt, out, (bf16_t*)g, part, lpart, N, HW, OC, gs, st)
                       : launch_wide<bf16_t, HW_L1>(nb, (const bf16_t*)act, w, b, tgt, out, (bf16_t*)g, part, lpart, N, HW, OC, gs, st);
    else rc = mse ? launch_wide<float, HW_MSE>(nb, (const float*)act, w, b, tgt, out, (float*)g, part, lpart, N, HW, OC, gs, st)
                  : launch_wide<float, HW_L1>(nb, (const float*)act, w, b, tgt, out, (float*)g, part, lpart, N, HW, OC, gs, st);
    if (rc) return rc;
    ELD_LAUNCH(head_wide_loss_kernel, dim3(1), dim3(256), 0, st, lpart, loss, nb, 1.0f / n);
    ELD_LAUNCH_CHECK();
    return 0;
}

int launch_head_wide_train_reduce(const float* part, float* dw, float* db, int N, int H, int W, int OC, hipStream_t st) {
    if (OC <= 4 || OC > 16) return ELD_EINVAL;
    const size_t total = (size_t)N * H * W;
    if (!total) return 0;
    return launch_wide_reduce(part, dw, db, head_wide_blocks(total), OC, st);
}

// ------------------------------------------------------------------------------------------------
// NCHW fp32 (C <= 16 planes) -> NHWC 32-channel bf16, channels C..31 zero: conv1_1's operand in the bf16 network for C > 4.  One pixel
// per lane: C coalesced plane reads, four 16-byte writes.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nchw_to_nhwc32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, int N, int C, size_t HW) {
    const size_t total = (size_t)N * HW;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (size_t)gridDim.x * blockDim.x) {
        const size_t n = p / HW, q = p - n * HW;
        float v[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) v[c] = c < C ? x[(n * C + c) * HW + q] : 0.f;
        uint4* o = reinterpret_cast<uint4*>(y + p * 32);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const uint2 a = pack_bf4(make_float4(v[8 * k], v[8 * k + 1], v[8 * k + 2], v[8 * k + 3]));
            const uint2 c2 = pack_bf4(make_float4(v[8 * k + 4], v[8 * k + 5], v[8 * k + 6], v[8 * k + 7]));
            o[k] = make_uint4(a.x, a.y, c2.x, c2.y);
        }
        o[2] = make_uint4(0u, 0u, 0u, 0u);
        o[3] = make_uint4(0u, 0u, 0u, 0u);
    }
}

int launch_nchw_to_nhwc32_bf16(const float* x, bf16_t* y, int N, int C, int H, int W, hipStream_t st) {
    if (C < 1 || C > 16) return ELD_EINVAL;
    const size_t total = (size_t)N * H * W;
    if (!total) return 0;
    ELD_LAUNCH(nchw_to_nhwc32_bf16_kernel, dim3((unsigned)min((total + 255) / 256, (size_t)16384)), dim3(256), 0, st, x, y, N, C, (size_t)H * W);
    ELD_LAUNCH_CHECK();
    return 0;
}
