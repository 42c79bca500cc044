// framepool.hip -- the device-resident frame pool: cut B patches out of uint16 sensor mosaics that stay in HBM and emit the uint16 codes
// the reference's patch databases hold (util/lmdb_data.py:24-98 pack, :201-210 ratio -> clip -> * 65535 -> astype(uint16)), bit for bit.
//
//   Bayer   (float32 throughout)            p = clip((float(u) - black_k) / (white - black_k), 0, 1)
//                                           p = clip(fl32(p * ratio), 0, 1);  code = trunc(fl32(p * 65535))
//   X-Trans (the reference packs into a     p = the same float32 value (one black level), widened to float64
//            float64 array, :62)            code = trunc(clip(p * double(ratio), 0, 1) * 65535.0)      float64 products
//
// Streaming: 2 B read and 2 B written per packed value.  A patch is a blockIdx.y slice, so the record (frame, y0, x0, ratio) and the frame's
// table entry are wave-uniform and live in SGPRs.  VEC (pw % 8 == 0): a lane owns 8 consecutive packed columns of one packed row and
// writes one 16-byte store per plane; its mosaic rows arrive as 16-byte loads when the record's alignment allows it and as 4-byte loads
// otherwise -- chosen per patch, so the choice is wave-uniform.  Any other patch width takes the one-lane-per-code kernel.
//
// The kernels never read outside the pool: a record whose frame index, offsets or frame entry do not describe a patch inside a frame
// inside the pool is SKIPPED (its output slice is left as it was).  The Python layer refuses such records before upload.
#include "common.h"
#include "xtrans.h"

namespace {

struct CropBayerArgs { int plane[4]; float black[4], denom[4]; };      // per 2x2 cell position (row-major): packed plane and its constants

struct Patch { const uint16_t* src; int Hm, Wm, y0, x0; float ratio; bool ok, wide; };

// CELL: mosaic pixels per packed pixel and side (Bayer 2, X-Trans 3).  Everything here is uniform over the block.
template <int CELL>
__device__ __forceinline__ Patch load_patch(const uint16_t* __restrict__ pool, size_t pool_elems, const EldPoolFrame* __restrict__ frames, int F,
                                            const EldCropRecord* __restrict__ recs, int ph, int pw) {
    Patch p;
    const EldCropRecord r = recs[blockIdx.y];
    p.ok = false; p.wide = false; p.src = pool; p.Hm = p.Wm = 0; p.y0 = r.y0; p.x0 = r.x0; p.ratio = r.ratio;
    if (r.frame < 0 || r.frame >= F) return p;
    const EldPoolFrame f = frames[r.frame];
    if (f.Hm < 2 || f.Wm < 2 || (f.Wm & 1) || (f.offset & 1)) return p;          // 4-byte loads: even row pitch and frame start
    const uint64_t area = (uint64_t)f.Hm * (uint64_t)f.Wm;
    if (f.offset > pool_elems || area > pool_elems - f.offset) return p;
    const int hp = CELL == 2 ? f.Hm / 2 : 2 * (f.Hm / 6), wp = CELL == 2 ? f.Wm / 2 : 2 * (f.Wm / 6);      // the frame's packed extent
    if (r.y0 < 0 || r.x0 < 0 || ph > hp || pw > wp || r.y0 > hp - ph || r.x0 > wp - pw) return p;
    p.src = pool + f.offset; p.Hm = f.Hm; p.Wm = f.Wm;
    // 16-byte loads: every row segment a lane reads starts on a 16-byte boundary (the pool base is 16-byte aligned: checked by the entry)
    p.wide = ((f.offset + (uint64_t)(CELL * r.x0)) & 7) == 0 && (f.Wm & 7) == 0;
    p.ok = true;
    return p;
}

__device__ __forceinline__ float norm32(uint32_t u, float black, float denom) {
    return fminf(fmaxf(__fdiv_rn(__fsub_rn((float)u, black), denom), 0.f), 1.f);
}
__device__ __forceinline__ uint32_t code_f32(uint32_t u, float black, float denom, float ratio) {
    const float p = fminf(fmaxf(__fmul_rn(norm32(u, black, denom), ratio), 0.f), 1.f);
    return (uint32_t)__fmul_rn(p, 65535.f);
}
__device__ __forceinline__ uint32_t code_f64(uint32_t u, float black, float denom, double ratio) {
    const double p = fmin(fmax(__dmul_rn((double)norm32(u, black, denom), ratio), 0.0), 1.0);
    return (uint32_t)__dmul_rn(p, 65535.0);
}

// N32 32-bit words starting at the 4-byte aligned s; WIDE: as 16-byte loads (s is 16-byte aligned then, N32 a multiple of 4)
template <int N32>
__device__ __forceinline__ void load_words(const uint16_t* s, bool wide, uint32_t* w) {
    if (wide) {
#pragma unroll
        for (int q = 0; q < N32 / 4; ++q) {
            const uint4 v = reinterpret_cast<const uint4*>(s)[q];
            w[4 * q] = v.x; w[4 * q + 1] = v.y; w[4 * q + 2] = v.z; w[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int q = 0; q < N32; ++q) w[q] = reinterpret_cast<const uint32_t*>(s)[q];
    }
}

__device__ __forceinline__ void store8(uint16_t* o, const uint32_t* c) {
    *reinterpret_cast<uint4*>(o) = make_uint4(c[0] | (c[1] << 16), c[2] | (c[3] << 16), c[4] | (c[5] << 16), c[6] | (c[7] << 16));
}

// ---- Bayer ----------------------------------------------------------------------------------------------------------------------
// VEC: lane -> packed row y, columns 8g..8g+7: mosaic rows 2(y0+y), 2(y0+y)+1, columns 2(x0+8g).. +15 (32 bytes each)
template <bool VEC>
__global__ __launch_bounds__(256) void crop_bayer_kernel(const uint16_t* __restrict__ pool, size_t pool_elems, const EldPoolFrame* __restrict__ frames, int F,
                                                         const EldCropRecord* __restrict__ recs, int ph, int pw, CropBayerArgs a, uint16_t* __restrict__ out) {
    const Patch p = load_patch<2>(pool, pool_elems, frames, F, recs, ph, pw);
    if (!p.ok) return;
    const size_t hw = (size_t)ph * pw;
    uint16_t* dst = out + (size_t)blockIdx.y * 4 * hw;
    const uint32_t wq = VEC ? pw / 8 : pw, total = (uint32_t)ph * wq;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const uint32_t y = i / wq, x = (VEC ? 8 : 1) * (i - y * wq);
        const uint16_t* s = p.src + (size_t)(2 * (p.y0 + (int)y)) * p.Wm + 2 * (p.x0 + (int)x);
        if (VEC) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                uint32_t w[8];
                load_words<8>(s + (size_t)r * p.Wm, p.wide, w);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int k = 2 * r + c;
                    uint32_t code[8];
#pragma unroll
                    for (int t = 0; t < 8; ++t) code[t] = code_f32(c ? w[t] >> 16 : w[t] & 0xffffu, a.black[k], a.denom[k], p.ratio);
                    store8(dst + (size_t)a.plane[k] * hw + (size_t)y * pw + x, code);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(s + (size_t)r * p.Wm);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int k = 2 * r + c;
                    dst[(size_t)a.plane[k] * hw + (size_t)y * pw + x] = (uint16_t)code_f32(c ? w >> 16 : w & 0xffffu, a.black[k], a.denom[k], p.ratio);
                }
            }
        }
    }
}

// ---- X-Trans --------------------------------------------------------------------------------------------------------------------
// VEC: lane -> packed row i (absolute iy = y0 + i), columns 8g..8g+7 (absolute jx = x0 + 8g): the 3 x 24 mosaic block at row 3 iy, column
// 3 jx feeds all nine planes.  Plane c < 5 reads cell position XT_RC[c][iy & 1][j & 1]: with XPAR = x0 & 1 (uniform over the patch, 8g is
// even) and PI = iy & 1 every index below is a compile-time constant.  XPAR == 1: 3 jx is odd, so the row segment starts one code early
// (4-byte aligned) and the block's last code, which that shift pushes out of the 12 words, is a 2-byte load of its own.
template <int XPAR, int PI>
__device__ __forceinline__ void xtrans_lane(const uint16_t* s, int Wm, bool wide, float black, float denom, double ratio, uint16_t* o, size_t hw) {
    uint32_t w[3][13];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const uint16_t* row = s + (size_t)d * Wm;
        if (XPAR) {
            load_words<12>(row - 1, false, w[d]);
            w[d][12] = row[23];
        } else {
            load_words<12>(row, wide, w[d]);
            w[d][12] = 0;
        }
    }
#pragma unroll
    for (int c = 0; c < 9; ++c) {
        uint32_t code[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int pj = (XPAR + t) & 1;
            const int d = c < 5 ? XT_RC[c][PI][pj][0] - 3 * PI : XT_RC3[c - 5][0];
            const int e = 3 * t + (c < 5 ? XT_RC[c][PI][pj][1] - 3 * pj : XT_RC3[c - 5][1]) + XPAR;      // index into the loaded row segment
            const uint32_t u = (e & 1) ? w[d][e >> 1] >> 16 : w[d][e >> 1] & 0xffffu;
            code[t] = code_f64(u, black, denom, ratio);
        }
        store8(o + (size_t)c * hw, code);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void crop_xtrans_kernel(const uint16_t* __restrict__ pool, size_t pool_elems, const EldPoolFrame* __restrict__ frames, int F,
                                                          const EldCropRecord* __restrict__ recs, int ph, int pw, float black, float denom,
                                                          uint16_t* __restrict__ out) {
    const Patch p = load_patch<3>(pool, pool_elems, frames, F, recs, ph, pw);
    if (!p.ok) return;
    const size_t hw = (size_t)ph * pw;
    uint16_t* dst = out + (size_t)blockIdx.y * 9 * hw;
    const double ratio = (double)p.ratio;
    if (VEC) {
        const uint32_t wq = pw / 8, total = (uint32_t)ph * wq;
        const bool xpar = p.x0 & 1;
        for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
            const uint32_t y = i / wq, x = 8 * (i - y * wq);
            const int iy = p.y0 + (int)y, jx = p.x0 + (int)x;
            const uint16_t* s = p.src + (size_t)(3 * iy) * p.Wm + 3 * jx;
            uint16_t* o = dst + (size_t)y * pw + x;
            if (xpar) {
                if (iy & 1) xtrans_lane<1, 1>(s, p.Wm, false, black, denom, ratio, o, hw);
                else xtrans_lane<1, 0>(s, p.Wm, false, black, denom, ratio, o, hw);
            } else {
                if (iy & 1) xtrans_lane<0, 1>(s, p.Wm, p.wide, black, denom, ratio, o, hw);
                else xtrans_lane<0, 0>(s, p.Wm, p.wide, black, denom, ratio, o, hw);
            }
        }
    } else {                                   // one lane per code; the index map as pack_raw_xtrans_kernel states it
        const size_t total = 9 * hw;
        for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
            const int c = (int)(e / hw);
            const int r = (int)(e - (size_t)c * hw);
            const int i = r / pw + p.y0, j = r % pw + p.x0;
            int row, col;
            if (c < 5) { row = 6 * (i >> 1) + XT_RC[c][i & 1][j & 1][0]; col = 6 * (j >> 1) + XT_RC[c][i & 1][j & 1][1]; }
            else { row = 3 * i + XT_RC3[c - 5][0]; col = 3 * j + XT_RC3[c - 5][1]; }
            dst[e] = (uint16_t)code_f64(p.src[(size_t)row * p.Wm + col], black, denom, ratio);
        }
    }
}

// what the host can see: sizes, pointers and alignment (the records and the frame table are device memory)
bool crop_args_ok(const void* pool, size_t pool_elems, const void* frames, int F, int max_h, int max_w, const void* recs, int B, int ph, int pw,
                  const void* out) {
    if (F <= 0 || B <= 0 || B > 65535 || ph <= 0 || pw <= 0 || max_h <= 0 || max_w <= 0 || pool_elems == 0) return false;
    if (ph > max_h || pw > max_w) return false;                              // larger than every frame
    if ((size_t)ph * (size_t)pw > (size_t)0x7fffffff / 9) return false;      // 32-bit work-item counts
    if (!pool || !frames || !recs || !out) return false;
    return ((uintptr_t)pool & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)frames & 7) == 0 && ((uintptr_t)recs & 3) == 0;
}

unsigned crop_grid_x(size_t items) { return (unsigned)min((items + 255) / 256, (size_t)4096); }

}  // namespace

extern "C" int eld_crop_pack_raw_bayer_u16(const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int max_h, int max_w,
                                           const EldCropRecord* recs, int B, int ph, int pw, const int* raw_pattern, const float* black_level,
                                           float white_point, uint16_t* out, void* stream) {
    if (!raw_pattern || !black_level || !crop_args_ok(pool, pool_elems, frames, F, max_h, max_w, recs, B, ph, pw, out)) return ELD_EINVAL;
    if (!bayer_permutation(raw_pattern)) return ELD_EINVAL;
    CropBayerArgs a;
    for (int i = 0; i < 4; ++i) {
        const int k = raw_pattern[i];
        if (!(black_level[k] >= 0.f) || !(white_point > black_level[k]) || !(white_point <= 65535.f)) return ELD_EINVAL;
        a.plane[i] = k; a.black[i] = black_level[k]; a.denom[i] = white_point - black_level[k];
    }
    const bool vec = pw % 8 == 0;
    dim3 grid(crop_grid_x((size_t)ph * (vec ? pw / 8 : pw)), B);
    if (vec) ELD_LAUNCH(crop_bayer_kernel<true>, grid, dim3(256), 0, as_stream(stream), pool, pool_elems, frames, F, recs, ph, pw, a, out);
    else ELD_LAUNCH(crop_bayer_kernel<false>, grid, dim3(256), 0, as_stream(stream), pool, pool_elems, frames, F, recs, ph, pw, a, out);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_crop_pack_raw_xtrans_u16(const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int max_h, int max_w,
                                            const EldCropRecord* recs, int B, int ph, int pw, float black_level, float white_point, uint16_t* out,
                                            void* stream) {
    if (!crop_args_ok(pool, pool_elems, frames, F, max_h, max_w, recs, B, ph, pw, out)) return ELD_EINVAL;
    if (!(black_level >= 0.f) || !(white_point > black_level) || !(white_point <= 65535.f)) return ELD_EINVAL;
    const bool vec = pw % 8 == 0;
    dim3 grid(crop_grid_x(vec ? (size_t)ph * (pw / 8) : (size_t)9 * ph * pw), B);
    const float denom = white_point - black_level;
    if (vec) ELD_LAUNCH(crop_xtrans_kernel<true>, grid, dim3(256), 0, as_stream(stream), pool, pool_elems, frames, F, recs, ph, pw, black_level, denom, out);
    else ELD_LAUNCH(crop_xtrans_kernel<false>, grid, dim3(256), 0, as_stream(stream), pool, pool_elems, frames, F, recs, ph, pw, black_level, denom, out);
    ELD_LAUNCH_CHECK();
    return 0;
}
