// hist.hip -- exact integer histograms of sensor codes and of sampler output (eld_amd/validate.py).
//
//   eld_hist_u16   uint16 mosaics [F,Hm,Wm] (optionally minus a second stack) -> counts[F][G][2R+1], per colour group of a period-2 or -6 cell
//   eld_hist_f32   float32 planes [N,C,H,W] quantised as rintf(x * scale[n]) (optionally minus a second tensor's) -> counts[N][G][2R+1]
//
// One pass over the pixels, 16 bytes per lane where the alignment allows.  Layout of the counters (the "replicated LDS" layout):
//   * a workgroup (512 threads) keeps NC copies of its table of uint32 counters in LDS (u16: G x B counters, f32: the B counters of its plane's
//     group); thread t adds to copy t % NC with ds_add_u32.  The copy stride is 1 modulo 32 words, so the same bin of the NC copies lies in NC
//     different banks: on a constant frame (every lane in one bin) a 32-lane group meets 32 / NC-way serialisation instead of 32-way.
//     NC = min(16, 72 KiB / table): two workgroups per CU.  A table between 72 and 152 KiB runs with one copy and one workgroup per CU.
//   * a table larger than that (R beyond ~4800 with four groups) has no LDS stage: the lanes add to the uint64 counts in global memory.
//   * at the end a workgroup folds its copies and adds every non-zero counter to counts[] with a 64-bit global integer atomic; counts[] is
//     zeroed by a kernel of this call first.  Integer adds only: any arrival order gives the same bits.
// LDS counters cannot wrap: a workgroup adds one per pixel it reads, all of one frame (plane), and the host refuses Hm * Wm >= 2^31 (H * W).
// The group of a pixel comes from a per-row 64-bit word of 4-bit codes (group + 1, 0 = not counted) shifted by the column phase, the defect
// bit from one 32-bit word of the bitmap per 16-byte load: neither needs a pass of its own.
#include "mosaic_dev.h"

namespace {

constexpr int HT = 512;                          // threads per workgroup
constexpr int H_LDS_SHARED = 72 * 1024;          // budget of the replicated layout (two workgroups per CU)
constexpr int H_LDS_SINGLE = 152 * 1024;         // one copy, one workgroup per CU
constexpr int H_MAX_COPIES = 16;
constexpr float Q_LIM = 536870912.0f;            // 2^29: q saturates here, so q(x) - q(x2) + R stays inside int32

struct HistU16Args {
    const uint16_t* u;
    const uint16_t* v;
    const uint32_t* bitmap;
    uint64_t* counts;
    int Hm, Wm, G, R, B, wpr;
    uint32_t cpr, nchunks;                       // chunks per row, per frame
    FastDiv dcpr;
    int nc, stride;
    int centre[4];
    uint64_t roww[6];                            // row class r: 12 codes of 4 bits, code k = group[r*p + k % p] + 1
};

struct HistF32Args {
    const float* x;
    const float* x2;
    const float* scale;
    uint64_t* counts;
    int C, G, R, B;
    uint32_t hw;
    int nc, stride;
    signed char grp[64];
};

extern __shared__ uint32_t h_lds[];

__device__ __forceinline__ void lds_clear(int words) {
    for (int i = threadIdx.x; i < words; i += HT) h_lds[i] = 0;
    __syncthreads();
}

// fold the copies and add the non-zero counters to out[0 .. tw)
__device__ __forceinline__ void lds_flush(int tw, int nc, int stride, uint64_t* __restrict__ out) {
    __syncthreads();
    for (int i = threadIdx.x; i < tw; i += HT) {
        uint32_t s = 0;
        for (int c = 0; c < nc; ++c) s += h_lds[c * stride + i];   // <= the pixels of the workgroup < 2^31: no wrap
        if (s) atomicAdd(reinterpret_cast<unsigned long long*>(out + i), (unsigned long long)s);
    }
}

template <bool GLOBAL>
__device__ __forceinline__ void hist_add(uint32_t* __restrict__ lds, uint64_t* __restrict__ glob, int idx) {
    if (GLOBAL) atomicAdd(reinterpret_cast<unsigned long long*>(glob + idx), 1ull);
    else atomicAdd(lds + idx, 1u);
}

// NPX pixels per chunk: 8 (one 16-byte load; Wm % 8 == 0, 16-byte aligned stacks) or 2 (one 32-bit word).  Chunk i of a frame lies at
// element i * NPX of it: chunks never straddle a row.
template <int P, int NPX, bool GLOBAL>
__global__ __launch_bounds__(HT) void hist_u16_kernel(HistU16Args a) {
    __shared__ uint64_t s_roww[6];
    constexpr int NW = NPX / 2;
    const int f = blockIdx.y;
    if (threadIdx.x < 6) s_roww[threadIdx.x] = a.roww[threadIdx.x];
    if (!GLOBAL) lds_clear(a.nc * a.stride);
    else __syncthreads();
    uint32_t* tab = h_lds + (GLOBAL ? 0 : (int)(threadIdx.x % (unsigned)a.nc) * a.stride);
    uint64_t* out = a.counts + (size_t)f * a.G * a.B;
    const size_t fo = (size_t)f * a.Hm * a.Wm;
    const uint32_t* uw = reinterpret_cast<const uint32_t*>(a.u + fo);
    const uint32_t* vw = a.v ? reinterpret_cast<const uint32_t*>(a.v + fo) : nullptr;
    const int c0 = a.centre[0], c1 = a.centre[1], c2 = a.centre[2], c3 = a.centre[3];
    const int R = a.R, B = a.B;

    auto load = [&](const uint32_t* __restrict__ base, uint32_t i, uint32_t (&w)[NW]) __attribute__((always_inline)) {
        if constexpr (NPX == 8) {
            const uint4 q = reinterpret_cast<const uint4*>(base)[i];
            w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
        } else {
            w[0] = base[i];
        }
    };
    auto bin_chunk = [&](uint32_t i, const uint32_t (&wu)[NW], const uint32_t (&wv)[NW]) __attribute__((always_inline)) {
        const uint32_t y = fdiv_u32(i, a.dcpr);
        const uint32_t x0 = (i - y * a.cpr) * NPX;
        const uint32_t rm = cell_phase<P>(y);
        const uint32_t cm = P == 2 ? 0u : mod6(x0);
        const uint64_t rw = s_roww[rm] >> (4u * cm);
        uint32_t bad = 0;
        if (a.bitmap) bad = defect_bits(a.bitmap, a.wpr, y, x0);
#pragma unroll
        for (int j = 0; j < NPX; ++j) {
            const int code = (int)code_of(wu, j);
            const int nib = (int)((uint32_t)(rw >> (4 * j)) & 15u);
            if (nib != 0 && !((bad >> j) & 1u)) {
                const int g = nib - 1;
                const int sub = vw ? (int)code_of(wv, j) : (g == 0 ? c0 : g == 1 ? c1 : g == 2 ? c2 : c3);
                const int b = min(max(code - sub + R, 0), 2 * R);
                hist_add<GLOBAL>(tab, out, g * B + b);
            }
        }
    };

    const uint32_t step = gridDim.x * HT;
    uint32_t i = blockIdx.x * HT + threadIdx.x;
    for (; i < a.nchunks && i + step < a.nchunks; i += 2 * step) {   // two loads in flight per lane (i + step < 2^31: nchunks < 2^30)
        uint32_t wa[NW], wb[NW], va[NW] = {}, vb[NW] = {};
        load(uw, i, wa);
        load(uw, i + step, wb);
        if (vw) { load(vw, i, va); load(vw, i + step, vb); }
        bin_chunk(i, wa, va);
        bin_chunk(i + step, wb, vb);
    }
    if (i < a.nchunks) {
        uint32_t wa[NW], va[NW] = {};
        load(uw, i, wa);
        if (vw) load(vw, i, va);
        bin_chunk(i, wa, va);
    }
    if (!GLOBAL) lds_flush(a.G * B, a.nc, a.stride, out);
}

// q(t) = (int)clamp(rintf(t * s), -2^29, 2^29); a NaN product is not counted.  The product is one float32 multiply (no contraction: there
// is nothing to contract with, the subtraction and the + R are integer operations).
__device__ __forceinline__ bool quant(float t, float s, int& q) {
    const float p = __fmul_rn(t, s);
    q = (int)fminf(fmaxf(rintf(p), -Q_LIM), Q_LIM);
    return p == p;
}

// One workgroup column (blockIdx.x) per plane (c = blockIdx.y, n = blockIdx.z): a plane has one group, so the LDS table is B counters.
template <int NPX, bool GLOBAL>
__global__ __launch_bounds__(HT) void hist_f32_kernel(HistF32Args a) {
    const int c = blockIdx.y, n = blockIdx.z;
    const int g = a.grp[c];
    if (g < 0) return;                                           // uniform: the whole workgroup leaves
    if (!GLOBAL) lds_clear(a.nc * a.stride);
    uint32_t* tab = h_lds + (GLOBAL ? 0 : (int)(threadIdx.x % (unsigned)a.nc) * a.stride);
    uint64_t* out = a.counts + ((size_t)n * a.G + g) * a.B;
    const size_t po = ((size_t)n * a.C + c) * a.hw;
    const float* px = a.x + po;
    const float* p2 = a.x2 ? a.x2 + po : nullptr;
    const float sc = a.scale[n];
    const int R = a.R;
    const uint32_t nch = a.hw / NPX;
    for (uint32_t i = blockIdx.x * HT + threadIdx.x; i < nch; i += gridDim.x * HT) {
        float t[NPX], t2[NPX];
        if constexpr (NPX == 4) {
            const float4 q = reinterpret_cast<const float4*>(px)[i];
            t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
            if (p2) {
                const float4 r = reinterpret_cast<const float4*>(p2)[i];
                t2[0] = r.x; t2[1] = r.y; t2[2] = r.z; t2[3] = r.w;
            }
        } else {
            t[0] = px[i];
            if (p2) t2[0] = p2[i];
        }
#pragma unroll
        for (int j = 0; j < NPX; ++j) {
            int q, q2 = 0;
            bool ok = quant(t[j], sc, q);
            if (p2) ok = quant(t2[j], sc, q2) && ok;
            if (ok) hist_add<GLOBAL>(tab, out, min(max(q - q2 + R, 0), 2 * R));
        }
    }
    if (!GLOBAL) lds_flush(a.B, a.nc, a.stride, out);
}

// copies and stride of a table of tw words; nc == 0: no LDS stage
void lds_layout(size_t tw, int& nc, int& stride, size_t& bytes) {
    const size_t st = (tw + 30) / 32 * 32 + 1;                   // >= tw and 1 modulo 32: copy c's bin b lies in bank (b + c) % 32
    stride = (int)st;
    nc = (int)((size_t)H_LDS_SHARED / (st * 4));
    if (nc > H_MAX_COPIES) nc = H_MAX_COPIES;
    if (nc == 0 && st * 4 <= (size_t)H_LDS_SINGLE) nc = 1;
    bytes = (size_t)nc * st * 4;
}

unsigned grid_x(uint32_t nchunks, int per_thread, size_t lds_bytes, int others) {
    const unsigned want = (unsigned)((nchunks + (uint32_t)(HT * per_thread) - 1) / (uint32_t)(HT * per_thread));
    const int wg_per_cu = lds_bytes > (size_t)H_LDS_SHARED ? 1 : 2;
    unsigned cap = (unsigned)((2 * wg_per_cu * eld_num_cus() + others - 1) / others);   // two rounds of resident workgroups over the call
    if (cap < 1) cap = 1;
    return want < 1 ? 1 : (want < cap ? want : cap);
}

template <typename K, typename A>
int launch_hist(K kern, EldAttrOnce& once, dim3 grid, size_t lds_bytes, hipStream_t s, const A& a) {
    if (lds_bytes > 48 * 1024) {
        const int rc = once.ensure(kern, (size_t)H_LDS_SINGLE);
        if (rc) return rc;
    }
    ELD_LAUNCH(kern, grid, dim3(HT), lds_bytes, s, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

template <int P, int NPX>
int launch_u16(const HistU16Args& a, dim3 grid, size_t lds_bytes, hipStream_t s) {
    static EldAttrOnce once;
    if (a.nc == 0) return launch_hist(hist_u16_kernel<P, NPX, true>, once, grid, 0, s, a);
    return launch_hist(hist_u16_kernel<P, NPX, false>, once, grid, lds_bytes, s, a);
}

template <int NPX>
int launch_f32(const HistF32Args& a, dim3 grid, size_t lds_bytes, hipStream_t s) {
    static EldAttrOnce once;
    if (a.nc == 0) return launch_hist(hist_f32_kernel<NPX, true>, once, grid, 0, s, a);
    return launch_hist(hist_f32_kernel<NPX, false>, once, grid, lds_bytes, s, a);
}

}  // namespace

extern "C" int eld_hist_u16(const uint16_t* u, const uint16_t* v, int F, int Hm, int Wm, int p, const int* group, int G, const int32_t* centre,
                            int R, const uint32_t* bitmap, uint64_t* counts, void* stream) {
    if ((p != 2 && p != 6) || F < 0 || F > 65535 || Hm < 0 || Wm < 0 || Wm % 2 || G < 1 || G > 4 || R < 1 || R > 32767 || !group) return ELD_EINVAL;
    if ((uint64_t)Hm * (uint64_t)Wm >= (1ull << 31)) return ELD_EINVAL;
    for (int k = 0; k < p * p; ++k)
        if (group[k] < -1 || group[k] >= G) return ELD_EINVAL;
    if (!v) {
        if (!centre) return ELD_EINVAL;
        for (int k = 0; k < G; ++k)
            if (centre[k] < -(1 << 30) || centre[k] > (1 << 30)) return ELD_EINVAL;
    }
    if (F == 0) return 0;
    if (!counts || ((uintptr_t)counts & 7u)) return ELD_EINVAL;
    const bool empty = Hm == 0 || Wm == 0;
    if (!empty && (!u || ((uintptr_t)u & 3u) || ((uintptr_t)v & 3u) || ((uintptr_t)bitmap & 3u))) return ELD_EINVAL;
    HistU16Args a;
    a.u = u; a.v = v; a.bitmap = bitmap; a.counts = counts;
    a.Hm = Hm; a.Wm = Wm; a.G = G; a.R = R; a.B = 2 * R + 1; a.wpr = bitmap_pitch(Wm);
    for (int k = 0; k < 4; ++k) a.centre[k] = (!v && k < G) ? centre[k] : 0;
    for (int r = 0; r < 6; ++r) {
        a.roww[r] = 0;
        for (int k = 0; k < 12 && r < p; ++k) a.roww[r] |= (uint64_t)(group[r * p + k % p] + 1) << (4 * k);
    }
    hipStream_t s = as_stream(stream);
    const int rc = zero_u64(counts, (size_t)F * G * a.B, s);
    if (rc || empty) return rc;
    const bool vec = Wm % 8 == 0 && !((uintptr_t)u & 15u) && !((uintptr_t)v & 15u);
    const int npx = vec ? 8 : 2;
    a.cpr = (uint32_t)(Wm / npx);
    a.nchunks = a.cpr * (uint32_t)Hm;
    a.dcpr = make_fastdiv(a.cpr);
    size_t lds_bytes;
    lds_layout((size_t)G * a.B, a.nc, a.stride, lds_bytes);
    const dim3 grid(grid_x(a.nchunks, 2, lds_bytes, F), F);
    if (p == 2) return vec ? launch_u16<2, 8>(a, grid, lds_bytes, s) : launch_u16<2, 2>(a, grid, lds_bytes, s);
    return vec ? launch_u16<6, 8>(a, grid, lds_bytes, s) : launch_u16<6, 2>(a, grid, lds_bytes, s);
}

extern "C" int eld_hist_f32(const float* x, const float* x2, int N, int C, int H, int W, const int* group, int G, const float* scale, int R,
                            uint64_t* counts, void* stream) {
    if (N < 0 || N > 65535 || C < 1 || C > 64 || H < 0 || W < 0 || G < 1 || G > 4 || R < 1 || R > 32767 || !group) return ELD_EINVAL;
    if ((uint64_t)H * (uint64_t)W >= (1ull << 31)) return ELD_EINVAL;
    for (int k = 0; k < C; ++k)
        if (group[k] < -1 || group[k] >= G) return ELD_EINVAL;
    if (N == 0) return 0;
    if (!counts || ((uintptr_t)counts & 7u)) return ELD_EINVAL;
    const bool empty = H == 0 || W == 0;
    if (!empty && (!x || !scale || ((uintptr_t)x & 3u) || ((uintptr_t)x2 & 3u) || ((uintptr_t)scale & 3u))) return ELD_EINVAL;
    HistF32Args a;
    a.x = x; a.x2 = x2; a.scale = scale; a.counts = counts;
    a.C = C; a.G = G; a.R = R; a.B = 2 * R + 1; a.hw = (uint32_t)H * (uint32_t)W;
    for (int k = 0; k < 64; ++k) a.grp[k] = (signed char)(k < C ? group[k] : -1);
    hipStream_t s = as_stream(stream);
    const int rc = zero_u64(counts, (size_t)N * G * a.B, s);
    if (rc || empty) return rc;
    const bool vec = a.hw % 4 == 0 && !((uintptr_t)x & 15u) && !((uintptr_t)x2 & 15u);
    size_t lds_bytes;
    lds_layout((size_t)a.B, a.nc, a.stride, lds_bytes);
    const dim3 grid(grid_x(a.hw / (vec ? 4 : 1), 2, lds_bytes, N * C), C, N);
    return vec ? launch_f32<4>(a, grid, lds_bytes, s) : launch_f32<1>(a, grid, lds_bytes, s);
}
