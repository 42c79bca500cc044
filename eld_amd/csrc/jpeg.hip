// jpeg.hip -- the baseline-JPEG encoder behind eld_amd.jpeg.encode_jpeg: a planar uint8 sRGB render in HBM becomes the
// entropy-coded data of one ITU-T T.81 process-1 scan.  The per-block arithmetic is jpeg_dev.h, which a host compiler takes too; the kernels
// here are the loops, the scans and the stores around it.
//   coef     a lane per block of the scan: colour conversion, downsampling, forward DCT and quantisation in registers, 128 bytes out per lane
//   hist     a workgroup per segment of blocks: the four symbol histograms by LDS atomics (integer adds: the order does not matter)
//   pack     a workgroup per segment: a lane per contiguous run of blocks; the run's bit count, an exclusive scan over the workgroup, the bits
//            into an LDS image of the segment, the image out as byte-swapped dwords (the first and last one by global atomic OR); a segment
//            whose bits do not fit the image ORs every dword into the buffer directly
// The FF stuffing is dng_enc.hip's: its two byte-level kernels know nothing of what the bytes are.
#include "common.h"
#include "jpeg_dev.h"

namespace {

constexpr int JP_T = 256;
constexpr int JP_WAVES = JP_T / ELD_WAVE;
constexpr int JP_DEFAULT_LDS = 32 << 10;

struct QTables {
    uint16_t q[128];
};

struct CoefArgs {
    JpegSrc src;
    JpegGeom g;
    QTables q;
    int16_t* coef;
};

struct ScanArgs {
    const int16_t* coef;
    JpegGeom g;
    uint32_t segment, nseg, run;                                     // blocks per segment, segments, blocks per lane
    uint32_t* hist;
    const uint32_t* tables;
    const uint64_t* seg_bit;
    uint32_t* raw;
    size_t raw_dwords;
    uint32_t img_dwords;
};

__global__ __launch_bounds__(JP_T) void jpeg_coef_kernel(CoefArgs a) {
    const uint32_t b = blockIdx.x * JP_T + threadIdx.x;
    if (b >= a.g.nblocks) return;
    int16_t out[64];
    jpeg_block_coef(a.src, a.g, a.q.q, b, out);
    uint4* dst = reinterpret_cast<uint4*>(a.coef + (size_t)b * 64);  // 16-byte aligned: the entry point checked the base
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint4 v;
        v.x = (uint32_t)(uint16_t)out[8 * i + 0] | ((uint32_t)(uint16_t)out[8 * i + 1] << 16);
        v.y = (uint32_t)(uint16_t)out[8 * i + 2] | ((uint32_t)(uint16_t)out[8 * i + 3] << 16);
        v.z = (uint32_t)(uint16_t)out[8 * i + 4] | ((uint32_t)(uint16_t)out[8 * i + 5] << 16);
        v.w = (uint32_t)(uint16_t)out[8 * i + 6] | ((uint32_t)(uint16_t)out[8 * i + 7] << 16);
        dst[i] = v;
    }
}

// the coefficient buffer through 16-byte loads: a block is eight of them (the base is 16-byte aligned: the entry points check)
struct CoefRegs {
    const int16_t* p;
    __device__ __forceinline__ JpegBlockRegs block(uint32_t b) const {
        const uint4* src = reinterpret_cast<const uint4*>(p + (size_t)b * 64);
        JpegBlockRegs r;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 v = src[i];
            r.w[4 * i] = v.x; r.w[4 * i + 1] = v.y; r.w[4 * i + 2] = v.z; r.w[4 * i + 3] = v.w;
        }
        return r;
    }
    __device__ __forceinline__ int dc(uint32_t b) const { return p[(size_t)b * 64]; }
};

// the blocks of segment g: [first, first + count)
__device__ __forceinline__ void segment_of(const ScanArgs& a, uint32_t g, uint32_t* first, uint32_t* count) {
    *first = g * a.segment;
    *count = a.g.nblocks - *first < a.segment ? a.g.nblocks - *first : a.segment;
}

struct LdsAdd {
    uint32_t* h;
    __device__ __forceinline__ void operator()(uint32_t bin) const {
        if (bin < (uint32_t)ELD_JPEG_HIST) atomicAdd(&h[bin], 1u);
    }
};

__global__ __launch_bounds__(JP_T) void jpeg_hist_kernel(ScanArgs a) {
    __shared__ uint32_t h[ELD_JPEG_HIST];
    for (uint32_t i = threadIdx.x; i < (uint32_t)ELD_JPEG_HIST; i += JP_T) h[i] = 0u;
    __syncthreads();
    uint32_t first, count;
    segment_of(a, blockIdx.x, &first, &count);
    LdsAdd add = {h};
    const CoefRegs coef = {a.coef};
    for (uint32_t j = threadIdx.x; j < count; j += JP_T) jpeg_block_hist(coef, a.g, first + j, add);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)ELD_JPEG_HIST; i += JP_T) a.hist[(size_t)blockIdx.x * ELD_JPEG_HIST + i] = h[i];
}

// exclusive scan of v over the workgroup's JP_T lanes; *total: the sum.  wsum: JP_WAVES dwords of LDS nobody else touches.
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t* wsum, uint32_t* total) {
    const uint32_t lane = threadIdx.x & (ELD_WAVE - 1), wave = threadIdx.x / ELD_WAVE;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < ELD_WAVE; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, ELD_WAVE);
        if ((int)lane >= o) inc += t;
    }
    if (lane == ELD_WAVE - 1) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)JP_WAVES; ++w) {
        const uint32_t x = wsum[w];
        base += w < wave ? x : 0u;
        all += x;
    }
    *total = all;
    return base + inc - v;
}

// a lane's dwords into the segment's LDS image
struct LdsOr {
    uint32_t* img;
    uint32_t cap;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t v) const {
        if (i < cap) atomicOr(&img[i], v);
    }
};

// a lane's dwords straight into the buffer: the image index counts from the segment's first dword
struct GlobalOr {
    uint32_t* raw;
    size_t dw0, raw_dwords;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t v) const {
        if (dw0 + i < raw_dwords) atomicOr(&raw[dw0 + i], __builtin_bswap32(v));
    }
};

__global__ __launch_bounds__(JP_T) void jpeg_pack_kernel(ScanArgs a) {
    extern __shared__ uint32_t img[];                                // a.img_dwords
    __shared__ uint32_t tab[ELD_JPEG_TABLE];
    __shared__ uint32_t wsum[JP_WAVES];
    const uint32_t g = blockIdx.x;
    for (uint32_t i = threadIdx.x; i < (uint32_t)ELD_JPEG_TABLE; i += JP_T) tab[i] = a.tables[i];
    __syncthreads();
    uint32_t seg_first, seg_count;
    segment_of(a, g, &seg_first, &seg_count);
    const uint32_t off = threadIdx.x * a.run;
    const uint32_t first = seg_first + off, count = off < seg_count ? (seg_count - off < a.run ? seg_count - off : a.run) : 0u;
    const CoefRegs coef = {a.coef};
    const uint32_t bits = jpeg_run_bits(coef, a.g, tab, first, count);
    uint32_t total;
    const uint32_t ex = block_exscan(bits, wsum, &total);
    const uint64_t b0 = a.seg_bit[g], b1 = a.seg_bit[g + 1];
    if ((uint64_t)total != b1 - b0) return;                          // the plan and the data disagree (uniform): nothing is written
    const bool last = g == a.nseg - 1;
    const uint32_t pad = last ? (uint32_t)((0u - b1) & 7u) : 0u, phase = (uint32_t)(b0 & 31u);
    const uint32_t ndw = (phase + total + pad + 31u) >> 5;           // total < 2^22: no wrap
    const size_t dw0 = (size_t)(b0 >> 5);
    const bool tail = last && count && first + count == a.g.nblocks; // the lane that holds the scan's last block
    if (ndw > a.img_dwords) {                                        // uniform: the segment does not fit the image
        if (count) {
            GlobalOr put = {a.raw, dw0, a.raw_dwords};
            jpeg_run_pack(coef, a.g, tab, first, count, phase + ex, tail ? pad : 0u, put);
        }
        return;
    }
    for (uint32_t i = threadIdx.x; i < ndw; i += JP_T) img[i] = 0u;
    __syncthreads();
    if (count) {
        LdsOr put = {img, ndw};
        jpeg_run_pack(coef, a.g, tab, first, count, phase + ex, tail ? pad : 0u, put);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < ndw; i += JP_T) {
        if (dw0 + i >= a.raw_dwords) break;
        const uint32_t v = __builtin_bswap32(img[i]);                // bit 0 of the image is the top bit of byte 0
        if (i == 0 || i == ndw - 1) atomicOr(&a.raw[dw0 + i], v);    // shared with the neighbouring segments
        else a.raw[dw0 + i] = v;
    }
}

// what the two scan passes refuse; fills the geometry
bool scan_args(ScanArgs* a, const int16_t* coef, size_t coef_elems, int H, int W, int sub, int segment) {
    if (!coef || ((uintptr_t)coef & 15u) || !jpeg_geom(&a->g, H, W, sub)) return false;
    if (coef_elems != (size_t)a->g.nblocks * 64) return false;
    if (segment == 0) segment = ELD_JPEG_SEGMENT;
    if (segment < ELD_JPEG_MIN_SEGMENT || segment > ELD_JPEG_MAX_SEGMENT || segment % ELD_JPEG_MIN_SEGMENT) return false;
    a->coef = coef;
    a->segment = (uint32_t)segment;
    a->nseg = (a->g.nblocks + a->segment - 1) / a->segment;
    a->run = (a->segment + JP_T - 1) / JP_T;
    return true;
}

}  // namespace

extern "C" int eld_jpeg_coef_u8(const uint8_t* rgb, int H, int W, int subsampling, const uint16_t* qtables, int16_t* coef, size_t coef_elems,
                                void* stream) {
    CoefArgs a = {};
    if (!rgb || !qtables || !coef || ((uintptr_t)coef & 15u) || ((uintptr_t)qtables & 1u)) return ELD_EINVAL;
    if (!jpeg_geom(&a.g, H, W, subsampling) || coef_elems != (size_t)a.g.nblocks * 64) return ELD_EINVAL;
    for (int i = 0; i < 128; ++i) {
        if (qtables[i] < 1 || qtables[i] > 255) return ELD_EINVAL;
        a.q.q[i] = qtables[i];
    }
    a.src.rgb = rgb; a.src.H = H; a.src.W = W;
    a.coef = coef;
    ELD_LAUNCH(jpeg_coef_kernel, dim3((a.g.nblocks + JP_T - 1) / JP_T), dim3(JP_T), 0, as_stream(stream), a);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_jpeg_hist_i16(const int16_t* coef, size_t coef_elems, int H, int W, int subsampling, int segment, uint32_t* hist,
                                 size_t hist_elems, void* stream) {
    ScanArgs a = {};
    if (!scan_args(&a, coef, coef_elems, H, W, subsampling, segment)) return ELD_EINVAL;
    if (!hist || ((uintptr_t)hist & 3u) || hist_elems != (size_t)a.nseg * ELD_JPEG_HIST) return ELD_EINVAL;
    a.hist = hist;
    ELD_LAUNCH(jpeg_hist_kernel, dim3(a.nseg), dim3(JP_T), 0, as_stream(stream), a);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_jpeg_pack_i16(const int16_t* coef, size_t coef_elems, int H, int W, int subsampling, int segment, const uint32_t* tables,
                                 const uint64_t* seg_bit, uint32_t* raw, size_t raw_dwords, int lds_bytes, void* stream) {
    ScanArgs a = {};
    if (!scan_args(&a, coef, coef_elems, H, W, subsampling, segment)) return ELD_EINVAL;
    if (!tables || !seg_bit || !raw || raw_dwords < 1 || lds_bytes > 61440) return ELD_EINVAL;
    if ((((uintptr_t)tables | (uintptr_t)raw) & 3u) || ((uintptr_t)seg_bit & 7u)) return ELD_EINVAL;
    if (lds_bytes < 0) lds_bytes = JP_DEFAULT_LDS;
    a.tables = tables; a.seg_bit = seg_bit; a.raw = raw; a.raw_dwords = raw_dwords;
    a.img_dwords = (uint32_t)lds_bytes / 4u;
    const uint32_t worst = a.segment * 53u + 2u;                     // 27 + 63 * 26 bits a block, 31 phase bits, 7 of padding
    if (a.img_dwords > worst) a.img_dwords = worst;
    a.img_dwords = (a.img_dwords + 3u) & ~3u;                        // the dynamic LDS stays a multiple of 16 bytes
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(raw, 0, sizeof(uint32_t) * raw_dwords, st);
    if (e != hipSuccess) return (int)e;
    ELD_LAUNCH(jpeg_pack_kernel, dim3(a.nseg), dim3(JP_T), sizeof(uint32_t) * (size_t)a.img_dwords, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}
