// dng_enc.hip -- the lossless-JPEG encoder behind eld_amd.dng.write_dng(compression=7) and encode_ljpeg: the tiles of a mosaic
// in HBM become the entropy-coded data of one ITU-T T.81 process-14 stream each.  The per-lane arithmetic is dng_enc_dev.h, which a host compiler
// takes too; the kernels here are the loops, the scans and the stores around it.
//
// Encoding is parallel per sample: with predictor 1 a sample's code depends on two samples, its bit position is a prefix sum of code lengths and
// the byte stuffing a prefix sum of FF counts.  A stream is cut into segments of a fixed number of samples, and the host, which builds the
// Huffman table from the histogram, knows every segment's first bit from histogram . (code length + extra bits) before a bit is packed: no
// kernel scans across workgroups.
//   hist     a workgroup per (stream, segment): categories by wave ballots into scalar counters, summed over the waves in LDS
//   pack     a workgroup per (stream, segment): a lane per contiguous run; the run's bit count, an exclusive scan over the workgroup, the bits
//            into an LDS image of the segment by LDS ORs, the image out as byte-swapped dwords (the first and last one by global atomic OR)
//   ffcount  a workgroup per chunk of unstuffed bytes, 16 bytes per lane
//   stuff    the same cut: FF counts scanned over the workgroup, the stuffed bytes into an LDS image aligned like their destination, whole
//            dwords out
#include "common.h"
#include "dng_enc_dev.h"

namespace {

constexpr int DE_T = 256;
constexpr int DE_WAVES = DE_T / ELD_WAVE;

struct EncArgs {
    const uint16_t* mos;
    int H, W, th, tw, nx;
    uint32_t half, n, segment, nseg, run;    // samples per tile, per segment, segments per stream, samples per lane
    uint32_t* hist;
    uint32_t* maxcode;
    const uint32_t* tables;
    const uint32_t* seg_bit;
    const uint32_t* raw_dword;
    uint32_t* raw;
    size_t raw_dwords;
    uint32_t img_dwords;
};

struct StuffArgs {
    const uint8_t* raw;
    size_t raw_bytes;
    const EldDngEncChunk* chunks;
    uint32_t chunk;
    uint32_t* count;
    const uint32_t* ffbefore;
    uint8_t* out;
    size_t out_bytes;
    uint32_t img_bytes;
};

__device__ __forceinline__ DngEncSrc enc_src(const EncArgs& a, uint32_t s) {
    DngEncSrc src;
    const uint32_t ty = s / (uint32_t)a.nx, tx = s - ty * (uint32_t)a.nx;
    src.mos = a.mos; src.H = a.H; src.W = a.W; src.y0 = (int)ty * a.th; src.x0 = (int)tx * a.tw; src.tw = a.tw; src.half = a.half;
    return src;
}

// the lane's run of segment g: [first, first + count) of the tile's samples; count 0 behind the segment's end
__device__ __forceinline__ void enc_run_of(const EncArgs& a, uint32_t g, uint32_t* first, uint32_t* count, uint32_t* seg_count) {
    const uint32_t seg_first = g * a.segment;
    const uint32_t sc = a.n - seg_first < a.segment ? a.n - seg_first : a.segment;
    const uint32_t off = threadIdx.x * a.run;
    *first = seg_first + off;
    *count = off < sc ? (sc - off < a.run ? sc - off : a.run) : 0u;
    *seg_count = sc;
}

// exclusive scan of v over the workgroup's DE_T lanes; *total: the sum.  wsum: DE_WAVES dwords of LDS nobody else touches.
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
    for (uint32_t w = 0; w < (uint32_t)DE_WAVES; ++w) {
        const uint32_t x = wsum[w];
        base += w < wave ? x : 0u;
        all += x;
    }
    *total = all;
    return base + inc - v;
}

__global__ __launch_bounds__(DE_T) void dng_enc_hist_kernel(EncArgs a) {
    __shared__ uint32_t wh[DE_WAVES][17];
    __shared__ uint32_t wmax[DE_WAVES];
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    const DngEncSrc src = enc_src(a, s);
    uint32_t first, count, seg_count;
    enc_run_of(a, g, &first, &count, &seg_count);
    DngEncCursor k = dng_enc_cursor(src, first);
    uint32_t cnt[17];
#pragma unroll
    for (int b = 0; b < 17; ++b) cnt[b] = 0;
    uint32_t mx = 0;
    for (uint32_t j = 0; j < a.run; ++j) {                           // a.run is uniform: every lane reaches every ballot
        uint32_t ssss = 31u;
        if (j < count) {
            uint32_t code;
            ssss = dng_enc_ssss(dng_enc_next(src, k, &code));
            mx = code > mx ? code : mx;
        }
#pragma unroll
        for (int b = 0; b < 17; ++b) cnt[b] += (uint32_t)__popcll(__ballot(ssss == (uint32_t)b));
    }
#pragma unroll
    for (int o = ELD_WAVE / 2; o > 0; o >>= 1) {
        const uint32_t t = __shfl_xor(mx, o, ELD_WAVE);
        mx = t > mx ? t : mx;
    }
    const uint32_t lane = threadIdx.x & (ELD_WAVE - 1), wave = threadIdx.x / ELD_WAVE;
    if (lane == 0) {
#pragma unroll
        for (int b = 0; b < 17; ++b) wh[wave][b] = cnt[b];
        wmax[wave] = mx;
    }
    __syncthreads();
    if (threadIdx.x < 17) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < DE_WAVES; ++w) t += wh[w][threadIdx.x];
        a.hist[((size_t)s * a.nseg + g) * 17 + threadIdx.x] = t;
    }
    if (threadIdx.x == 0) {
        uint32_t m = 0;
#pragma unroll
        for (int w = 0; w < DE_WAVES; ++w) m = wmax[w] > m ? wmax[w] : m;
        atomicMax(&a.maxcode[s], m);
    }
}

// a lane's dwords into the segment's LDS image
struct LdsOr {
    uint32_t* img;
    uint32_t cap;
    __device__ __forceinline__ void operator()(uint32_t i, uint32_t v) const {
        if (i < cap) atomicOr(&img[i], v);
    }
};

__global__ __launch_bounds__(DE_T) void dng_enc_pack_kernel(EncArgs a) {
    extern __shared__ uint32_t img[];                                // a.img_dwords
    __shared__ uint32_t tab[17];
    __shared__ uint32_t wsum[DE_WAVES];
    const uint32_t g = blockIdx.x, s = blockIdx.y;
    if (threadIdx.x < 17) tab[threadIdx.x] = a.tables[(size_t)s * 17 + threadIdx.x];
    for (uint32_t i = threadIdx.x; i < a.img_dwords; i += DE_T) img[i] = 0u;
    __syncthreads();
    const DngEncSrc src = enc_src(a, s);
    uint32_t first, count, seg_count;
    enc_run_of(a, g, &first, &count, &seg_count);
    const uint32_t bits = dng_enc_run_bits(src, tab, first, count);
    uint32_t total;
    const uint32_t ex = block_exscan(bits, wsum, &total);
    const uint32_t b0 = a.seg_bit[(size_t)s * (a.nseg + 1) + g], b1 = a.seg_bit[(size_t)s * (a.nseg + 1) + g + 1];
    if (total != b1 - b0) return;                                    // the plan and the data disagree (uniform): nothing is written
    const bool last = g == a.nseg - 1;
    const uint32_t pad = last ? (0u - b1) & 7u : 0u, phase = b0 & 31u;
    if (count) {
        const bool tail = last && threadIdx.x == (seg_count - 1) / a.run;     // the lane that holds the stream's last sample
        LdsOr put = {img, a.img_dwords};
        dng_enc_run(src, tab, first, count, phase + ex, tail ? pad : 0u, put);
    }
    __syncthreads();
    const uint32_t ndw = (phase + total + pad + 31u) >> 5;
    const size_t dw0 = (size_t)a.raw_dword[s] + (b0 >> 5);
    for (uint32_t i = threadIdx.x; i < ndw && i < a.img_dwords; i += DE_T) {
        if (dw0 + i >= a.raw_dwords) break;
        const uint32_t v = __builtin_bswap32(img[i]);                // bit 0 of the image is the top bit of byte 0
        if (i == 0 || i == ndw - 1) atomicOr(&a.raw[dw0 + i], v);    // shared with the neighbouring segments
        else a.raw[dw0 + i] = v;
    }
}

// the lane's 16 bytes of its chunk: m of them valid
__device__ __forceinline__ uint32_t load_lane_bytes(const StuffArgs& a, const EldDngEncChunk& ch, uint8_t* b) {
    const uint32_t n = ch.nbytes < a.chunk ? ch.nbytes : a.chunk;
    const uint32_t off = threadIdx.x * DNG_ENC_LANE_BYTES;
    uint32_t m = off < n ? (n - off < DNG_ENC_LANE_BYTES ? n - off : DNG_ENC_LANE_BYTES) : 0u;
    const size_t pos = (size_t)ch.src + off;
    if (pos >= a.raw_bytes) m = 0;
    else if (a.raw_bytes - pos < m) m = (uint32_t)(a.raw_bytes - pos);
    if (m == DNG_ENC_LANE_BYTES && ((pos | (uintptr_t)a.raw) & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(a.raw + pos);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = (uint32_t)i < m ? a.raw[pos + i] : (uint8_t)0;
    }
    return m;
}

__global__ __launch_bounds__(DE_T) void dng_enc_ffcount_kernel(StuffArgs a) {
    __shared__ uint32_t wsum[DE_WAVES];
    const EldDngEncChunk ch = a.chunks[blockIdx.x];
    uint8_t b[16];
    const uint32_t m = load_lane_bytes(a, ch, b);
    uint32_t total;
    (void)block_exscan(dng_enc_count_ff(b, m), wsum, &total);
    if (threadIdx.x == 0) a.count[blockIdx.x] = total;
}

__global__ __launch_bounds__(DE_T) void dng_enc_stuff_kernel(StuffArgs a) {
    extern __shared__ uint32_t simg[];                               // a.img_bytes, a multiple of 4
    __shared__ uint32_t wsum[DE_WAVES];
    uint8_t* simg8 = reinterpret_cast<uint8_t*>(simg);
    const EldDngEncChunk ch = a.chunks[blockIdx.x];
    uint8_t b[16];
    const uint32_t m = load_lane_bytes(a, ch, b);
    uint32_t total;
    const uint32_t ex = block_exscan(dng_enc_count_ff(b, m), wsum, &total);
    uint32_t valid = ch.nbytes < a.chunk ? ch.nbytes : a.chunk;      // the bytes the lanes hold: the chunk's, unless raw ends inside it
    if ((size_t)ch.src >= a.raw_bytes) valid = 0;
    else if (a.raw_bytes - ch.src < valid) valid = (uint32_t)(a.raw_bytes - ch.src);
    const size_t dst = (size_t)ch.dst + a.ffbefore[blockIdx.x];
    const uint32_t sh = (uint32_t)(dst & 3u);                        // the image is aligned like its destination: whole dwords go out
    (void)dng_enc_stuff(b, m, simg8, sh + threadIdx.x * DNG_ENC_LANE_BYTES + ex, a.img_bytes);
    __syncthreads();
    const uint32_t end = sh + valid + total < a.img_bytes ? sh + valid + total : a.img_bytes;
    const size_t base = dst - sh;
    for (uint32_t i = threadIdx.x; 4u * i < end; i += DE_T) {
        const uint32_t lo = 4u * i, hi = lo + 4u;
        if (lo >= sh && hi <= end && base + hi <= a.out_bytes) {
            *reinterpret_cast<uint32_t*>(a.out + base + lo) = simg[i];
        } else {
            for (uint32_t j = lo; j < hi; ++j)
                if (j >= sh && j < end && base + j < a.out_bytes) a.out[base + j] = simg8[j];
        }
    }
}

// what the two mosaic passes refuse; fills the geometry
bool enc_args(EncArgs* a, const uint16_t* mosaic, int H, int W, int th, int tw, int bits, int segment) {
    if (!mosaic || ((uintptr_t)mosaic & 1u) || H < 1 || W < 1 || (uint64_t)H * (uint64_t)W >= (1ull << 31)) return false;
    if (th < 16 || tw < 16 || th % 16 || tw % 16 || (uint64_t)th * (uint64_t)tw > (1ull << 24)) return false;
    if (bits < 8 || bits > 16) return false;
    if (segment == 0) segment = ELD_DNG_ENC_SEGMENT;
    if (segment < 64 || segment > ELD_DNG_ENC_MAX_SEGMENT || segment % 64) return false;
    a->mos = mosaic; a->H = H; a->W = W; a->th = th; a->tw = tw; a->nx = (W + tw - 1) / tw;
    a->half = 1u << (bits - 1);
    a->n = (uint32_t)th * (uint32_t)tw;
    a->segment = (uint32_t)segment;
    a->nseg = (a->n + a->segment - 1) / a->segment;
    a->run = (a->segment + DE_T - 1) / DE_T;
    a->img_dwords = a->segment + 2;                                  // 31 phase bits, 31 bits a sample, 7 of padding
    const uint64_t ny = ((uint64_t)H + th - 1) / th;
    return ny <= 65535u && a->nseg <= 0x7FFFFFFFu;                   // gridDim.y, gridDim.x
}

bool stuff_args(StuffArgs* a, const uint8_t* raw, size_t raw_bytes, const EldDngEncChunk* chunks, int nchunks, int chunk) {
    if (nchunks < 0 || (nchunks > 0 && (!raw || !chunks)) || ((uintptr_t)chunks & 3u)) return false;
    if (chunk == 0) chunk = ELD_DNG_ENC_CHUNK;
    if (chunk < 16 || chunk > ELD_DNG_ENC_MAX_CHUNK || chunk % 16) return false;
    a->raw = raw; a->raw_bytes = raw_bytes; a->chunks = chunks; a->chunk = (uint32_t)chunk;
    a->img_bytes = 2u * (uint32_t)chunk + 4u;                        // every byte an FF, three bytes of alignment
    return true;
}

}  // namespace

extern "C" int eld_dng_enc_hist_u16(const uint16_t* mosaic, int H, int W, int th, int tw, int bits, int segment, uint32_t* hist, uint32_t* maxcode,
                                    void* stream) {
    EncArgs a = {};
    if (!enc_args(&a, mosaic, H, W, th, tw, bits, segment)) return ELD_EINVAL;
    if (!hist || !maxcode || ((uintptr_t)hist & 3u) || ((uintptr_t)maxcode & 3u)) return ELD_EINVAL;
    const unsigned ny = (unsigned)((H + th - 1) / th), nstreams = ny * (unsigned)a.nx;
    if (nstreams > 65535u) return ELD_EINVAL;
    a.hist = hist; a.maxcode = maxcode;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(maxcode, 0, sizeof(uint32_t) * (size_t)nstreams, st);
    if (e != hipSuccess) return (int)e;
    ELD_LAUNCH(dng_enc_hist_kernel, dim3(a.nseg, nstreams), dim3(DE_T), 0, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_dng_enc_pack_u16(const uint16_t* mosaic, int H, int W, int th, int tw, int bits, int segment, const uint32_t* tables,
                                    const uint32_t* seg_bit, const uint32_t* raw_dword, uint32_t* raw, size_t raw_dwords, void* stream) {
    EncArgs a = {};
    if (!enc_args(&a, mosaic, H, W, th, tw, bits, segment)) return ELD_EINVAL;
    if (!tables || !seg_bit || !raw_dword || !raw || raw_dwords < 1) return ELD_EINVAL;
    if (((uintptr_t)tables | (uintptr_t)seg_bit | (uintptr_t)raw_dword | (uintptr_t)raw) & 3u) return ELD_EINVAL;
    const unsigned ny = (unsigned)((H + th - 1) / th), nstreams = ny * (unsigned)a.nx;
    if (nstreams > 65535u) return ELD_EINVAL;
    a.tables = tables; a.seg_bit = seg_bit; a.raw_dword = raw_dword; a.raw = raw; a.raw_dwords = raw_dwords;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(raw, 0, sizeof(uint32_t) * raw_dwords, st);
    if (e != hipSuccess) return (int)e;
    ELD_LAUNCH(dng_enc_pack_kernel, dim3(a.nseg, nstreams), dim3(DE_T), sizeof(uint32_t) * (size_t)a.img_dwords, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_dng_enc_ffcount_u8(const uint8_t* raw, size_t raw_bytes, const EldDngEncChunk* chunks, int nchunks, int chunk, uint32_t* count,
                                      void* stream) {
    StuffArgs a = {};
    if (!stuff_args(&a, raw, raw_bytes, chunks, nchunks, chunk)) return ELD_EINVAL;
    if (nchunks == 0) return 0;
    if (!count || ((uintptr_t)count & 3u)) return ELD_EINVAL;
    a.count = count;
    ELD_LAUNCH(dng_enc_ffcount_kernel, dim3((unsigned)nchunks), dim3(DE_T), 0, as_stream(stream), a);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_dng_enc_stuff_u8(const uint8_t* raw, size_t raw_bytes, const EldDngEncChunk* chunks, int nchunks, int chunk, const uint32_t* ffbefore,
                                    uint8_t* out, size_t out_bytes, void* stream) {
    StuffArgs a = {};
    if (!stuff_args(&a, raw, raw_bytes, chunks, nchunks, chunk)) return ELD_EINVAL;
    if (nchunks == 0) return 0;
    if (!ffbefore || !out || ((uintptr_t)ffbefore & 3u) || ((uintptr_t)out & 3u)) return ELD_EINVAL;
    a.ffbefore = ffbefore; a.out = out; a.out_bytes = out_bytes;
    ELD_LAUNCH(dng_enc_stuff_kernel, dim3((unsigned)nchunks), dim3(DE_T), a.img_bytes, as_stream(stream), a);
    ELD_LAUNCH_CHECK();
    return 0;
}
