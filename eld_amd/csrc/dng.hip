// dng.hip -- the two decoders behind eld_amd/dng.py: packed-bit rows (DNG compression 1) and lossless JPEG (compression 7,
// ITU-T T.81 process 14) of a DNG's strips or tiles, written straight into the visible mosaic in HBM.  The per-stream code is dng_dev.h, which a
// host compiler takes too; the kernels here are the loops over it.
//
// Lossless JPEG: one lane per stream (a tile or strip is one independent Huffman stream, and inside it the bit position is a serial
// dependency).  `lanes` streams share a wave.  With as many lanes as a wave has, a 24 MP frame in 256 x 256 tiles (384 streams) would run on six
// waves of a chip that has 1024 SIMDs; with one lane per wave every stream has a SIMD to itself and pays no divergence, so the launcher picks
// the smallest `lanes` that still puts at most one wave on every SIMD.
// Packed bits: one lane per four samples (bits / 2 bytes, byte-aligned for every supported width), a stream per blockIdx.x.
#include "common.h"
#include "dng_dev.h"

namespace {

constexpr int DU_T = 256;
constexpr int DU_CHUNKS = 1024;          // blockIdx.y at most: grid-stride chunks of one stream's quads

struct DngArgs {
    const uint8_t* blob;
    size_t blob_bytes;
    const EldDngStream* streams;
    int nstreams;
    const EldDngHuff* tables;
    int ntables;
    uint16_t* ws;
    size_t ws_elems;
    int32_t* status;
    DngOut o;
    int bits, big_endian, lanes;
};

__global__ __launch_bounds__(ELD_WAVE) void dng_ljpeg_kernel(DngArgs a) {
    if ((int)threadIdx.x >= a.lanes) return;
    const long long i = (long long)blockIdx.x * a.lanes + threadIdx.x;
    if (i >= a.nstreams) return;
    const EldDngStream s = a.streams[i];
    a.status[i] = dng_ljpeg_stream(a.blob, a.blob_bytes, s, a.tables, a.ntables, a.ws, a.ws_elems, a.o);
}

__global__ __launch_bounds__(DU_T) void dng_unpack_kernel(DngArgs a) {
    const EldDngStream s = a.streams[blockIdx.x];
    if (!dng_unpack_record_ok(s, a.blob_bytes, a.bits)) {
        if (blockIdx.y == 0 && threadIdx.x == 0) a.status[blockIdx.x] = s.tw >= 1 && s.th >= 1 && s.x0 >= 0 && s.y0 >= 0 &&
                                                                      (uint64_t)s.data_off + s.data_len <= (uint64_t)a.blob_bytes
                                                                      ? ELD_DNG_TRUNCATED : ELD_DNG_BADRECORD;
        return;
    }
    const uint32_t rowbytes = dng_row_bytes(s.tw, a.bits);
    const uint32_t gpr = ((uint32_t)s.tw + 3u) >> 2;                // quads per row; th * gpr <= 2^16 * 2^14
    const uint32_t units = (uint32_t)s.th * gpr;
    const uint8_t* base = a.blob + s.data_off;
    for (uint32_t u = blockIdx.y * DU_T + threadIdx.x; u < units; u += gridDim.y * DU_T) {
        const uint32_t r = u / gpr, g = u - r * gpr;
        dng_unpack_quad(base + (size_t)r * rowbytes, rowbytes, (int)g, a.bits, a.big_endian != 0, s, (int)r, a.o);
    }
}

// what both entry points refuse before any device work
bool bad_common(const void* blob, const void* streams, int nstreams, int H, int W, int top, int left, int Hm, int Wm, const uint16_t* lin, int lin_len,
                const uint16_t* out, const int32_t* status) {
    if (nstreams < 0 || H < 1 || W < 1 || Hm < 1 || Wm < 1 || top < 0 || left < 0) return true;
    if ((long long)top + Hm > H || (long long)left + Wm > W || (uint64_t)H * (uint64_t)W >= (1ull << 31)) return true;
    if (lin_len < 0 || lin_len > 65536 || (lin_len > 0 && !lin) || ((uintptr_t)lin & 1u)) return true;
    if (nstreams > 0 && (!blob || !streams || !out || !status)) return true;
    return ((uintptr_t)out & 1u) || ((uintptr_t)streams & 3u) || ((uintptr_t)status & 3u);
}

DngOut make_out(uint16_t* out, int H, int W, int top, int left, int Hm, int Wm, const uint16_t* lin, int lin_len) {
    DngOut o;
    o.out = out; o.H = H; o.W = W; o.top = top; o.left = left; o.Hm = Hm; o.Wm = Wm;
    o.lin = lin_len > 0 ? lin : nullptr; o.lin_len = lin_len;
    return o;
}

}  // namespace

extern "C" int eld_dng_unpack_u16(const uint8_t* blob, size_t blob_bytes, const EldDngStream* streams, int nstreams, int bits, int big_endian, int H,
                                  int W, int top, int left, int Hm, int Wm, const uint16_t* lin, int lin_len, uint16_t* out, int32_t* status,
                                  void* stream) {
    if (bits != 8 && bits != 10 && bits != 12 && bits != 14 && bits != 16) return ELD_EINVAL;
    if (bad_common(blob, streams, nstreams, H, W, top, left, Hm, Wm, lin, lin_len, out, status)) return ELD_EINVAL;
    if (nstreams == 0) return 0;
    hipStream_t st = as_stream(stream);
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)nstreams, st);
    if (e != hipSuccess) return (int)e;
    DngArgs a = {};
    a.blob = blob; a.blob_bytes = blob_bytes; a.streams = streams; a.nstreams = nstreams; a.status = status;
    a.o = make_out(out, H, W, top, left, Hm, Wm, lin, lin_len);
    a.bits = bits; a.big_endian = big_endian;
    // chunks per stream from the mean stream (the records are on the device): about four quads per lane, the grid-stride loop takes the rest
    const long long quads = ((long long)H * W / 4 + nstreams - 1) / nstreams;
    long long chunks = (quads + 4 * DU_T - 1) / (4 * DU_T);
    chunks = chunks < 1 ? 1 : chunks > DU_CHUNKS ? DU_CHUNKS : chunks;
    ELD_LAUNCH(dng_unpack_kernel, dim3((unsigned)nstreams, (unsigned)chunks), dim3(DU_T), 0, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

extern "C" int eld_dng_ljpeg_u16(const uint8_t* blob, size_t blob_bytes, const EldDngStream* streams, int nstreams, const EldDngHuff* tables,
                                 int ntables, int H, int W, int top, int left, int Hm, int Wm, const uint16_t* lin, int lin_len, uint16_t* ws,
                                 size_t ws_elems, int lanes, uint16_t* out, int32_t* status, void* stream) {
    if (ntables < 0 || lanes < 0 || lanes > ELD_WAVE || (ws_elems > 0 && !ws) || ((uintptr_t)ws & 1u) || ((uintptr_t)tables & 3u)) return ELD_EINVAL;
    if (bad_common(blob, streams, nstreams, H, W, top, left, Hm, Wm, lin, lin_len, out, status)) return ELD_EINVAL;
    if (nstreams > 0 && (!tables || ntables < 1)) return ELD_EINVAL;
    if (nstreams == 0) return 0;
    if (lanes == 0) {                                               // at most one wave per SIMD, as few lanes per wave as that allows
        const int simds = 4 * eld_num_cus();
        lanes = (nstreams + simds - 1) / simds;
        lanes = lanes < 1 ? 1 : lanes > ELD_WAVE ? ELD_WAVE : lanes;
    }
    DngArgs a = {};
    a.blob = blob; a.blob_bytes = blob_bytes; a.streams = streams; a.nstreams = nstreams; a.tables = tables; a.ntables = ntables;
    a.ws = ws; a.ws_elems = ws_elems; a.status = status; a.lanes = lanes;
    a.o = make_out(out, H, W, top, left, Hm, Wm, lin, lin_len);
    const unsigned grid = (unsigned)(((long long)nstreams + lanes - 1) / lanes);
    ELD_LAUNCH(dng_ljpeg_kernel, dim3(grid), dim3(ELD_WAVE), 0, as_stream(stream), a);
    ELD_LAUNCH_CHECK();
    return 0;
}
