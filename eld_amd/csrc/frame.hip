// frame.hip -- the frame of the full-resolution render: a crop rectangle of demosaiced camera RGB is resampled to an output
// size by a separable antialiasing filter given as per-axis tap tables, the three resampled values of a pixel go through the renders' tail
// (render_tail.h: CCM, gamma table / pow / CRF, quantiser), and the result is stored where one of the eight TIFF orientations puts it.  The
// per-output arithmetic is frame_dev.h, which a host compiler takes too; the two kernels here are the tiling around it.
//
// Row pass (frame_row_kernel): h[r][j] = the horizontal tap sum of source row row0 + r at unoriented column j, for the `rows` source rows any
// vertical table uses, into the caller's float32 workspace (N, 3, rows, Wc).  256 lanes along j, FR_ROWS rows per lane.  Neighbouring lanes
// read `scale` elements apart, so read directly every load of a wave touches up to 64 different lines, and the pass is then bound by line
// accesses, not bytes (sec. 34: 4.8 ms for a 24 MP picture to 171 x 256 with lanczos).  So the workgroup stages the span of the source its
// 256 outputs read, [min start, max start + count), in LDS with coalesced loads, in ascending chunks of FR_CHUNK elements: the span is
// bounded by nothing but T and the stride, the chunk is not.  For every chunk a lane adds the taps of its own range that fall inside it
// (frame_sums_part), so every sum still runs in ascending tap order and the bits do not depend on the chunking.  The x weights are stored
// tap-major (xw[k * Wc + j]): a wave reads 64 consecutive floats per tap.  Tables narrower than FR_STAGE_TAPS are read directly, through L1:
// with few taps and a small stride the lines a wave touches are few, and the full-size case (one tap, unit stride) runs at the rate of
// a copy directly and 4.5 times slower staged.  A workgroup whose table entries are not all plain -- a start
// below 0 or a run past the row's end, which eld_amd.isp never builds -- takes the direct path through the clamps of frame_dev.h instead
// (a uniform choice per workgroup): staging never sees a value that needs a clamp, and a corrupt table cannot lengthen the chunk loop.
//
// Column pass (frame_col_kernel): a workgroup of 256 lanes owns a tile of FT x FT unoriented outputs.  A wave owns FT / 4 rows i, a lane one
// column j: the vertical table's entries are wave-uniform (scalar loads), the workspace reads are rows of 64 consecutive floats.  The tail
// runs on the three sums.  Orientations 1 .. 4 keep rows as rows (mirrored or not), so a wave's 64 values go to 64 consecutive elements of an
// output row directly.  Orientations 5 .. 8 transpose: the tile goes through LDS (as output elements: bytes or floats, rows padded against
// bank conflicts) and is read back with the lanes along i, so that again every wave stores 64 consecutive elements of one output row.
#include <type_traits>

#include "common.h"
#include "frame_dev.h"

namespace {
#include "render_tail.h"

constexpr int FR_T = 256;                        // lanes of a row-pass workgroup, along j
constexpr int FR_ROWS = 4;                       // source rows per lane
constexpr int FR_CHUNK = 2048;                   // source elements per row staged at a time: 32 KB of LDS
constexpr int FR_STAGE_TAPS = 16;                // tables at least this wide are staged: measured, 7 taps are faster direct (122 against 148 us), 25 staged (sec. 34)
static_assert(FR_ROWS == 4, "frame_row_kernel names its four staged rows");
constexpr int FC_T = 256;                        // lanes of a column-pass workgroup
constexpr int FT = 64;                           // the column pass's tile: FT x FT unoriented outputs
constexpr int FC_WAVES = FC_T / ELD_WAVE;        // 4
constexpr int FC_ROWS = FT / FC_WAVES;           // rows of a wave
static_assert(FT == ELD_WAVE, "a wave spans the tile's columns, and after the transpose its rows");

struct FrameRowArgs {
    const float* rgb;
    float* ws;
    const int* xstart;
    const int* xcount;
    const float* xw;
    int Tx, Hs, Ws, Wc, row0, rows;
};

struct FrameColArgs {
    const float* ws;
    void* out;
    TailArgs t;
    const int* ystart;
    const int* ycount;
    const float* yw;
    int Ty, Hc, Wc, row0, rows, o;
};

__global__ __launch_bounds__(FR_T) void frame_row_kernel(FrameRowArgs a) {
    __shared__ float s_src[FR_ROWS][FR_CHUNK];
    __shared__ int s_lo, s_hi;
    const int tid = threadIdx.x, j = blockIdx.x * FR_T + tid;
    const bool live = j < a.Wc;
    const int r0 = blockIdx.y * FR_ROWS;                             // < rows: the grid is ceil(rows / FR_ROWS)
    const size_t z = blockIdx.z;                                     // frame * 3 + plane
    const float* src = a.rgb + z * (size_t)a.Hs * (size_t)a.Ws;
    const float* row[FR_ROWS];
#pragma unroll
    for (int q = 0; q < FR_ROWS; ++q)                                // rows past the last one repeat it and are not stored
        row[q] = src + (size_t)frame_source_row(a.row0, min(r0 + q, a.rows - 1), a.Hs) * (size_t)a.Ws;
    const int start = live ? a.xstart[j] : 0, n = live ? frame_count(a.xcount[j], a.Tx) : 0;
    const float* w = a.xw + (size_t)(live ? j : 0);
    if (tid == 0) { s_lo = a.Ws; s_hi = 0; }
    const bool plain = a.Tx >= FR_STAGE_TAPS && (!live || (start >= 0 && (int64_t)start + n <= (int64_t)a.Ws));
    const bool staged = __syncthreads_and(plain) != 0;               // also publishes s_lo, s_hi
    float v[FR_ROWS];
    if (!staged) {
        if (live) frame_sums_part<FR_ROWS>(row, 1, a.Ws, start, 0, n, w, (size_t)a.Wc, v);
    } else {
        if (live) {                                                  // 0 <= start, start + n <= Ws
            atomicMin(&s_lo, start);
            atomicMax(&s_hi, start + n);
        }
        __syncthreads();
        const int lo = s_lo, hi = s_hi;                              // lo < hi <= Ws: the workgroup's first lane is live
        for (int c0 = lo; c0 < hi; c0 += FR_CHUNK) {
            const int len = min(FR_CHUNK, hi - c0);
            if (c0 != lo) __syncthreads();                           // the last chunk has been read
            for (int e = tid; e < len; e += FR_T)
#pragma unroll
                for (int q = 0; q < FR_ROWS; ++q) s_src[q][e] = row[q][c0 + e];
            __syncthreads();
            const int k0 = max(0, c0 - start), k1 = min(n, c0 + len - start);      // the lane's taps inside [c0, c0 + len)
            const float* const piece[FR_ROWS] = {s_src[0], s_src[1], s_src[2], s_src[3]};
            if (k0 < k1) frame_sums_part<FR_ROWS>(piece, 1, len, (int64_t)start - c0, k0, k1, w, (size_t)a.Wc, v);
        }
    }
    if (!live) return;
    float* dst = a.ws + z * (size_t)a.rows * (size_t)a.Wc + (size_t)j;
#pragma unroll
    for (int q = 0; q < FR_ROWS; ++q)
        if (r0 + q < a.rows) dst[(size_t)(r0 + q) * (size_t)a.Wc] = v[q];
}

template <int TAIL>
__device__ __forceinline__ void frame_store(void* out, size_t e, float v) {
    if (TAIL == TAIL_LINEAR) ((float*)out)[e] = v;
    else ((unsigned char*)out)[e] = (unsigned char)v;
}

// TR: the orientation transposes (5 .. 8)
template <int TAIL, bool TR>
__global__ __launch_bounds__(FC_T) void frame_col_kernel(FrameColArgs a) {
    using Elem = typename std::conditional<TAIL == TAIL_LINEAR, float, unsigned char>::type;
    constexpr int PITCH = TAIL == TAIL_LINEAR ? FT + 1 : FT + 4;     // floats: 65 words; bytes: 17 words: a column of the tile spreads over the banks
    __shared__ Elem s_tile[TR ? 3 * FT * PITCH : 1];                 // [plane][j][i]
    __shared__ unsigned s_t[256];
    const int tid = threadIdx.x, lane = tid & (ELD_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / ELD_WAVE);
    stage_gamma_table<TAIL, FC_T>(s_t);
    __syncthreads();
    const int n = blockIdx.z, Hc = a.Hc, Wc = a.Wc;
    const int i0 = blockIdx.y * FT, j0 = blockIdx.x * FT;
    const int Ho = TR ? Wc : Hc, Wo = TR ? Hc : Wc;                  // the upright picture
    const size_t oplane = (size_t)Ho * (size_t)Wo, wplane = (size_t)a.rows * (size_t)Wc;
    const float* ws = a.ws + (size_t)n * 3 * wplane;
    const size_t obase = (size_t)n * 3 * oplane;
    float m[9];
    load_ccm(a.t.ccms, n, m);
    const double ig = (double)a.t.inv_gamma;
    const int j = j0 + lane;
#pragma unroll 1
    for (int q = 0; q < FC_ROWS; ++q) {
        const int il = wave * FC_ROWS + q, i = i0 + il;              // wave-uniform
        if (i >= Hc) break;
        if (j >= Wc) continue;
        const float* const col[3] = {ws + (size_t)j, ws + wplane + (size_t)j, ws + 2 * wplane + (size_t)j};
        float v[3];
        frame_sums<3>(col, (size_t)Wc, a.rows, (int64_t)a.ystart[i] - (int64_t)a.row0, a.ycount[i], a.yw + (size_t)i * (size_t)a.Ty, 1, a.Ty, v);
        float o[3];
        site_out<TAIL>(v[0], v[1], v[2], m, a.t, ig, s_t, o);
        if (TR) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s_tile[(c * FT + lane) * PITCH + il] = (Elem)o[c];
        } else {
            int Y, X;
            frame_upright(a.o, i, j, Hc, Wc, &Y, &X);
            const size_t e = obase + (size_t)Y * (size_t)Wo + (size_t)X;
#pragma unroll
            for (int c = 0; c < 3; ++c) frame_store<TAIL>(a.out, e + c * oplane, o[c]);
        }
    }
    if (!TR) return;
    __syncthreads();
    // the lanes along i now: a wave stores FT consecutive (o = 5, 8) or mirrored consecutive (o = 6, 7) elements of the output row its j gives
    const int i = i0 + lane;
#pragma unroll 1
    for (int q = 0; q < FC_ROWS; ++q) {
        const int jl = wave * FC_ROWS + q, jj = j0 + jl;
        if (jj >= Wc) break;
        if (i >= Hc) continue;
        int Y, X;
        frame_upright(a.o, i, jj, Hc, Wc, &Y, &X);
        const size_t e = obase + (size_t)Y * (size_t)Wo + (size_t)X;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const Elem s = s_tile[(c * FT + jl) * PITCH + lane];
            if (TAIL == TAIL_LINEAR) ((float*)a.out)[e + c * oplane] = (float)s;
            else ((unsigned char*)a.out)[e + c * oplane] = (unsigned char)s;
        }
    }
}

template <int TAIL, bool TR>
int frame_col_launch(const FrameColArgs& a, dim3 grid, hipStream_t st) {
    ELD_LAUNCH((frame_col_kernel<TAIL, TR>), grid, dim3(FC_T), 0, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

bool overlap(const void* p, size_t np, const void* q, size_t nq) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + nq && b < a + np;
}

}  // namespace

extern "C" int eld_frame_rgb_tile(int* tile_h, int* tile_w, int* lds_bytes) {
    if (!tile_h || !tile_w) return ELD_EINVAL;
    *tile_h = FT;
    *tile_w = FT;
    if (lds_bytes) *lds_bytes = 3 * FT * (FT + 1) * (int)sizeof(float) + 256 * (int)sizeof(unsigned);      // the widest instantiation: float32, transposed
    return 0;
}

extern "C" int eld_frame_rgb_f32(const float* rgb, void* out, int out_mode, int N, int Hs, int Ws, int Ho, int Wo, int orientation,
                                 const int* ystart, const int* ycount, const float* yw, int Ty, const int* xstart, const int* xcount,
                                 const float* xw, int Tx, int row0, int rows, float* workspace, size_t workspace_bytes, const float* ccms,
                                 float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream) {
    if (!rgb || !out || !ystart || !ycount || !yw || !xstart || !xcount || !xw || !workspace) return ELD_EINVAL;
    if (tail_args_bad(ccms, out_mode, gamma, crf_E, crf_f, crf_n)) return ELD_EINVAL;
    if (((uintptr_t)rgb & 3u) || ((uintptr_t)workspace & 3u) || (out_mode == ELD_RENDER_LINEAR_F32 && ((uintptr_t)out & 3u))) return ELD_EINVAL;
    if (((uintptr_t)ystart | (uintptr_t)ycount | (uintptr_t)yw | (uintptr_t)xstart | (uintptr_t)xcount | (uintptr_t)xw) & 3u) return ELD_EINVAL;
    if (N < 0 || N > 65535 / 3 || Hs < 1 || Ws < 1 || (uint64_t)Hs * (uint64_t)Ws >= (1ull << 31)) return ELD_EINVAL;
    if (Ho < 1 || Wo < 1 || (uint64_t)Ho * (uint64_t)Wo >= (1ull << 31)) return ELD_EINVAL;
    if (orientation < 1 || orientation > 8) return ELD_EINVAL;
    if (Ty < 1 || Ty > FRAME_MAX_TAPS || Tx < 1 || Tx > FRAME_MAX_TAPS) return ELD_EINVAL;
    if (row0 < 0 || rows < 1 || (int64_t)row0 + (int64_t)rows > (int64_t)Hs) return ELD_EINVAL;
    const bool tr = frame_transposed(orientation);
    const int Hc = tr ? Wo : Ho, Wc = tr ? Ho : Wo;
    if ((uint64_t)rows * (uint64_t)Wc >= (1ull << 31)) return ELD_EINVAL;
    const dim3 rgrid((unsigned)((Wc + FR_T - 1) / FR_T), (unsigned)((rows + FR_ROWS - 1) / FR_ROWS), (unsigned)(3 * N));
    const dim3 cgrid((unsigned)((Wc + FT - 1) / FT), (unsigned)((Hc + FT - 1) / FT), (unsigned)N);
    if (rgrid.y > 65535u || cgrid.y > 65535u) return ELD_EINVAL;
    const size_t in_bytes = (size_t)N * 3 * (size_t)Hs * (size_t)Ws * sizeof(float);
    const size_t out_bytes = (size_t)N * 3 * (size_t)Ho * (size_t)Wo * (out_mode == ELD_RENDER_LINEAR_F32 ? sizeof(float) : 1u);
    const size_t ws_bytes = (size_t)N * 3 * (size_t)rows * (size_t)Wc * sizeof(float);
    if (workspace_bytes < ws_bytes) return ELD_EWS;
    if (overlap(rgb, in_bytes, out, out_bytes) || overlap(rgb, in_bytes, workspace, ws_bytes) || overlap(out, out_bytes, workspace, ws_bytes))
        return ELD_EINVAL;
    if (N == 0) return 0;
    hipStream_t st = as_stream(stream);
    FrameRowArgs r = {};
    r.rgb = rgb; r.ws = workspace; r.xstart = xstart; r.xcount = xcount; r.xw = xw;
    r.Tx = Tx; r.Hs = Hs; r.Ws = Ws; r.Wc = Wc; r.row0 = row0; r.rows = rows;
    ELD_LAUNCH(frame_row_kernel, rgrid, dim3(FR_T), 0, st, r);
    ELD_LAUNCH_CHECK();
    FrameColArgs c = {};
    c.ws = workspace; c.out = out; c.ystart = ystart; c.ycount = ycount; c.yw = yw;
    c.Ty = Ty; c.Hc = Hc; c.Wc = Wc; c.row0 = row0; c.rows = rows; c.o = orientation;
    c.t = tail_args(ccms, gamma, crf_E, crf_f, crf_n);
    return with_tail(render_tail(out_mode, gamma, crf_n), [&](auto T) {
        constexpr int TAIL = decltype(T)::value;
        return tr ? frame_col_launch<TAIL, true>(c, cgrid, st) : frame_col_launch<TAIL, false>(c, cgrid, st);
    });
}
