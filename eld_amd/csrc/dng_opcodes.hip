// dng_opcodes.hip -- the mosaic-domain DNG opcodes on the device (eld_amd/dng_opcodes.py): a compiled list-2 program applied
// to float32 frames in one pass, and the per-site product of the multiplicative opcodes as a gain plane.  The per-site arithmetic is
// dng_opcodes_dev.h, which a host compiler takes too; the kernel here is the tiling around it.
//
// One workgroup of 256 lanes owns a block of 128 rows x 256 columns and walks it in four tiles of 32 rows; a lane holds 8 rows x 4 columns of
// a tile in registers, runs the whole program on them and writes them back: 4 B read and 4 B written per site whatever the program's length
// (the gain plane reads no frame).  Everything an operation derives from the row alone or the column alone -- the area test, a GainMap's cell
// index and weight (two float64 divisions each), the entry of a per-row or per-column vector -- is computed once per row and per column of the
// block into LDS (an OpcAxis, 8 bytes, per operation and line), so a site pays two LDS reads instead of four float64 divisions per GainMap,
// and the column pass is shared by the four tiles.  The gains of the GainMaps are copied into LDS as long as they fit the budget (a phone's
// four 13 x 17 maps: 3.5 KB); a map beyond it is read from the blob in HBM / L2.
// The records travel as kernel arguments (32 x 104 bytes): every loop over them is wave-uniform, so they are scalar loads.
#include "common.h"
#include "dng_opcodes_dev.h"

namespace {

constexpr int OT = 256;                  // lanes of a workgroup
constexpr int OTX = 256, OTY = 32;       // the tile
constexpr int OBY = 128;                 // rows of a workgroup's block: OBY / OTY tiles, one column pass
constexpr int OROWS = OTY / (OT / ELD_WAVE);      // rows of a lane: a wave owns OROWS consecutive rows
constexpr int OCOLS = OTX / ELD_WAVE;    // columns of a lane
constexpr int OPC_DEFAULT_MAP_LDS = 32 << 10;
constexpr int OPC_MAX_MAP_LDS = 64 << 10;
static_assert(OCOLS == 4 && OT == OTX, "a lane loads one float4 per row and fills one column entry");

struct OpcArgs {
    const float* in;
    float* out;
    const uint8_t* blob;
    size_t blob_bytes;
    int Hm, Wm, nops;
    int map_off[ELD_DNG_MAX_OPS];        // where the operation's gains start in the LDS copy (floats), -1: read from the blob
    EldDngOp ops[ELD_DNG_MAX_OPS];
};

// VEC: rows are read and written as float4 (Wm a multiple of 4, 16-byte aligned frames); a lane's columns are then 4 tx .. 4 tx + 3.
// Otherwise a lane's columns are tx, tx + 64, ...: consecutive lanes on consecutive floats.
template <bool GAIN, bool VEC>
__global__ __launch_bounds__(OT) void opc_kernel(OpcArgs a) {
    extern __shared__ __align__(16) unsigned char opc_smem[];
    OpcAxis* rows = reinterpret_cast<OpcAxis*>(opc_smem);            // [nops][OBY]
    OpcAxis* cols = rows + (size_t)a.nops * OBY;                     // [nops][OTX]
    float* maps = reinterpret_cast<float*>(cols + (size_t)a.nops * OTX);
    const int tid = threadIdx.x, x0 = blockIdx.x * OTX, yb = blockIdx.y * OBY;
    uint32_t okmask = 0u;                                            // bit i: record i passed opc_record_ok and belongs to this entry point
    for (int i = 0; i < a.nops; ++i) {
        const EldDngOp& op = a.ops[i];
        const bool ok = opc_record_ok(op, a.blob_bytes, a.Hm, a.Wm) && (GAIN ? opc_is_gain_kind(op.kind) : op.kind != ELD_DNG_OP_VIGNETTE);
        okmask |= ok ? 1u << i : 0u;
        cols[i * OTX + tid] = opc_axis(op, ok && x0 + tid < a.Wm, a.blob, 1, x0 + tid, a.Hm, a.Wm);
        if (tid < OBY) rows[i * OBY + tid] = opc_axis(op, ok && yb + tid < a.Hm, a.blob, 0, yb + tid, a.Hm, a.Wm);
        if (ok && op.kind == ELD_DNG_OP_GAINMAP && a.map_off[i] >= 0) {
            const float* g = reinterpret_cast<const float*>(a.blob + op.data_off);
            const int n = op.n0 * op.n1;                             // the launcher sized the LDS copy from the same product
            for (int k = tid; k < n; k += OT) maps[a.map_off[i] + k] = g[k];
        }
    }
    __syncthreads();
    const int tx = tid & (ELD_WAVE - 1), ty = tid / ELD_WAVE;
    int cx[OCOLS];
#pragma unroll
    for (int j = 0; j < OCOLS; ++j) cx[j] = VEC ? OCOLS * tx + j : ELD_WAVE * j + tx;
    const size_t plane = (size_t)a.Hm * (size_t)a.Wm;
    const float* in = GAIN ? nullptr : a.in + (size_t)blockIdx.z * plane;
    float* out = a.out + (size_t)blockIdx.z * plane;
    for (int t = 0; t < OBY / OTY; ++t) {
        const int y0 = yb + t * OTY, r0 = t * OTY + ty * OROWS;      // the tile's first row; this wave's first row inside the block
        if (y0 >= a.Hm) break;
        float v[OROWS][OCOLS];
#pragma unroll
        for (int r = 0; r < OROWS; ++r) {
            const int y = yb + r0 + r;
#pragma unroll
            for (int j = 0; j < OCOLS; ++j) v[r][j] = 1.f;
            if (GAIN || y >= a.Hm) continue;
            const float* p = in + (size_t)y * (size_t)a.Wm + (size_t)x0;
            if (VEC) {
                if (x0 + cx[0] < a.Wm) {                             // Wm is a multiple of 4: the other three are inside too
                    const float4 q = *reinterpret_cast<const float4*>(p + cx[0]);
                    v[r][0] = q.x; v[r][1] = q.y; v[r][2] = q.z; v[r][3] = q.w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < OCOLS; ++j)
                    if (x0 + cx[j] < a.Wm) v[r][j] = p[cx[j]];
            }
        }
        for (int i = 0; i < a.nops; ++i) {
            if (!(okmask >> i & 1u)) continue;                       // scalar; none of a refused record's entries is addressed either
            const EldDngOp& op = a.ops[i];
            OpcAxis c[OCOLS];
#pragma unroll
            for (int j = 0; j < OCOLS; ++j) c[j] = cols[i * OTX + cx[j]];
            const bool lds = a.map_off[i] >= 0;                      // wave-uniform: the two branches read LDS resp. global memory
            const float* gl = reinterpret_cast<const float*>(a.blob + op.data_off);
            const float* gs = maps + (lds ? a.map_off[i] : 0);
#pragma unroll
            for (int r = 0; r < OROWS; ++r) {
                const OpcAxis rw = rows[i * OBY + r0 + r];           // one address per wave: a broadcast
                if (!(rw.idx & OPC_ADDRESSED)) continue;
                const int y = yb + r0 + r;
#pragma unroll
                for (int j = 0; j < OCOLS; ++j) {
                    if (!(c[j].idx & OPC_ADDRESSED)) continue;       // an entry is addressed only under a record that passed opc_record_ok
                    if (GAIN) {
                        const float f = lds ? opc_factor(op, gs, rw, c[j], y, x0 + cx[j], a.Hm, a.Wm)
                                            : opc_factor(op, gl, rw, c[j], y, x0 + cx[j], a.Hm, a.Wm);
                        v[r][j] = OPC_MUL(v[r][j], f);
                    } else if (v[r][j] == v[r][j]) {                 // a NaN site passes through
                        v[r][j] = lds ? opc_apply(op, a.blob, gs, rw, c[j], v[r][j]) : opc_apply(op, a.blob, gl, rw, c[j], v[r][j]);
                    }
                }
            }
        }
#pragma unroll
        for (int r = 0; r < OROWS; ++r) {
            const int y = yb + r0 + r;
            if (y >= a.Hm) continue;
            float* p = out + (size_t)y * (size_t)a.Wm + (size_t)x0;
            if (VEC) {
                if (x0 + cx[0] < a.Wm) *reinterpret_cast<float4*>(p + cx[0]) = make_float4(v[r][0], v[r][1], v[r][2], v[r][3]);
            } else {
#pragma unroll
                for (int j = 0; j < OCOLS; ++j)
                    if (x0 + cx[j] < a.Wm) p[cx[j]] = v[r][j];
            }
        }
    }
}

template <bool GAIN>
int opc_launch(const float* in, float* out, int N, int Hm, int Wm, const EldDngOp* ops, int nops, const uint8_t* blob, size_t blob_bytes,
               int map_lds_bytes, void* stream) {
    if (N < 0 || Hm < 1 || Wm < 1 || (uint64_t)Hm * (uint64_t)Wm >= (1ull << 31) || N > 65535) return ELD_EINVAL;
    if (nops < 0 || nops > ELD_DNG_MAX_OPS || (nops > 0 && !ops)) return ELD_EINVAL;
    if (blob_bytes > ELD_DNG_MAX_BLOB || (blob_bytes > 0 && !blob) || ((uintptr_t)blob & 7u)) return ELD_EINVAL;
    if (map_lds_bytes > OPC_MAX_MAP_LDS) return ELD_EINVAL;
    if (!out || ((uintptr_t)out & 3u) || (!GAIN && (!in || ((uintptr_t)in & 3u)))) return ELD_EINVAL;
    if (!GAIN && in != out) {                                        // in place, or apart
        const uintptr_t a0 = (uintptr_t)in, b0 = (uintptr_t)out, n = (uintptr_t)N * (uintptr_t)Hm * (uintptr_t)Wm * sizeof(float);
        if (a0 < b0 + n && b0 < a0 + n) return ELD_EINVAL;
    }
    OpcArgs a = {};
    int budget = (map_lds_bytes < 0 ? OPC_DEFAULT_MAP_LDS : map_lds_bytes) / (int)sizeof(float), used = 0;
    for (int i = 0; i < nops; ++i) {
        if (!opc_record_ok(ops[i], blob_bytes, Hm, Wm)) return ELD_EINVAL;
        if (GAIN ? !opc_is_gain_kind(ops[i].kind) : ops[i].kind == ELD_DNG_OP_VIGNETTE) return ELD_EINVAL;
        a.ops[i] = ops[i];
        a.map_off[i] = -1;
        if (ops[i].kind == ELD_DNG_OP_GAINMAP && ops[i].n0 * ops[i].n1 <= budget - used) {
            a.map_off[i] = used;
            used += ops[i].n0 * ops[i].n1;
        }
    }
    if (N == 0) return 0;
    a.in = in; a.out = out; a.blob = blob; a.blob_bytes = blob_bytes; a.Hm = Hm; a.Wm = Wm; a.nops = nops;
    const size_t lds = (size_t)nops * (OTX + OBY) * sizeof(OpcAxis) + (size_t)used * sizeof(float);
    const bool vec = Wm % 4 == 0 && !((uintptr_t)out & 15u) && (GAIN || !((uintptr_t)in & 15u));
    const dim3 grid((unsigned)((Wm + OTX - 1) / OTX), (unsigned)((Hm + OBY - 1) / OBY), (unsigned)N);
    if (grid.y > 65535u) return ELD_EINVAL;
    hipStream_t st = as_stream(stream);
    auto kern = vec ? opc_kernel<GAIN, true> : opc_kernel<GAIN, false>;
    if (lds > (48u << 10)) {                                         // a long program: more dynamic LDS than a launch gets by default
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    ELD_LAUNCH(kern, grid, dim3(OT), lds, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int eld_dng_opcodes_apply_f32(const float* in, float* out, int N, int Hm, int Wm, const EldDngOp* ops, int nops, const uint8_t* blob,
                                         size_t blob_bytes, int map_lds_bytes, void* stream) {
    return opc_launch<false>(in, out, N, Hm, Wm, ops, nops, blob, blob_bytes, map_lds_bytes, stream);
}

extern "C" int eld_dng_opcodes_gain_f32(float* out, int Hm, int Wm, const EldDngOp* ops, int nops, const uint8_t* blob, size_t blob_bytes,
                                        int map_lds_bytes, void* stream) {
    return opc_launch<true>(nullptr, out, 1, Hm, Wm, ops, nops, blob, blob_bytes, map_lds_bytes, stream);
}
