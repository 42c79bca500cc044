// conv_bf_dev.h -- what the bf16 LDS-DMA convolution kernels (conv_bfd.hip, conv_bfs.hip, conv_bfw.hip, conv_bfg.hip) share beyond conv.h's
// lds_dma16 / eld_wait_vmcnt / bf16_line_swap: the tile width, the swizzled fragment offset of the 64-byte-row LDS images, the piece arithmetic of
// the halo tile (BfHalo), the fused 2x2 pool of one block (bf_pool_block), and the host-side launch of a persistent grid.  Ring depths, item order,
// the halo-unit tables and descriptors, and the block stores with their addressing stay in the kernels' own files.
#pragma once
#include "conv.h"

#define TW 32

namespace {

// Byte offset of lane (m, hi)'s fragment of k-block kb (channels 16 kb + 8 hi .. + 7 of a 32-channel chunk) in an LDS image of 64-byte rows whose
// four 16-byte units are XOR-swizzled by (row >> 2) & 3 (conv_bfd.hip, header): weight-slab rows (row = m) and, where a pixel is one row, the
// activation tiles (row = pixel or halo column).  The 16 lanes a ds_read_b128 services together then fall on 16 distinct slots of the bank row.
__device__ __forceinline__ unsigned bf_frag_off(int row, int kb, int hi) { return (unsigned)(row * 64 + (((kb * 2 + hi) ^ ((row >> 2) & 3)) * 16)); }

// The halo tile of a TH x TW pixel tile -- (TH + 2) x (TW + 2) pixels of one channel slice -- as conv_bfs / conv_bfw fetch it: in 16-byte units, UPP
// per pixel (4: a 32-channel chunk, 2: a 16-channel half chunk), 64 units to a linear 1 KiB LDS-DMA piece, the pieces dealt round-robin over WAVES
// waves (IT per wave).  One definition for the kernel's ring and the launcher's LDS size.  The unit table itself (which pixel and swizzled unit a lane
// fetches) and the per-image descriptor stay in the two kernels: profiles/r08_bf16_dev_notes.md section 3.
template <int UPP, int TH, int WAVES>
struct BfHalo {
    static constexpr int HW2 = TW + 2, UNITS = (TH + 2) * HW2 * UPP, PIECES = (UNITS + 63) / 64, BYTES = PIECES * 1024, IT = (PIECES + WAVES - 1) / WAVES;
    static constexpr unsigned OOB = 0xFFFFFFF0u;           // an offset past every image's descriptor: the DMA writes zeros
};

// Fused nn.MaxPool2d(2) of one 32-channel block of one MFMA column of 32 pixels (conv_bfd, conv_bfs, conv_bfw): vertical pair = two accumulator rows
// of the lane, horizontal pair in lane ^ 1, on the activated fp32 values (max commutes with the monotone bf16 rounding, so this equals pooling the
// stored tensor).  Every lane takes part; lanes of even x store w0 at channel 8 hi of the pooled pixel and w1 sixteen channels on.  (The block store
// itself -- slope multiply, pack_bf4, bf16_line_swap -- stays written out in the four files: same notes, section 3.)
__device__ __forceinline__ void bf_pool_block(const f32x16& r0, const f32x16& r1, uint4& w0, uint4& w1) {
    uint2 pk[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = fmax_lane_xor1(fmax_raw(r0[4 * q + j], r1[4 * q + j]));
        pk[q] = pack_bf4(make_float4(u[0], u[1], u[2], u[3]));
    }
    w0 = bf16_pair_swap(pk[0], pk[1]);
    w1 = bf16_pair_swap(pk[2], pk[3]);
}

// Launch KERN as a persistent grid: one workgroup per CU (fewer if there are fewer tiles), each walking tile ids blockIdx.x, + gridDim.x, ...
// tiles <= 0: nothing to do; tiles > max_tiles (what the kernel's item arithmetic holds in an int): ELD_ENOTSUP.  attr_lds_bytes = the dynamic LDS
// limit the kernel is given once per device (>= lds_bytes of every launch).  KERN is a template argument so that every kernel has its own once-flag.
template <auto KERN>
int launch_persistent(ConvArgs a, long long tiles, long long max_tiles, int threads, size_t attr_lds_bytes, size_t lds_bytes, hipStream_t st) {
    a.xcd = eld_xcd_mask() & XCD_BF16;
    if (tiles <= 0) return 0;
    if (tiles > max_tiles) return ELD_ENOTSUP;
    static EldAttrOnce once;
    { const int rc = once.ensure(KERN, attr_lds_bytes); if (rc) return rc; }
    long long grid = (long long)eld_num_cus();
    if (grid > tiles) grid = tiles;
    ELD_LAUNCH(KERN, dim3((unsigned)grid), dim3(threads), lds_bytes, st, a);
    ELD_LAUNCH_CHECK();
    return 0;
}

}  // namespace
