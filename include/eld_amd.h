/* eld_amd.h -- C ABI of libeld_amd.so: the MI355X (gfx950) hot path of ELD.
 *
 * The reference (Vandermode/ELD) has no FFI: its boundary for this path is three Python
 * duck-typed plugin points.  The Python package `eld_amd` implements those
 * plugin points and binds THIS header with ctypes; every entry point below names the reference
 * code it replaces (paths relative to the reference checkout).
 *
 * Conventions (all entry points):
 *   - plain C types only; device pointers are BORROWED (the caller, normally PyTorch's caching
 *     allocator, owns every allocation; scratch is passed in as `ws`);
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *     no hipMalloc / hipFree / hipDeviceSynchronize inside, so calls are hipGraph-capturable;
 *   - return value is a hipError_t as int (0 = success) or a negative ELD_E* code; nothing throws;
 *   - re-entrant per stream.  Process-wide state is limited to (a) immutable per-device caches (compute-unit count,
 *     per-kernel LDS attribute set once per device) and (b) the DEFAULT fp32 product scheme of eld_conv_fp32_algo(), which
 *     only the entry points that do not take a scheme argument consult; eld_unet_forward_ex / eld_unet_backward_ex name the
 *     scheme per call and never read it.  Developer switches (ELD_CONV_DBG, ELD_NOISE_DBG, eld_debug_conv_prof) exist only in
 *     builds made with -DELD_DEV_TOOLS=1; the default build ignores them.
 */
#ifndef ELD_AMD_H
#define ELD_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 6): eld_unet_infer_ex and eld_debug_ws_state_entries exist; the U-Net workspace grew (slope-code regions) -- size it with
 * eld_unet_workspace_bytes of the SAME library; eld_unet_backward_ex accepts an explicit dout after eld_unet_forward_loss_ex and refuses a backward
 * after eld_unet_infer_ex.  A binding must compare eld_abi_version() with the ELD_ABI_VERSION it was written against.
 * 3: ELD_CFA_XTRANS (row noise and colour bias on 9-plane X-Trans inputs) and the cell-statistics calibration entry points
 * (eld_calib_cell_*) exist; every version-2 call behaves as before.
 * 4: the write-back entry points (eld_unpack_raw_bayer_u16 / eld_unpack_raw_xtrans_u16, ELD_ROUND_*), the fused evaluation input stage
 * (eld_pack_raw_*_u16_gain) and the X-Trans ISP (eld_isp_process_xtrans) exist; every version-3 call behaves as before.
 * 5: the frame-pool crop entry points (eld_crop_pack_raw_bayer_u16 / eld_crop_pack_raw_xtrans_u16, EldPoolFrame, EldCropRecord) exist; every
 * version-4 call behaves as before.
 * 6: the full-resolution renders (eld_render_bayer / eld_render_xtrans, ELD_RENDER_*) and eld_debug_xtrans_demosaic_tables exist; every
 * version-5 call behaves as before.
 * 7: the defective-pixel entry points (eld_defect_deviation / eld_defect_flags / eld_defect_repair_u16, eld_debug_xtrans_defect_tables) exist;
 * every version-6 call behaves as before.
 * 8: the histogram entry points (eld_hist_u16 / eld_hist_f32) exist; every version-7 call behaves as before.
 * Still 8: eld_noise_forward_dark and ELD_DARK were added (signal-independent noise read from a pool of dark frames; EldNoiseParams.reserved
 * names the frame range) without a new number, because no existing call changed its signature, its record layout or its result: the one
 * difference is that ELD_DARK in the flags of the two older sampler entries is now ELD_EINVAL instead of an ignored bit.  A binding that needs
 * the new entry looks for its symbol (eld_amd/_lib.py binds every prototype at load and names the missing one with a rebuild hint).
 * Still 8: eld_struct_sums_u16 and eld_struct_cross_u16 were added (exact row, column, cell and frame-pair sums for the spatial structure of
 * noise) without a new number: two new symbols, no existing call changed in any way.  A binding finds them by symbol, as above.
 * Still 8: the dark-shading entry points (eld_shading_fit_u16, eld_shading_apply_u16, eld_pack_raw_bayer_u16_shaded,
 * eld_pack_raw_xtrans_u16_shaded) were added the same way: four new symbols, no existing call changed, so the Python binding, which binds
 * every symbol, needs a library built from this header or a later one (an older ABI-8 library fails at bind with the symbol's name).
 * Still 8: eld_pair_level_stats_u16 and eld_pair_level_stats_workspace_bytes were added the same way (exact error-versus-signal sums of an
 * estimate against a reference frame): two new symbols, no existing call changed.
 * Still 8: eld_burst_stack_u16 and eld_burst_stack_workspace_bytes were added the same way (robust mean and photon-transfer sums of a burst of
 * a static scene): two new symbols, no existing call changed.
 * Still 8: eld_burst_luma_pyramid_elems, eld_burst_luma_pyramid_u16, eld_burst_align_workspace_bytes, eld_burst_align_u16,
 * eld_burst_stack_aligned_workspace_bytes and eld_burst_stack_aligned_u16 were added the same way (registration of a hand-held burst and the
 * stack through its displacement field): six new symbols, no existing call changed.
 * Still 8: ELD_COL (model letter 'C', a per-sensor-column Gaussian), ELD_PLANE_NCOL and ELD_NPLANES_COL were added without a new number and
 * without a new symbol: no existing call, record layout or result changes.  The 64-byte EldNoiseParams keeps its layout; with ELD_COL in the
 * flags reserved[0] is read as the float bits of the column scale (ELD_COL and ELD_DARK, the field's other user, exclude each other), and the
 * inject / dump buffers then hold ELD_NPLANES_COL planes.  Without ELD_COL the field is ignored and the buffers hold ELD_NPLANES planes, as
 * before.  The one difference: bit 2048 in the flags of the sampler entries was ignored and now selects the term.
 * Still 8: eld_tile_noise_sums_u16 and eld_tile_noise_workspace_bytes were added the same way (exact per-tile second- and first-difference
 * sums of a single frame, for its gain and read noise): two new symbols, no existing call changed.
 * Still 8: eld_warp_rgb_f32 and EldWarp were added the same way (DNG WarpRectilinear on demosaiced camera RGB, followed by the renders' tail):
 * one new symbol, no existing call changed.
 * Still 8: eld_jpeg_coef_u8, eld_jpeg_hist_i16 and eld_jpeg_pack_i16 were added the same way (baseline JPEG of the uint8 sRGB render, encoded
 * on the device): three new symbols, no existing call changed.
 * Still 8: eld_render_bayer_edge and eld_render_bayer_edge_tile were added the same way (the full-resolution Bayer render behind an
 * edge-directed demosaic): two new symbols, no existing call changed.
 * Still 8: eld_frame_rgb_f32 and eld_frame_rgb_tile were added the same way (crop, antialiased resize and orientation of the full-resolution
 * render, followed by the renders' tail): two new symbols, no existing call changed. */
#define ELD_ABI_VERSION 8

/* negative = argument errors (hipError_t values are >= 0) */
#define ELD_EINVAL   (-1)   /* bad shape / flag combination / null pointer                   */
#define ELD_ENOTSUP  (-2)   /* valid request this build does not implement                    */
#define ELD_EWS      (-3)   /* workspace too small                                             */

/* ---- noise-model terms: letters of NoiseModel(model=...) (noise.py:158-166, 175) ----------- */
#define ELD_SHOT_POISSON  1u   /* 'P'  z = Poisson(y/K)*K                      noise.py:158-159 */
#define ELD_SHOT_GAUSS    2u   /* 'p'  z = y + N*sqrt(max(K*y,1e-10))          noise.py:160-161 */
#define ELD_READ_GAUSS    4u   /* 'g'  z += N*max(g_scale,1e-10)               noise.py:165-166 */
#define ELD_READ_TL       8u   /* 'G'  Tukey-lambda read noise   [withheld from the reference:  */
#define ELD_ROW          16u   /* 'R'  per-sensor-row Gaussian    README.md:41, noise.py:173;   */
#define ELD_QUANT        32u   /* 'U'  uniform quantisation noise  follows the ELD paper and    */
#define ELD_CBIAS        64u   /* 'B'  per-channel colour bias     camera_params/release/ npy tables] */
#define ELD_CLIP        128u   /* fuse the caller's clip to [0,1]       dataset/sid_dataset.py:277 */
#define ELD_AUG_NOTRANSPOSE 256u /* eld_augment only: no image of the batch has its transpose bit set (then H != W is fine) */
#define ELD_CFA_XTRANS  512u   /* the C == 9 input is in RawPacker.pack_raw_xtrans's plane layout (noise.py:22-64): ELD_ROW and
                                  ELD_CBIAS follow the X-Trans mosaic; without ELD_ROW / ELD_CBIAS / ELD_DARK it changes nothing */
#define ELD_DARK       1024u   /* 'D'  z += code - black: the signal-independent noise is a random crop of a real dark frame
                                  (eld_noise_forward_dark only; SFRN, Zhang et al., ICCV 2021) */
#define ELD_COL        2048u   /* 'C'  per-sensor-column Gaussian: z += N(column) * col_scale, directly after the row term.  col_scale is
                                  the float whose bits are EldNoiseParams.reserved[0].  Not with ELD_DARK; C == 4, or 9 with ELD_CFA_XTRANS */

/* input element types */
#define ELD_IN_F32  0   /* float32 in [0,1]                                                      */
#define ELD_IN_U16  1   /* uint16 LMDB code, decoded as clip(u16/65535,0,1) (lmdb_dataset.py:38-39) */

/* Per-image parameter record: the tuple returned by NoiseModel._sample_params (noise.py:225)
 * plus the withheld-model terms.  64 bytes. */
typedef struct EldNoiseParams {
    float K;            /* system gain (ADU per e-)                    noise.py:220           */
    float g_scale;      /* Gaussian read-noise std (ADU)               noise.py:221           */
    float tl_lambda;    /* Tukey-lambda shape        ('G_shape')                              */
    float tl_scale;     /* Tukey-lambda scale (ADU)  ('G_scale' regression)                   */
    float row_scale;    /* row-noise std (ADU)       ('R_scale' regression)                   */
    float q_step;       /* quantisation step (ADU), 1                                         */
    float saturation;   /* 16383-800                                   noise.py:205           */
    float ratio;        /* exposure ratio                              noise.py:223           */
    float color_bias[4];/* per packed channel (ADU)  ('color_bias'); ELD_CFA_XTRANS: (R, G, B) per CFA colour, [3] unused */
    uint32_t sample_id_lo, sample_id_hi;  /* GLOBAL sample index -> Philox counter words 1,2  */
    uint32_t reserved[2];                 /* ELD_DARK: first index and count of the frame-table range this image draws from; ELD_COL: [0] =
                                             the bits of the float32 column-noise std (ADU) ('C_scale' regression); else ignored */
} EldNoiseParams;

/* Variate planes of the debug/inject buffers: float[ELD_NPLANES][N*C*H*W]. */
#define ELD_PLANE_COUNT   0   /* Poisson count (as float)        */
#define ELD_PLANE_NSHOT   1   /* N(0,1) of the 'p' term          */
#define ELD_PLANE_NREAD   2   /* N(0,1) of the 'g' term          */
#define ELD_PLANE_TL      3   /* unit-scale Tukey-lambda variate */
#define ELD_PLANE_NROW    4   /* row normal, broadcast per pixel */
#define ELD_PLANE_UQ      5   /* quantisation uniform in [0,1)   */
#define ELD_NPLANES       6
#define ELD_PLANE_NCOL    6   /* column normal, broadcast per pixel: present only with ELD_COL in the flags */
#define ELD_NPLANES_COL   7   /* planes of the inject / dump buffers when ELD_COL is set (ELD_NPLANES otherwise) */

int eld_abi_version(void);
const char* eld_build_info(void);               /* "gfx950 hipcc <ver> ..." */
const char* eld_error_string(int code);

/* Fused per-pixel noise sampler.  Replaces NoiseModelBase.__call__ (noise.py:149-170), batched:
 *   in     N*C*H*W elements, NCHW contiguous (packed raw: C=4 Bayer planes), type `in_dtype`
 *   out    float32, same shape.  NOT clipped unless ELD_CLIP (the reference's callers clip).
 *   params device array of N records
 *   seed   Philox key; counters come from (element index, params[n].sample_id), so the output
 *          does not depend on launch geometry or on how images are spread over GPUs
 *   inject optional float[ELD_NPLANES][numel]: take the variates from here instead of Philox
 *          (deterministic-arithmetic parity against the reference's own draws)
 *   dump   optional float[ELD_NPLANES][numel]: also write the variates that were used
 * ELD_ROW and ELD_CBIAS require C == 4 (Bayer packing: channels 0,1 <- sensor row 2h, 2,3 <- 2h+1; noise.py:16-19), or C == 9 with
 * ELD_CFA_XTRANS.  X-Trans: packed row i holds sensor rows 3i..3i+2; element (c, i, j) reads sensor row 3i + d, d = 0 for planes
 * 0-2, 1 for 5-6, 2 for 7-8, and for planes 3 / 4 d = 1 / 2 where i + j is even, 2 / 1 where it is odd.  Its row normal is
 * the one of that sensor row (same Philox counter layout as Bayer's, indexed by the sensor row).  The colour bias of plane c
 * is color_bias[colour of c]: planes 0, 3 R; 2, 4 B; 1, 5-8 G.  ELD_CFA_XTRANS with C != 9 is ELD_EINVAL.
 * ELD_COL has the same shape requirement.  Its index is the patch-local sensor column: Bayer element (c, h, w) sits on column
 * 2w + ((c ^ (c >> 1)) & 1) (planes 0 and 3 even, 1 and 2 odd); X-Trans element (c, i, j) on the mosaic column eld_pack_xtrans reads for
 * it, 3j + d with d = 2 for planes 1, 3, 4; 0 for 5, 7; 1 for 6, 8; and for planes 0 / 2 d = 0 / 1 where i + j is even, 1 / 0 where it is
 * odd.  The normal of a column is a function of (seed, sample id, column) only (Philox stream 9, words 0 and 1, the row transform); planes
 * that share a sensor column share it.  zz = zz + n_col * col_scale follows the row term directly (float32, one rounding per operation).
 * ELD_COL with ELD_DARK is ELD_EINVAL. */
int eld_noise_forward(const void* in, int in_dtype, float* out, const EldNoiseParams* params,
                      int N, int C, int H, int W, uint32_t flags, uint64_t seed,
                      const float* inject, float* dump, void* stream);

/* The same sampler with explicit image strides (in ELEMENTS): image n is read at in + n*in_image_stride and written at
 * out + n*out_image_stride.  Burst synthesis (SynDataset, dataset/sid_dataset.py:267-273: num_burst noisy frames of ONE clean
 * image with ONE parameter draw, concatenated on the channel axis) is num_burst launches with out_image_stride =
 * num_burst*C*H*W and out advanced by k*C*H*W, each with its own sample ids; in_image_stride 0 re-reads one clean image. */
int eld_noise_forward_strided(const void* in, int in_dtype, size_t in_image_stride, float* out, size_t out_image_stride,
                              const EldNoiseParams* params, int N, int C, int H, int W, uint32_t flags, uint64_t seed,
                              const float* inject, float* dump, void* stream);

/* Rounds of the Philox4x32 generator this build's sampler runs (7 since round 3 of this library; -DELD_PHILOX_ROUNDS=10 restores
 * cuRAND's count).  The noise stream of a (seed, sample id) pair is a function of this number: a binding that pins or replays streams
 * (checkpoints, golden vectors, the test oracle) must compare it with the count it was made for -- eld_amd/_lib.py does at load time. */
int eld_philox_rounds(void);

/* Raw Philox4x32-7 words (ELD_PHILOX_ROUNDS, csrc/philox.h) of the sampler's counter layout, for bit-exact RNG tests:
 * out[i*4..i*4+3] = philox(ctr=(index0+i, sample_id, stream|iter<<8), key=seed). */
int eld_philox_words(uint32_t* out, uint32_t n, uint32_t index0, uint64_t sample_id,
                     uint32_t stream, uint32_t iter, uint64_t seed, void* stream_h);

/* Bayer pack / unpack.  Replaces RawPacker.pack_raw_bayer / unpack_raw_bayer (noise.py:10-20,66-81),
 * batched: mosaic float32 [N,2h,2w] <-> packed float32 [N,4,h,w]. */
int eld_pack_bayer(const float* mosaic, float* packed, int N, int h, int w, void* stream);
int eld_unpack_bayer(const float* packed, float* mosaic, int N, int h, int w, void* stream);
/* X-Trans pack / unpack.  Replaces RawPacker.pack_raw_xtrans / unpack_raw_xtrans (noise.py:22-64, 83-127), batched:
 * mosaic float32 [N,Hm,Wm] -> packed float32 [N,9,2*(Hm/6),2*(Wm/6)] (the reference truncates to whole 6x6 cells, noise.py:25-26);
 * packed float32 [N,9,h,w] -> mosaic float32 [N,3h,3w].  Index maps only: bit-exact. */
int eld_pack_xtrans(const float* mosaic, float* packed, int N, int Hm, int Wm, void* stream);
int eld_unpack_xtrans(const float* packed, float* mosaic, int N, int h, int w, void* stream);
/* pack_raw_bayer (dataset/sid_dataset.py:172-196): uint16 sensor mosaic [N,2h,2w] (raw.raw_image_visible) -> packed float32
 * [N,4,h,w] in the order R, G1, B, G2 given by the 2x2 `raw_pattern` (row-major colour codes 0..3, HOST array of 4 ints),
 * normalised per channel: clip((x - black_level[k]) / (white_point - black_level[k]), 0, 1), float32 arithmetic as NumPy's
 * (black_level: HOST array of 4 floats = raw.black_level_per_channel; white_point 16383 in the reference).  Bit-exact. */
int eld_pack_raw_bayer_u16(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern,
                           const float* black_level, float white_point, void* stream);
/* The X-Trans branch of the same dataset pack (dataset/sid_dataset.py:199-239): uint16 sensor mosaic [N,Hm,Wm] -> packed float32
 * [N,9,2*(Hm/6),2*(Wm/6)] (eld_pack_xtrans's index map; sides truncated to whole 6x6 cells) of
 * clip((x - black_level) / (white_point - black_level), 0, 1), float32 arithmetic as NumPy's (one black level for all planes;
 * 1024 / 16383 in the reference).  white_point must exceed black_level.  Bit-exact. */
int eld_pack_raw_xtrans_u16(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point, void* stream);
/* The evaluation input stage of dataset/sid_dataset.py:398-409 in one pass: the pack above, then min(max(p * ratios[n], 0), 1) in float32
 * (bit-identical to NumPy's np.maximum(np.minimum(pack * np.float32(ratio), 1), 0)).  ratios: DEVICE array of N float32 exposure
 * ratios, one per image. */
int eld_pack_raw_bayer_u16_gain(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern,
                                const float* black_level, float white_point, const float* ratios, void* stream);
int eld_pack_raw_xtrans_u16_gain(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point,
                                 const float* ratios, void* stream);

/* Write-back: a packed network output in [0, 1] -> uint16 sensor codes, the inverse of the two packs above (the mosaic half of the
 * reference's postprocess_bayer / postprocess_xtrans, models/ELD_model.py:41-129).  Per element, with the black level b of the element's
 * channel and the white point w (integers, 0 <= b < w <= 65535):
 *     v = double(clip(x, 0, 1)) * (w - b) + b          (exact in double: a 24-bit mantissa times w - b < 2^16, plus b)
 * then, by `rounding`:
 *     ELD_ROUND_TRUNC      truncation toward zero -- the reference's assignment of its float64 Bayer expression into the uint16
 *                          raw_image_visible, bit for bit;
 *     ELD_ROUND_NEAREST    round half to even;
 *     ELD_ROUND_TRUNC_F32  fl32(fl32(x * (w - b)) + b) truncated -- the reference's X-Trans expression (its black / white are Python
 *                          ints, which leave the float32 array float32), bit for bit.
 * Measured (NumPy, exhaustive over the codes): pack followed by a truncating float64 write-back is NOT the identity -- of the 15872
 * codes in [512, 16383], 7893 come back one DN low (7676 of 15360 for black 1024); with ELD_ROUND_NEAREST every code in [b, w]
 * round-trips, for (b, w) = (512, 16383), (1024, 16383), (2048, 16383) and (0, 65535); the float32 X-Trans expression round-trips
 * those codes too.  A NaN writes b.
 * Bayer: packed [N,4,h,w] -> mosaic [N,2h,2w], every pixel written; raw_pattern (HOST, 4 ints, a permutation of 0..3) and black_level
 * (HOST, 4 floats, per channel) as eld_pack_raw_bayer_u16.
 * X-Trans: packed [N,9,2*(Hm/6),2*(Wm/6)] -> the pixels of the whole 6x6 cells of mosaic [N,Hm,Wm] (eld_pack_xtrans's index map); the
 * rows / columns beyond the last whole cell are not written, so a mosaic that already holds the input frame keeps its codes there, as
 * the reference's in-place write into raw_image_visible does.  packed must be 8-byte aligned. */
#define ELD_ROUND_TRUNC      0
#define ELD_ROUND_NEAREST    1
#define ELD_ROUND_TRUNC_F32  2
int eld_unpack_raw_bayer_u16(const float* packed, uint16_t* mosaic, int N, int h, int w, const int* raw_pattern,
                             const float* black_level, float white_point, int rounding, void* stream);
int eld_unpack_raw_xtrans_u16(const float* packed, uint16_t* mosaic, int N, int Hm, int Wm, float black_level, float white_point,
                              int rounding, void* stream);

/* ---- frame pool: training patches cut from device-resident mosaics (eld_amd/framepool.py) ----------------------
 * What util/lmdb_data.py::create_lmdb_train stores in its patch databases, made on the device from the sensor's own uint16 mosaics:
 * pack (:24-98), x ratio, clip, x 65535, astype(uint16) (:201-210), bit for bit.  The dtypes are the reference's and differ by CFA:
 *   Bayer    float32 throughout: p = clip((float32(u) - b_k) / (white - b_k), 0, 1); p = clip(fl32(p * ratio), 0, 1);
 *            code = trunc(fl32(p * 65535))
 *   X-Trans  p is the same float32 value (one black level); the reference packs it into a float64 array (:62), so
 *            code = trunc(clip(double(p) * double(ratio), 0, 1) * 65535.0), both products in float64
 * ratio 1 gives the codes of the chain without the ratio multiply (x * 1 is exact).
 *   pool     one flat DEVICE uint16 buffer of pool_elems codes, 16-byte aligned, holding F mosaics
 *   frames   DEVICE table of F entries: element offset of the mosaic in the pool (even), its sides Hm x Wm (Wm even).  The packed extent of
 *            a frame is (Hm/2) x (Wm/2) for Bayer and 2*(Hm/6) x 2*(Wm/6) for X-Trans (whole 6x6 cells only, eld_pack_xtrans's index map)
 *   max_h, max_w   HOST: the largest packed extent over the frames (what the entry can check a patch size against)
 *   recs     DEVICE array of B records (B <= 65535): frame index, y0, x0 in PACKED coordinates -- any values, odd ones included -- and the ratio
 *   out      DEVICE uint16 [B, C, ph, pw], C = 4 (R, G1, B, G2 by raw_pattern, as eld_pack_raw_bayer_u16) or 9; 16-byte aligned
 * ELD_EINVAL before any launch for what the host can see: zero or negative sizes, ph > max_h or pw > max_w, a raw_pattern that is not a
 * permutation of 0..3, white_point <= a black level or > 65535, null or misaligned pointers.  The records and the frame table are device
 * memory: a record that does not describe a patch inside its frame, or a frame entry that does not lie inside the pool, makes the kernel
 * SKIP that patch (its slice of `out` is not written); nothing outside the pool is ever read.
 * pw % 8 == 0 takes the 16-byte-store kernel; per patch it reads 16 bytes per load when (offset + 2 x0) % 8 == 0 (X-Trans: offset + 3 x0)
 * and Wm % 8 == 0, and 4 bytes per load otherwise.  Any other pw takes a one-code-per-lane kernel. */
typedef struct EldPoolFrame { uint64_t offset; int32_t Hm, Wm; } EldPoolFrame;                 /* 16 bytes */
typedef struct EldCropRecord { int32_t frame, y0, x0; float ratio; } EldCropRecord;            /* 16 bytes */
int eld_crop_pack_raw_bayer_u16(const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int max_h, int max_w,
                                const EldCropRecord* recs, int B, int ph, int pw, const int* raw_pattern, const float* black_level,
                                float white_point, uint16_t* out, void* stream);
int eld_crop_pack_raw_xtrans_u16(const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int max_h, int max_w,
                                 const EldCropRecord* recs, int B, int ph, int pw, float black_level, float white_point, uint16_t* out,
                                 void* stream);

/* ---- the sampler with the sensor's own dark frames (ELD_DARK, model letter 'D') -------------------------------------
 * eld_noise_forward_strided plus one term: every signal-independent component (read noise, banding, fixed pattern, colour bias) is taken
 * from a random crop of a real dark frame held in a frame pool, in the same pass:
 *     zz = shot term;  zz = zz + (float(code) - black_c);  [ELD_QUANT: zz = zz + (u - 0.5) * q_step];  zz = zz * ratio;  zz = zz / S;  [clip]
 * float32, one rounding per operation.  black_c is the NOMINAL black level of the plane (black_level[c]; X-Trans: black_level[0]), so the
 * sensor's colour bias stays in the sample.  ELD_QUANT here is the dither that undoes the dark frame's own quantisation.  `inject` does
 * not reach this term (the code is data, not a variate).
 *   pool, pool_elems, frames, F   the frame pool's buffer and table, as eld_crop_pack_raw_*_u16 (same alignment rules)
 *   min_h, min_w   HOST: the smallest packed extent over the frames; H > min_h or W > min_w is ELD_EINVAL
 *   raw_pattern, black_level   as eld_pack_raw_bayer_u16 (HOST arrays of 4); ELD_CFA_XTRANS: raw_pattern is ignored (may be null)
 *   params[n].reserved[0], [1]   first index and count of the contiguous range of `frames` image n may draw from (its session)
 * The crop is chosen by the kernel, uniformly over the block, from w = Philox(index 0, sample id, stream 8):
 *     f = first + umulhi(w.x, count);  (hp, wp) = packed extent of frame f
 *     Bayer    y0 = umulhi(w.y, hp - H + 1),            x0 = umulhi(w.z, wp - W + 1)             (odd offsets included)
 *     X-Trans  y0 = 2 umulhi(w.y, (hp - H) / 2 + 1),    x0 = 2 umulhi(w.z, (wp - W) / 2 + 1)     (a patch starts on a 6x6 cell)
 * and element (c, h, w) reads the mosaic site that packed element (c, y0 + h, x0 + w) of frame f packs from (eld_pack_raw_bayer_u16's map by
 * raw_pattern; eld_pack_xtrans's index map).  The choice is a function of (seed, sample id) alone.
 * ELD_EINVAL before any launch: ELD_DARK with ELD_READ_GAUSS, ELD_READ_TL, ELD_ROW or ELD_CBIAS (those terms would be counted twice); C other
 * than 4, or other than 9 with ELD_CFA_XTRANS; a null or misaligned pool or table; F <= 0; H > min_h or W > min_w; a raw_pattern that is not a
 * permutation of 0..3; a null or negative black level.  On the device: a record whose range is empty or leaves the table, a frame smaller
 * than the patch, and a frame entry that leaves the pool (or has an odd offset / row pitch) make the kernel SKIP that image: its slice
 * of `out` is not written, and nothing outside the pool is read.
 * W % 4 == 0 (Bayer): a lane's four packed elements are eight consecutive codes of one mosaic row, read as one 16-byte load when
 * (offset + 2 x0) % 8 == 0 and Wm % 8 == 0, and as four 4-byte loads otherwise.  Without ELD_DARK in `flags` the pool arguments are ignored. */
int eld_noise_forward_dark(const void* in, int in_dtype, size_t in_image_stride, float* out, size_t out_image_stride,
                           const EldNoiseParams* params, int N, int C, int H, int W, uint32_t flags, uint64_t seed,
                           const float* inject, float* dump,
                           const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int min_h, int min_w,
                           const int* raw_pattern, const float* black_level, void* stream);

/* ---- noise-parameter calibration (eld_amd/calibrate.py; estimators: DESIGN.md "Calibration") ------------------------------
 * Inputs are uint16 Bayer sensor mosaics [F,Hm,Wm] with even sides; packed channel of pixel (y,x) = raw_pattern[y&1][x&1] (HOST
 * array of 4 ints, a permutation of 0..3: R, G1, B, G2), as eld_pack_raw_bayer_u16.  Integer sums are exact (uint64 / int64, equal
 * to NumPy int64 bit for bit); float64 sums are reduced in an order fixed by the shape, without atomics: two calls give identical bits.
 * The mosaics are read as 32-bit words (two pixels): `u` and `ab` must be 4-byte aligned (ELD_EINVAL otherwise), the residual `t` 8-byte
 * aligned; PyTorch allocations are, a view that starts at an odd element is not.
 *
 * Bias statistics: chan_sums[F][4][2] = (sum u, sum u^2) per frame and channel; row_sums[F][Hm][2] = sum u over the even / odd
 * columns of each mosaic row.  Workspace: eld_calib_bias_stats_workspace_bytes(F, Hm). */
size_t eld_calib_bias_stats_workspace_bytes(int F, int Hm);
int eld_calib_bias_stats(const uint16_t* u, int F, int Hm, int Wm, const int* raw_pattern, uint64_t* chan_sums, uint64_t* row_sums, void* ws, size_t ws_bytes, void* stream);
/* Bias residual: t[f][y][x] = float32(((u - black_level[c]) - color_bias[f][c]) - row_offset[f][y]), float64 arithmetic rounded once
 * (black_level: HOST array of 4 doubles; color_bias: device double[F][4]; row_offset: device double[F][Hm]; t: float32 [F,Hm,Wm]). */
int eld_calib_bias_residual(const uint16_t* u, int F, int Hm, int Wm, const int* raw_pattern, const double* black_level, const double* color_bias, const double* row_offset, float* t, void* stream);
/* Flat pairs ab [P][2][Hm][Wm] (a = ab[p][0], b = ab[p][1]): out[P][4][4] = per channel (sum(a+b), sum(a-b), sum((a-b)^2),
 * #pixels with a >= white_level or b >= white_level).  Workspace: eld_calib_flat_stats_workspace_bytes(P, Hm). */
size_t eld_calib_flat_stats_workspace_bytes(int P, int Hm);
int eld_calib_flat_stats(const uint16_t* ab, int P, int Hm, int Wm, const int* raw_pattern, int white_level, int64_t* out, void* ws, size_t ws_bytes, void* stream);
/* Tukey-lambda probability-plot sums of F sorted rows t_sorted[F][n] (n >= 3) against the quantiles M_lam(m_i) at Filliben's medians
 * m_i, for the L shapes lambdas[L] (device float32): sums[F][L][2] = (sum t*M, sum M^2), tsums[F][2] = (sum t, sum t^2); sum M = 0
 * exactly (the quantiles are built antisymmetric).  PPCC r = sum tM / sqrt(sum M^2 (sum t^2 - (sum t)^2/n)); probplot slope =
 * sum tM / sum M^2.  Workspace: eld_calib_ppcc_workspace_bytes(F, n, L). */
size_t eld_calib_ppcc_workspace_bytes(int F, size_t n, int L);
int eld_calib_ppcc(const float* t_sorted, int F, size_t n, const float* lambdas, int L, double* sums, double* tsums, void* ws, size_t ws_bytes, void* stream);
/* Cell statistics of a mosaic pattern of period p (2 or 6; anything else is ELD_EINVAL), for any CFA (X-Trans: p = 6).  They know
 * nothing about colours: cell (r, c) is the set of pixels (y, x) with y % p == r, x % p == c, and the host folds cells into colours.
 * The Bayer entry points above are these passes at p = 2, with the cells stored in the channel order of raw_pattern (and the Bayer
 * argument rules: even Hm, a permutation pattern).  Same rules here: exact integer sums, fixed reduction order, 4-byte aligned `u` /
 * `ab`, Wm even; Hm and Wm need not be multiples of p.
 *
 * cell_sums[F][p][p][2] = (sum u, sum u^2) per frame and cell; row_sums[F][Hm][p] = sum u over the columns x % p == c of each row.
 * Workspace: eld_calib_cell_stats_workspace_bytes(F, Hm, p). */
size_t eld_calib_cell_stats_workspace_bytes(int F, int Hm, int p);
int eld_calib_cell_stats(const uint16_t* u, int F, int Hm, int Wm, int p, uint64_t* cell_sums, uint64_t* row_sums, void* ws, size_t ws_bytes, void* stream);
/* Cell residual: t[f][y][x] = float32(((u - black[k]) - cell_bias[f][k]) - row_offset[f][y]), k = (y % p) * p + x % p, float64
 * arithmetic rounded once (black: HOST array of p*p doubles; cell_bias: device double[F][p*p]; row_offset: device double[F][Hm]). */
int eld_calib_cell_residual(const uint16_t* u, int F, int Hm, int Wm, int p, const double* black, const double* cell_bias, const double* row_offset, float* t, void* stream);
/* Flat pairs ab [P][2][Hm][Wm]: out[P][p][p][4] = per cell (sum(a+b), sum(a-b), sum((a-b)^2), #pixels with a or b >= white_level).
 * Workspace: eld_calib_cell_flat_stats_workspace_bytes(P, Hm, p). */
size_t eld_calib_cell_flat_stats_workspace_bytes(int P, int Hm, int p);
int eld_calib_cell_flat_stats(const uint16_t* ab, int P, int Hm, int Wm, int p, int white_level, int64_t* out, void* ws, size_t ws_bytes, void* stream);


/* Training-pair augmentation of ELDTrainDataset.__getitem__ (dataset/sid_dataset.py:344-352), batched on device:
 * per image n, bits of aug[n]: 1 = flip H (axis 1), 2 = flip W (axis 2), 4 = transpose (0,2,1), applied in that order;
 * ELD_CLIP in `flags` fuses the clip to [0,1] of sid_dataset.py:354.  A transposed image needs H == W (batched tensor): with
 * H != W the call returns ELD_ENOTSUP unless ELD_AUG_NOTRANSPOSE is set, which makes the kernel ignore bit 4.
 * in/out: float32 [N,C,H,W]; aug: device int32[N].  Pure index map: bit-exact. */
int eld_augment(const float* in, float* out, const int32_t* aug, int N, int C, int H, int W, uint32_t flags, void* stream);
/* The same on uint16 LMDB codes: out = augment(clip(u16/65535, 0, 1)) -- LMDBDataset.__getitem__'s decode (dataset/lmdb_dataset.py:
 * 35-39, true fp32 division: bit-exact for all 65536 codes) fused in front; aug == NULL is the plain decode. */
int eld_augment_u16(const uint16_t* in, float* out, const int32_t* aug, int N, int C, int H, int W, uint32_t flags, void* stream);

/* ====================================================================================================
 * U-Net ("See-in-the-Dark", 5 scales) -- replaces UNetSeeInDark.forward (models/arch/Unet.py:48-91) and
 * the autograd backward that ELDModel.backward_G triggers (models/ELD_model.py:411-420).
 *
 * Parameters live in ONE flat float32 buffer, tensors in the reference's named_parameters() order
 * (conv1_1.weight, conv1_1.bias, ... conv5_2, upv6, conv6_1, conv6_2, ... upv9, conv9_1, conv9_2, conv10_1),
 * each in the reference's own layout (Conv2d OIHW, ConvTranspose2d (Cin,Cout,2,2)), so a state_dict
 * maps onto it by plain views (models/ELD_model.py:516-523) and a data-parallel gradient all-reduce is
 * one contiguous buffer.  Activations are kept NHWC float32 in the caller-provided workspace.
 * x / out / dout are NCHW float32 like the reference's tensors.  H and W must be multiples of 16.
 * Channels: 1 <= in_ch <= 16 and 1 <= out_ch <= 16 in both precisions (4 -> 4 Bayer; 9 -> 9 X-Trans, ELD_model.py:377-391;
 * num_burst x 4 burst inputs); outside that range eld_unet_param_offsets returns ELD_EINVAL and eld_unet_workspace_bytes 0.
 * ==================================================================================================== */
#define ELD_UNET_NTENSORS 46

/* offsets[i] = first float of tensor i in the flat buffer, offsets[46] = total count (7,760,484 for 4->4). */
int eld_unet_param_offsets(int in_ch, int out_ch, int64_t* offsets /* [ELD_UNET_NTENSORS+1] */);
/* bytes of scratch eld_unet_forward/backward need for this shape (packed weights, activations, gradients, partials) */
size_t eld_unet_workspace_bytes(int N, int H, int W, int in_ch, int out_ch);
int eld_unet_forward(const float* x, const float* params, float* out, void* ws, size_t ws_bytes,
                     int N, int H, int W, int in_ch, int out_ch, void* stream);
/* Inference in bf16 (BASELINE config 3's precision): bf16 NHWC activations and packed weights on v_mfma_f32_32x32x16_bf16,
 * fp32 accumulation, bias, first-layer input and output.  Same arguments and workspace as eld_unet_forward; the saved
 * activations are bf16: follow it with eld_unet_backward_bf16, never with eld_unet_backward. */
int eld_unet_forward_bf16(const float* x, const float* params, float* out, void* ws, size_t ws_bytes,
                          int N, int H, int W, int in_ch, int out_ch, void* stream);
/* Backward of a bf16 forward: bf16 activation gradients on the bf16 MFMA; parameter gradients are accumulated and
 * written in fp32 (fp32 master weights and Adam are unchanged).  Same contract as eld_unet_backward. */
int eld_unet_backward_bf16(const float* dout, const float* params, float* grads, void* ws, size_t ws_bytes,
                           int N, int H, int W, int in_ch, int out_ch, void* stream);
/* Needs the workspace exactly as eld_unet_forward left it (saved activations).  Writes every element of grads. */
int eld_unet_backward(const float* dout, const float* params, float* grads, void* ws, size_t ws_bytes,
                      int N, int H, int W, int in_ch, int out_ch, void* stream);

/* eld_unet_backward / eld_unet_backward_bf16 (precision 0 / 1) for data-parallel training (the reference is
 * single-device, models/ELD_model.py:187-190): the flat gradient buffer is cut into n_buckets contiguous buckets starting at the
 * ascending float offsets bucket_start[k] (bucket k = [bucket_start[k], bucket_start[k+1]) ; the last one runs to the end;
 * bucket_start[0] is normally 0).  Gradients are produced from the END of the buffer towards its start, and
 * hipEventRecord(bucket_event[k], stream) is enqueued as soon as the last kernel writing bucket k is enqueued, so a
 * communication stream can wait on the events and all-reduce bucket by bucket while the rest of the backward runs.
 * bucket_event[k]: hipEvent_t created by the caller. */
int eld_unet_backward_buckets(const float* dout, const float* params, float* grads, void* ws, size_t ws_bytes,
                              int N, int H, int W, int in_ch, int out_ch, int precision,
                              const int64_t* bucket_start, void* const* bucket_event, int n_buckets, void* stream);

/* Training forward with the loss fused into the head (ELD_model.py:469-475: forward() + backward_G()'s loss): as eld_unet_forward_ex with the
 * activations kept for the backward, but the last layer (conv10_1, Unet.py:46,88), the loss against `target` (loss_kind 0: nn.L1Loss, 1:
 * nn.MSELoss, models/losses.py:30-34; mean over all elements, written to *loss on the device) and the head's own backward run as ONE pass over
 * conv9_2's output: `out` is written, the output gradient never touches memory, the gradient of conv9_2's output and the head's weight-gradient
 * partials stay in the workspace.  Follow with eld_unet_backward_ex(dout = NULL, same workspace, same shape / precision), which finishes the
 * head's dW / db and runs the rest of the backward.  grad_scale multiplies dLoss/dout (1 for a plain mean loss).
 * The pair shares more than the head: the forward packs the weights for both directions in one launch (the backward differentiates at the
 * parameters the forward ran with), and the backward's first-layer weight gradient reads `x` where the forward read it -- no copy of the input is
 * kept in the workspace.  `x` (and `params`) must therefore stay valid and unchanged until the backward that follows this forward on the
 * workspace has been enqueued on the same stream -- the matching eld_unet_backward_ex(dout = NULL), or a backward with an explicit dout
 * (allowed: the head is then recomputed from dout, the weights are packed again, and the first layer's weight gradient still reads `x`
 * from the caller). */
int eld_unet_forward_loss_ex(const float* x, const float* params, const float* target, float* out, float* loss, void* ws, size_t ws_bytes,
                             int N, int H, int W, int in_ch, int out_ch, int precision, int fp32_algo, int loss_kind, float grad_scale, void* stream);
/* The same two calls with everything per call: precision 0 = fp32 / 1 = bf16 activations; fp32_algo names the fp32 product
 * scheme (see eld_conv_fp32_algo below; < 0 = the process default); n_buckets may be 0.  A backward must name the scheme its
 * forward ran with: scheme 2 leaves operand bounds in the workspace that only a scheme-2 backward reads.
 * eld_unet_backward_ex accepts dout == NULL when (and only when) the LAST forward on this workspace (host call order) was
 * eld_unet_forward_loss_ex with the same N / H / W / channels / precision; otherwise it returns ELD_EINVAL (the library remembers, per
 * workspace pointer, which forward filled it -- host bookkeeping, no device read). */
int eld_unet_forward_ex(const float* x, const float* params, float* out, void* ws, size_t ws_bytes,
                        int N, int H, int W, int in_ch, int out_ch, int precision, int fp32_algo, void* stream);
int eld_unet_backward_ex(const float* dout, const float* params, float* grads, void* ws, size_t ws_bytes,
                         int N, int H, int W, int in_ch, int out_ch, int precision, int fp32_algo,
                         const int64_t* bucket_start, void* const* bucket_event, int n_buckets, void* stream);
/* The forward under torch.no_grad() (ELD_model.py:203-307 eval / test: `self.netG(self.input)` with nothing kept): eld_unet_forward_ex's arguments and
 * bit-identical output, but nothing a backward would need is produced -- no copy of the input in the workspace, no slope codes (round 5: the training
 * forwards also write 2 bits per element of four activations for the backward-data epilogues).  eld_unet_backward_ex on a workspace whose last forward was
 * this call returns ELD_EINVAL. */
int eld_unet_infer_ex(const float* x, const float* params, float* out, void* ws, size_t ws_bytes,
                      int N, int H, int W, int in_ch, int out_ch, int precision, int fp32_algo, void* stream);

/* How the fp32 3x3 convolutions of eld_unet_forward/backward and eld_conv3x3_* form their products:
 *   0  v_mfma_f32_32x32x2_f32 (fp32 operands);
 *   1  every fp32 operand cut exactly into three bf16 pieces, six v_mfma_f32_32x32x16_bf16 per k-block, fp32 accumulate
 *      (same fp32-level accuracy, see csrc/conv_x3.hip);
 *   2  every fp32 operand scaled by a per-tensor power of two and cut into two fp16 pieces (22 significant bits), three
 *      v_mfma_f32_32x32x16_f16 per k-block, fp32 accumulate: each product is good to 2^-22 instead of 2^-24, which stays
 *      inside the fp32 dot-product error bound for every contraction length >= 4 (csrc/conv_igemm.hip, H2).
 * algo < 0 only queries.  Process-wide DEFAULT for the entry points without a scheme argument; returns the value in force
 * before the call.  Initial value: env ELD_FP32_CONV. */
int eld_conv_fp32_algo(int algo);

/* mean |out-target| (nn.L1Loss, models/losses.py:32) and, if dout != NULL, its gradient times grad_scale.
 * ws: eld_l1_workspace_bytes() bytes.  loss: one device float. */
size_t eld_l1_workspace_bytes(void);
int eld_l1_loss(const float* out, const float* target, float* dout, float* loss, void* ws, size_t n, float grad_scale, void* stream);
/* --loss l2: nn.MSELoss (models/losses.py:34), same contract and workspace as eld_l1_loss. */
int eld_mse_loss(const float* out, const float* target, float* dout, float* loss, void* ws, size_t n, float grad_scale, void* stream);
/* torch.optim.Adam step over a flat buffer (models/ELD_model.py:400-401,475); step counts from 1;
 * the gradient is multiplied by grad_scale first (1/world_size after a sum all-reduce). */
int eld_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step, double grad_scale, void* stream);

/* ---- evaluation side -------------------------------------------------------------------------
 * util/index.py:76-81 quality_assess on the images of tensor2im (models/ELD_model.py:23-38: clip(x*255, 0, 255)):
 * est/ref are NCHW float32 in [0,1] units; out[2n] = PSNR (dB), out[2n+1] = SSIM of image n, as device doubles.
 * SSIM = skimage.metrics.structural_similarity(data_range=255, multichannel=True) with its defaults (7x7 uniform window,
 * K1=0.01, K2=0.03, sample covariance, windows inside the image, mean over channels); scikit-image is a third-party
 * dependency the reference does not pin. */
size_t eld_quality_assess_workspace_bytes(int N, int C, int H, int W);
int eld_quality_assess(const float* est, const float* ref, double* out, void* ws, size_t ws_bytes, int N, int C, int H, int W,
                       float data_range, void* stream);
/* the same for images already on the [0, data_range] scale (util/index.py:76-81 called on tensor2im outputs): no x255 stage */
int eld_quality_assess_images(const float* est, const float* ref, double* out, void* ws, size_t ws_bytes, int N, int C, int H, int W,
                              float data_range, void* stream);
/* models/ELD_model.py:138-169 IlluminanceCorrect: out[n] = <p,s>/<p,p> * p, p = clamp(predict[n], 0, 1), sums over the
 * elements with source != 1; source_N is N or 1 (one source for all).  chw = elements per image. */
size_t eld_illuminance_correct_workspace_bytes(int N);
int eld_illuminance_correct(const float* predict, const float* source, float* out, void* ws, size_t ws_bytes, int N, int source_N,
                            size_t chw, void* stream);

/* util/process.py:52-68 `process`: bayer (N,4,H,W) RGBG in [0,1] -> out (N,3,H,W) sRGB, quantised to
 * k/255.  wbs (N,4), ccms (N,3,3) row-major, all device float32.  crf_n = 0: gamma compression with 1/gamma; crf_n >= 2:
 * camera response by piecewise-linear interpolation of (crf_E, crf_f), ascending crf_E (torchinterp1d's rule). */
int eld_isp_process(const float* bayer, const float* wbs, const float* ccms, float* out, int N, int H, int W, float gamma,
                    const float* crf_E, const float* crf_f, int crf_n, void* stream);
/* The same pipeline on X-Trans: packed (N,9,H,W) in RawPacker.pack_raw_xtrans's planes (one packed pixel = one 3x3 mosaic block) ->
 * out (N,3,H,W), k/255.  wbs (N,3) R, G, B gains, applied by plane colour (R: planes 0, 3; G: 1, 5, 6, 7, 8; B: 2, 4 -- xtrans.h
 * XT_COLOUR), clamp, then per colour the mean of its planes summed in ascending plane order in float32 and divided by 2 / 5 / 2:
 * R = (p0 + p3) / 2, G = ((((p1 + p5) + p6) + p7) + p8) / 5, B = (p2 + p4) / 2; then the CCM, clamp and gamma / CRF quantiser
 * of eld_isp_process.  This is the reference's `process` applied to X-Trans binning, not LibRaw's demosaic. */
int eld_isp_process_xtrans(const float* packed, const float* wbs, const float* ccms, float* out, int N, int H, int W, float gamma,
                           const float* crf_E, const float* crf_f, int crf_n, void* stream);

/* ---- full-resolution renders (csrc/demosaic.hip) ------------------------------------------------------------------
 * The packed network output -> planar RGB (N,3,Hm,Wm) at MOSAIC resolution.  Bayer: packed (N,4,h,w), Hm = 2h, Wm = 2w, raw_pattern
 * (HOST, 4 ints, a permutation of 0..3 with the greens on a diagonal) as eld_unpack_raw_bayer_u16 takes it, wbs (N,4) by plane.
 * X-Trans: packed (N,9,h,w), h and w even (whole 6x6 cells, as the write-back), Hm = 3h, Wm = 3w, wbs (N,3) R, G, B by plane colour.
 * ccms (N,3,3) row-major or NULL.  out_mode:
 *     ELD_RENDER_SRGB8        uint8 codes k of the quantiser of eld_isp_process (which writes k / 255); ccms NULL = the identity;
 *     ELD_RENDER_LINEAR_F32   float32 after the CCM (after the demosaic when ccms is NULL): no second clamp, no gamma, no quantiser.
 * Per mosaic site, float32, one rounding per operation:
 *   1. v = min(max(p * gain, 0), 1), as eld_isp_process / eld_isp_process_xtrans.
 *   2. demosaic -> camera RGB at every site; the colour sampled at a site passes through unchanged.
 *      Bayer, Malvar-He-Cutler (2004), coefficients in eighths; borders mirrored without repeating the edge (index -1 -> 1, -2 -> 2,
 *      H -> H - 2), which preserves CFA parity; with c the site's own value and N, S, W, E / NN, SS, WW, EE / NW, NE, SW, SE its neighbours
 *      at distance 1 / 2 / diagonal:
 *          S1 = (N+S)+(W+E)    S2 = (NN+SS)+(WW+EE)    D = (NW+NE)+(SW+SE)
 *          G at R/B site            : ((4c + 2*S1) - S2) * 0.125
 *          R at G site, R left/right: (((5c + 4*(W+E)) + 0.5*(NN+SS)) - (D + (WW+EE))) * 0.125     (B likewise; up/down case transposed)
 *          R at B site, B at R site : ((6c + 2*D) - 1.5*S2) * 0.125
 *      X-Trans, normalised convolution on colour differences, windows clipped to the image; sums start at 0 and add w * value tap by
 *      tap in raster order (dy outer, dx inner), the weight sums are exact integers, the division is correctly rounded:
 *          stage 1  G^ = v at G sites, else (sum w*v over the G sites of the clipped 3x3) / (sum w),  w = [1 2 1] x [1 2 1]
 *          stage 2  for c in {R, B}, at sites not of colour c:
 *                   c^ = G^ + (sum w*(v - G^) over the c sites of the clipped 5x5) / (sum w),         w = [1 2 3 2 1] x [1 2 3 2 1]
 *   3. out[c] = ((r*m[c][0]) + g*m[c][1]) + b*m[c][2]; ELD_RENDER_SRGB8 then clamps to [0,1], applies the gamma table / pow / CRF and
 *      quantises exactly as eld_isp_process does (the same device function).
 * ELD_EINVAL before any launch: a null packed / wbs / out / raw_pattern, packed or out not 16-byte aligned, wbs / ccms / crf_E / crf_f
 * not 4-byte aligned, N < 1 or N > 65535, h < 2 or w < 2 (mosaic sides below 4), an odd X-Trans h or w, a raw_pattern that is not such a
 * permutation, an unknown out_mode, gamma <= 0, crf_n < 0 or crf_n == 1, crf_n >= 2 without crf_E / crf_f. */
#define ELD_RENDER_SRGB8       0
#define ELD_RENDER_LINEAR_F32  1
int eld_render_bayer(const float* packed, const int* raw_pattern, const float* wbs, const float* ccms, void* out, int out_mode,
                     int N, int h, int w, float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream);
int eld_render_xtrans(const float* packed, const float* wbs, const float* ccms, void* out, int out_mode,
                      int N, int h, int w, float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream);
/* Test hook (HOST, no device work): the per-phase tables the X-Trans render is compiled with, 36 rows (phase = 6 * row + col of the cell)
 * of 8 ints: colour (R 0, G 1, B 2), packed plane, then for G (3x3 window) and for R and B (5x5 window) the bit mask of the window taps that
 * hold the colour (bit = raster index of the tap) and the sum of their weights.  n = ints available in out (>= 288). */
int eld_debug_xtrans_demosaic_tables(int* out, int n);

/* ---- defective-pixel maps (csrc/defect.hip, eld_amd/defects.py) ----------------------------------------------------
 * All integer, so every result is defined bit for bit:
 *   class of site (y, x) = pattern[(y % period) * period + x % period] (HOST array of period^2 ints).  period 2: a permutation of 0..3, as
 *       eld_pack_raw_bayer_u16's raw_pattern (the two greens are classes of their own); period 6: rawpy's X-Trans colour codes (0 R, 2 B,
 *       1 and 3 both G) of the 6x6 cell this library packs (xtrans.h: row 0 = R B G B R G) -- any other cell is ELD_EINVAL, because the
 *       tap lists and the window radius are compiled for that cell.
 *   N(y, x) = the sites other than (y, x) inside the image with |dy| <= R, |dx| <= R and the class of (y, x).  Bayer: R = 2 (the 8 sites at
 *       offsets of +-2; 3 in a corner).  X-Trans: R = the smallest radius that leaves every site of every phase at least 3 neighbours in
 *       every image-clipped window of a mosaic with sides >= 6, derived at compile time (eld_debug_xtrans_defect_tables reports it).
 *   lower median of m >= 1 integers = the element of rank (m - 1) / 2 in ascending order.
 * Deviation: stack [F,Hm,Wm] uint16, 1 <= F <= 4096; S = sum over f (exact in uint32); D[y][x] = int32(S - lower median of S over N).
 *   Two passes: S goes through the workspace (eld_defect_deviation_workspace_bytes(Hm, Wm) = 4 Hm Wm bytes, 8-byte aligned).
 *   ELD_EINVAL: a null pointer, F outside [1, 4096], period not 2 or 6, a bad pattern, Hm or Wm < 1 (X-Trans: < 6), an odd Wm (the stack
 *   is read as 32-bit words), Hm * Wm >= 2^31, stack or D not 4-byte aligned; ELD_EWS: the workspace is too small.
 * Flags: site is hot when D > T_hi, cold when -D > T_lo; bitmap[y][x >> 5] bit x & 31, ceil(Wm / 32) uint32 words per row, every word
 *   written, unused bits zero.
 * Repair: out[n][y][x] = in[n][y][x] where the bit is clear, else the lower median of in[n] over the UNFLAGGED sites of N(y, x); a flagged
 *   site with no unflagged neighbour keeps its code.  One bitmap serves the N frames.  in == out is allowed and gives the same bits as
 *   out of place (only unflagged sites are read, and they are written back unchanged); any other overlap is ELD_EINVAL.  Per row, 16-byte
 *   loads and stores when both row pointers are 16-byte aligned, 4-byte ones when 4-byte aligned, 2-byte ones otherwise. */
size_t eld_defect_deviation_workspace_bytes(int Hm, int Wm);
int eld_defect_deviation(const uint16_t* stack, int F, int Hm, int Wm, int period, const int* pattern, int32_t* D, void* ws, size_t ws_bytes,
                         void* stream);
int eld_defect_flags(const int32_t* D, int Hm, int Wm, int32_t T_hi, int32_t T_lo, uint32_t* bitmap, void* stream);
int eld_defect_repair_u16(const uint16_t* in, uint16_t* out, int N, int Hm, int Wm, int period, const int* pattern, const uint32_t* bitmap,
                          void* stream);
/* Test hook (HOST, no device work): out[0] = the X-Trans window radius R, then 36 rows (phase = 6 * row + col of the cell) of 4 ints: colour
 * (R 0, G 1, B 2), number of same-colour taps in the (2R + 1)^2 window, and the low / high 32 bits of their mask (bit = raster index
 * (dy + R) * (2R + 1) + dx + R; the centre is never set).  n = ints available in out (>= 145). */
int eld_debug_xtrans_defect_tables(int* out, int n);

/* ---- exact histograms (csrc/hist.hip, eld_amd/validate.py) --------------------------------------------------------------
 * counts[.][G][B], B = 2R + 1, uint64, fully written by the call (zeros included); integer adds only, so the result is defined bit for bit
 * (it equals np.bincount).  1 <= G <= 4, 1 <= R <= 32767 (every R works: a table too large for the LDS is counted in global memory).  No
 * workspace.  bin = clamp(d + R, 0, 2R): the end bins absorb the overflow.
 *
 * eld_hist_u16: u [F,Hm,Wm] uint16 codes, F <= 65535, Wm even, Hm * Wm < 2^31; p = the pattern period (2 or 6); group: HOST array of p*p ints
 *   in [-1, G), cell (y % p, x % p) -> histogram group, -1 = not counted; d = int(u) - centre[g] (centre: HOST int32[G], |centre| <= 2^30), or
 *   int(u) - int(v) when v (optional, same shape) is given (centre is then ignored and may be NULL); bitmap (optional): the defect bitmap of
 *   eld_defect_flags, ceil(Wm / 32) uint32 words per row, one map for all F frames -- a flagged site is not counted.  counts[F][G][B].
 *   u, v and bitmap 4-byte aligned, counts 8-byte aligned.  16-byte loads when Wm % 8 == 0 and u (and v) are 16-byte aligned.
 * eld_hist_f32: x [N,C,H,W] float32, N <= 65535, C <= 64, H * W < 2^31; group: HOST array of C ints in [-1, G), plane c -> group; scale: DEVICE
 *   float32[N]; q(t) = (int)clamp(rintf(t * scale[n]), -2^29, 2^29) -- one float32 multiply, round half to even; d = q(x), or q(x) - q(x2)
 *   when x2 (optional, same shape) is given.  +-inf and values beyond the clamp land in the end bins; an element whose product x * scale[n]
 *   (or x2 * scale[n]) is NaN -- every NaN x -- is not counted.  counts[N][G][B].
 * ELD_EINVAL before any launch for everything the host can see: sizes, p, G, R, a group entry outside [-1, G), null or misaligned pointers. */
int eld_hist_u16(const uint16_t* u, const uint16_t* v, int F, int Hm, int Wm, int p, const int* group, int G, const int32_t* centre, int R,
                 const uint32_t* bitmap, uint64_t* counts, void* stream);
int eld_hist_f32(const float* x, const float* x2, int N, int C, int H, int W, const int* group, int G, const float* scale, int R,
                 uint64_t* counts, void* stream);

/* ---- exact sums for the spatial structure of noise (csrc/structure.hip, eld_amd/structure.py) ----------------------------
 * u [F,Hm,Wm] uint16 codes, F <= 65535, Wm even, Hm * Wm < 2^31; p = the pattern period (2 or 6); centre: HOST int32[p*p], one value in
 * [0, 65535] per cell (y % p, x % p); d = int(u) - centre[cell], so |d| <= 65535.  bitmap (optional): the defect bitmap of eld_defect_flags,
 * ceil(Wm / 32) uint32 words per row, one map for all frames -- a flagged site contributes nothing anywhere.  Every output is int64 and
 * fully written by the call (zeroed first); integer adds only, so the result is defined bit for bit.  sum d^2 <= 65535^2 Hm Wm
 * < 2^32 * 2^31 = 2^63 fits int64, and so does every other sum.  No workspace.
 *
 * eld_struct_sums_u16: row[F][Hm][p][2] = (n, sum d) over the unflagged columns x of row y with x % p == c; col[F][Wm][p][2] = (n, sum d)
 *   over the unflagged rows y of column x with y % p == r; cell[F][p*p][3] = (n, sum d, sum d^2) of cell r * p + c.  An entry with n == 0
 *   is (0, 0).
 * eld_struct_cross_u16: pairs: HOST int32[Q][2], frame indices (a, b) in [0, F), Q <= 2^24; cross[Q][p*p] = sum d_a d_b over the unflagged
 *   sites of the cell.  (a, a) gives that frame's sum d^2.  For two independent frames of one sensor cov(d_a, d_b) per site is the variance
 *   of what does not change between frames: the fixed pattern.
 * u and bitmap 4-byte aligned, outputs 8-byte aligned.  16-byte loads when Wm % 8 == 0 and u is 16-byte aligned, 32-bit words otherwise.
 * ELD_EINVAL before any launch for everything the host can see: p, sizes, an odd Wm, a centre outside [0, 65535], a pair outside [0, F),
 * null or misaligned pointers (an output without elements may be NULL).  F == 0 (Q == 0) or an empty frame: 0 after zeroing the outputs. */
int eld_struct_sums_u16(const uint16_t* u, int F, int Hm, int Wm, int p, const int32_t* centre, const uint32_t* bitmap, int64_t* row,
                        int64_t* col, int64_t* cell, void* stream);
int eld_struct_cross_u16(const uint16_t* u, int F, int Hm, int Wm, int p, const int32_t* centre, const uint32_t* bitmap, const int32_t* pairs,
                         int Q, int64_t* cross, void* stream);

/* ---- dark shading: per-site offset maps over ISO (csrc/shading.hip, eld_amd/shading.py) ---------------------------------
 * The mean of a sensor's dark frames is, per site, close to linear in ISO: offset(y, x, iso) = a(y, x) + b(y, x) * t, t = iso - x0.  The fit
 * pools the bias frames of all sessions; the other three entries subtract the map.  Every output depends on its own site only: no atomics,
 * no cross-lane sums, and every floating-point operation below is rounded once, in the order written, without FMA contraction -- two calls
 * give the same bits, and the results are defined bit for bit (tests/shading_ref.py restates them in NumPy).
 * Common rules: Wm even, Hm * Wm < 2^31; bitmap (optional) = the defect bitmap of eld_defect_flags, ceil(Wm / 32) uint32 words per row;
 * code, pool, map and bitmap pointers 4-byte aligned.  ELD_EINVAL before any launch for what the host can see: null pointers, an odd Wm, a
 * period other than 2 or 6, a misaligned pointer, S < 1, S > 16, a session with count < 1, count > 65536 or a range outside [0, F), a centre
 * outside [0, 65535].  A zero-sized problem returns 0.
 *
 * eld_shading_fit_u16: pool, pool_elems, frames, F = a frame pool's buffer and DEVICE table, as eld_crop_pack_raw_*_u16; all frames Hm x Wm.
 *   sessions: HOST int32[S][2], (first, count) ranges of the table; alpha, beta: HOST float64[S], the regression weights of the session means
 *   (eld_amd.shading.fit_coefficients); centre: HOST int32[period^2], the nominal black level of cell (y % period, x % period).  Per site,
 *   for s = 0 .. S-1 in order:
 *       T_s = sum over the session's frames of int(u)                               exact (uint32: 65536 * 65535 < 2^32)
 *       y_s = (double(T_s) - double(count_s) * double(centre)) / double(count_s)    product and difference exact: one rounding
 *       A = A + alpha_s * y_s;  B = B + beta_s * y_s                                float64 from +0.0
 *   out_a = float(A), out_b = float(B) (float32 [Hm,Wm]); a site flagged in the bitmap writes +0.0 to both.  A table entry that is not an
 *   Hm x Wm frame at an even offset inside the pool contributes no codes (nothing outside the pool is read; the host wrapper checks its
 *   table before the call).  One pass: 2 bytes read per site and frame, 8 written per site.  A lane owns 8 consecutive columns: 16-byte
 *   loads where Wm % 8 == 0, the pool is 16-byte aligned and the frame's offset is a multiple of 8 elements; 32-bit words otherwise.
 * eld_shading_apply_u16: in, out uint16 [N,Hm,Wm] (out == in is allowed), a, b float32 [Hm,Wm], one map for all frames:
 *       ds = a + b * t;  r = rintf(ds) (ties to even);  out = clamp(int(u) - int(r), 0, 65535)
 *   float32; r is limited to [-65536, 65536] before the conversion, which changes no result.  A flagged site passes through unchanged.
 *   |ds - r| <= 0.5 DN stays in the frame as a fixed remainder (variance 1/12 for a spread-out ds).  16-byte accesses when Wm % 8 == 0 and
 *   all four pointers are 16-byte aligned, 32-bit words otherwise.
 * eld_pack_raw_bayer_u16_shaded / eld_pack_raw_xtrans_u16_shaded: eld_pack_raw_*_u16_gain with the map of the mosaic site (row, col) an element
 *   packs from subtracted in float32 before the division -- nothing is rounded to codes:
 *       ds = a[row][col] + b[row][col] * t;  v = ((float(u) - black_k) - ds) / denom_k;  out = min(max(min(max(v, 0), 1) * ratios[n], 0), 1)
 *   a, b: float32 [2h,2w] (Bayer) / [Hm,Wm] (X-Trans), one map for all N frames.  With a = b = +0.0 the result is eld_pack_raw_*_u16_gain's,
 *   bit for bit.  Bayer reads the map 16 bytes at a time when w is even and a, b are 16-byte aligned. */
int eld_shading_fit_u16(const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int Hm, int Wm, const int32_t* sessions,
                        int S, const double* alpha, const double* beta, const int32_t* centre, int period, const uint32_t* bitmap,
                        float* out_a, float* out_b, void* stream);
int eld_shading_apply_u16(const uint16_t* in, uint16_t* out, int N, int Hm, int Wm, const float* a, const float* b, float t,
                          const uint32_t* bitmap, void* stream);
int eld_pack_raw_bayer_u16_shaded(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern, const float* black_level,
                                  float white_point, const float* ratios, const float* a, const float* b, float t, void* stream);
int eld_pack_raw_xtrans_u16_shaded(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point,
                                   const float* ratios, const float* a, const float* b, float t, void* stream);

/* ---- error versus signal level of an estimate against a reference (csrc/pairstats.hip, eld_amd/evaluate.py) ---------------
 * est, ref [F,Hm,Wm] uint16 codes (any width, odd ones included), F <= 65535, Hm * Wm < 2^31; p = the pattern period (2 or 6); group: HOST
 * array of p*p ints in [-1, G), cell (y % p, x % p) -> colour group, -1 = not counted, 1 <= G <= 4; black: HOST int32[p*p] in [0, 65535], the
 * black level of each cell; white in [1, 65536]; bitmap (optional): the defect bitmap of eld_defect_flags, ceil(Wm / 32) uint32 words per row,
 * one map for all frames.  A site (y, x) counts when y < Hc, x < Wc (0 <= Hc <= Hm, 0 <= Wc <= Wm: X-Trans passes the whole 6x6 cells, whose
 * borders the write-back leaves untouched), its bit is clear and its group is not -1.  With c = (y % p) * p + x % p, g = group[c]:
 *     s = int(ref) - black[c]        e = int(est) - int(ref)
 *     bin = NB - 1                                     when ref >= white   (the saturated bin)
 *           0                                          when s <= 0
 *           s                                          when s < 8
 *           8 + 4 * (o - 3) + ((s >> (o - 2)) & 3)     otherwise, o = floor(log2 s): quarter octaves
 *   NB = ELD_PAIRSTATS_BINS = 61 (s <= 65535 ends in bin 59).  out[f][g][bin][0..3] += (1, s, e, e^2): int64, fully written by the call
 *   (zeroed first).  e^2 < 2^32 and fewer than 2^31 sites: every sum fits.  Integer adds only, so the result is defined bit for bit whatever
 *   the launch geometry (tests/pairstats_ref.py restates it in NumPy).
 * One pass, 4 bytes read per site: 16-byte loads when est and ref are 16-byte aligned (any width: a frame is read as a flat array, the few
 * sites around its aligned body one by one), 2-byte loads otherwise.  est and ref 2-byte aligned, bitmap 4-byte, out 8-byte.
 * Workspace: eld_pair_level_stats_workspace_bytes(F, Hm, Wm) bytes (0 in this implementation: ws may then be NULL); ELD_EWS when ws_bytes
 * is smaller.  ELD_EINVAL before any launch for everything the host can see: p, G, sizes, Hc > Hm, Wc > Wm, a group outside [-1, G), a black
 * level outside [0, 65535], white outside [1, 65536], null or misaligned pointers.  F == 0: 0; an empty frame or crop: 0 after zeroing out. */
#define ELD_PAIRSTATS_BINS 61
size_t eld_pair_level_stats_workspace_bytes(int F, int Hm, int Wm);
int eld_pair_level_stats_u16(const uint16_t* est, const uint16_t* ref, int F, int Hm, int Wm, int Hc, int Wc, int p, const int* group, int G,
                             const int32_t* black, int white, const uint32_t* bitmap, int64_t* out, void* ws, size_t ws_bytes, void* stream);

/* ---- noise level from a single frame: per-tile difference sums (csrc/noiselevel.hip, eld_amd/noiselevel.py) ---------------
 * frames [F,Hm,Wm] uint16 codes (any width, odd ones included), F <= 65535, Hm * Wm < 2^31; Hc, Wc, p, group, G, black, white and bitmap as
 * eld_pair_level_stats_u16 (group and black: HOST arrays of p*p values per cell (y % p, x % p), group -1 = not counted, 1 <= G <= 4).
 * stride = s, the distance to the same-colour neighbours: 1 <= s <= p and p % s == 0 (Bayer: p = 2, s = 2; the X-Trans greens have period
 * 3: p = 6, s = 3 with every other cell in group -1; p = 6, s = 6 serves all colours).
 *   Per site (y, x) with s <= y < Hc - s and s <= x < Wc - s, let v[a][b] = the code at (y + (a - 1) s, x + (b - 1) s), a, b in 0..2.  The
 *   site is ELIGIBLE iff g = group[cell(y, x)] >= 0, all nine sites have group g, none of the nine is flagged in bitmap and all nine codes
 *   are > 0 and < white.  Then
 *       r  = v00 - 2 v01 + v02 - 2 v10 + 4 v11 - 2 v12 + v20 - 2 v21 + v22     (E r^2 = 36 sigma^2 for white noise of variance sigma^2)
 *       dx = v12 - v10,  dy = v21 - v01                                         (E (dx^2 + dy^2) = 4 sigma^2)
 *       S9 = the sum over the nine of (v - black[cell of that site])
 *   Tile (ty, tx) owns the sites with (y - s) / (16 s) == ty and (x - s) / (16 s) == tx; nty = Hc > 2 s ? ceil((Hc - 2 s) / (16 s)) : 0 and
 *   ntx the same from Wc.  out[F][nty][ntx][G][4] int64, every entry written by the call:  out[f][ty][tx][g] += (1, S9, r^2, dx^2 + dy^2)
 *   for every eligible site.  |r| <= 8 * 65535 < 2^20, so r^2 < 2^38; dx^2 + dy^2 < 2^33; |S9| < 2^20; a tile holds (16 s)^2 <= 9216 < 2^14
 *   sites: every sum stays below 2^52 in magnitude.  Integer adds only, so the result is defined bit for bit whatever the launch geometry
 *   (tests/noiselevel_ref.py restates it in NumPy).
 * One pass; a tile and its halo of s are read once, 16 bytes at a time when frames is 16-byte aligned (any width), 2-byte loads otherwise.
 * frames 2-byte aligned, bitmap 4-byte, out 8-byte.  Workspace: eld_tile_noise_workspace_bytes(F, Hm, Wm) bytes (0 in this implementation:
 * ws may then be NULL); ELD_EWS when ws_bytes is smaller.  ELD_EINVAL before any launch for everything the host can see: p, stride, G, sizes,
 * Hc > Hm, Wc > Wm, a group outside [-1, G), a black level outside [0, 65535], white outside [1, 65536], null or misaligned pointers.
 * F == 0 or an empty tile grid (nty * ntx == 0): 0, nothing is read or written. */
size_t eld_tile_noise_workspace_bytes(int F, int Hm, int Wm);
int eld_tile_noise_sums_u16(const uint16_t* frames, int F, int Hm, int Wm, int Hc, int Wc, int p, int stride, const int* group, int G,
                            const int32_t* black, int white, const uint32_t* bitmap, int64_t* out, void* ws, size_t ws_bytes, void* stream);

/* ---- a burst of a static scene: robust mean and photon-transfer sums (csrc/burst.hip, eld_amd/burst.py) --------------------
 * frames [N,Hm,Wm] uint16 codes of one scene shot N times from a tripod, 2 <= N <= 256, Hm * Wm < 2^31, any width; p, group, G, black, white
 * and bitmap as eld_pair_level_stats_u16 (group and black: HOST arrays of p*p values per cell (y % p, x % p)).  All arithmetic is integer.
 * Per site, with samples x_0 .. x_{N-1}:  S1 = sum x (< 2^24),  S2 = sum x^2 (< 2^40).
 *   Leave-one-out rejection, active when N >= 4 and k2q > 0: d = N x - S1 ((N - 1) times the deviation of x from the mean of the others),
 *   V1 = (N - 1)(S2 - x^2) - (S1 - x)^2 ((N - 1)^2 times the others' population variance); x is rejected iff
 *       |d| > (N - 1) min_dev   and   4 d^2 (N - 2) > k2q (N - 1) V1
 *   that is, iff x lies further than k sample deviations of the other N - 1 samples from their mean, k2q = round(4 k^2), and further than
 *   min_dev DN.  0 <= k2q <= 256, 0 <= min_dev <= 65535: both sides then fit unsigned 64 bits (d^2 < 2^48, V1 < 2^46).
 *   With n kept samples of sum S:  mean = (2 S + n) / (2 n) (rounds half up; n == 0, possible for k2q <= 5 only, gives 0);  kept = n as uint8,
 *   256 written as 0 (kept may be NULL).  A site flagged in bitmap still gets mean and kept: repair is eld_defect_repair_u16's.
 *   ptc (may be NULL) [G][ELD_PAIRSTATS_BINS][4] int64, fully written (zeroed first): over the ELIGIBLE sites -- group >= 0, not flagged,
 *   n == N, max x < white, min x > 0 -- ptc[g][bin] += (1, S1, V mod 2^32, V >> 32) with V = N S2 - S1^2 (< 2^46) and bin = the bin of
 *   eld_pair_level_stats_u16 for ref = mean, s = mean - black[cell].  The host recombines sum V = ptc[..][2] + 2^32 ptc[..][3].  Integer adds
 *   only: the result is defined bit for bit whatever the launch geometry (tests/burst_ref.py restates it in NumPy).
 * One pass, 2 N bytes read per site; 16-byte loads when frames and mean are 16-byte aligned, kept 8-byte aligned and Wm % 8 == 0, 32-bit
 * words when frames and mean are 4-byte aligned, kept 2-byte aligned and Wm is even, 2-byte loads otherwise.  frames and mean 2-byte
 * aligned, bitmap 4-byte, ptc 8-byte.  Workspace: eld_burst_stack_workspace_bytes(N, Hm, Wm) bytes (0 in this implementation: ws may then be
 * NULL); ELD_EWS when ws_bytes is smaller.  ELD_EINVAL before any launch for everything the host can see: p, G, sizes, N outside [2, 256],
 * k2q outside [0, 256], min_dev outside [0, 65535], a group outside [-1, G), a black level outside [0, 65535], white outside [1, 65536],
 * null or misaligned pointers.  An empty frame: 0 after zeroing ptc. */
size_t eld_burst_stack_workspace_bytes(int N, int Hm, int Wm);
int eld_burst_stack_u16(const uint16_t* frames, int N, int Hm, int Wm, int p, const int* group, int G, const int32_t* black, int white,
                        const uint32_t* bitmap, int k2q, int min_dev, uint16_t* mean, uint8_t* kept, int64_t* ptc, void* ws, size_t ws_bytes,
                        void* stream);

/* ---- aligning a hand-held burst: tile motion search, then the stack through the field (csrc/align.hip, eld_amd/burst.py) ------
 * frames [N,Hm,Wm] uint16, 2 <= N <= 256, Hm * Wm < 2^31; p the CFA period (2 or 6); frame `ref` is the reference.  All arithmetic is integer;
 * tests/align_ref.py restates every line below in NumPy.  T = 16 (tile side), R = 4 (search radius per level).
 *   luma      Hl = Hm / p, Wl = Wm / p (floor; rows and columns beyond p Hl, p Wl do not enter);
 *             L0[i][Y][X] = (sum of the p p codes of cell (Y, X) of frame i + p p / 2) / (p p), uint16.  Black levels are not subtracted.
 *   pyramid   level l + 1 has sides (h + 1) / 2, (w + 1) / 2 and L[l+1][Y][X] = (a + b + c + d + 2) >> 2 over the 2 x 2 block at (2Y, 2X) of
 *             level l, coordinates clamped to that level's last row and column.  `levels` counts the levels, the finest included: 1..4, and
 *             every level has both sides >= T (so Hl, Wl >= T), else ELD_EINVAL.
 *   tiles     a level with sides (h, w) has TY = ceil(h / T) by TX = ceil(w / T) tiles; tile (ty, tx) has origin y0 = min(ty T, h - T),
 *             x0 = min(tx T, w - T): the last tile of a row or column is a whole tile shifted back.
 *   search    coarsest level first.  The start (sy, sx) is (0, 0) at the coarsest level and otherwise twice the displacement of the parent tile
 *             (min(((y0 + T / 2) >> 1) / T, TY' - 1), the same in x) one level up.  The 81 candidates (sy + v, sx + u), v, u in [-R, R], are
 *             ranked 0..80 by ascending (|v| + |u|, v, u).  cost = sum over the tile's 256 pixels of |L[ref][y][x] - L[i][cl(y + dy)][cl(x + dx)]|
 *             with cl clamping to the level (cost < 2^24).  The winner minimises (cost << 7) | rank (< 2^31): ties fall to the smallest move.
 *   outputs   disp [N][TY0][TX0][2] int16, (dy, dx) at level 0 in luma units (CFA periods), |dy|, |dx| <= 60; cost (may be NULL) [N][TY0][TX0]
 *             uint32, the winner's cost.  Both are zero for frame ref.
 * eld_burst_luma_pyramid_u16 writes the pyramid alone: out holds eld_burst_luma_pyramid_elems(...) uint16 (0: bad arguments), level by level
 * from the finest, each level [N][h][w].  eld_burst_align_u16 runs the pyramid into its workspace and then one search launch per level.
 * Workspace: eld_burst_align_workspace_bytes(...) bytes (0: bad arguments), 4-byte aligned; ELD_EWS when ws_bytes is smaller.  frames, out and disp
 * 2-byte aligned, cost 4-byte. */
size_t eld_burst_luma_pyramid_elems(int N, int Hm, int Wm, int p, int levels);
int eld_burst_luma_pyramid_u16(const uint16_t* frames, int N, int Hm, int Wm, int p, int levels, uint16_t* out, void* stream);
size_t eld_burst_align_workspace_bytes(int N, int Hm, int Wm, int p, int levels);
int eld_burst_align_u16(const uint16_t* frames, int N, int Hm, int Wm, int p, int ref, int levels, int16_t* disp, uint32_t* cost, void* ws,
                        size_t ws_bytes, void* stream);

/* eld_burst_stack_u16 over the samples a displacement field points at.  disp [N][TY0][TX0][2] int16 as eld_burst_align_u16 writes it, TY0 =
 * ceil((Hm / p) / T), TX0 = ceil((Wm / p) / T) (anything else: ELD_EINVAL; Hm / p, Wm / p >= T).  Site (y, x) belongs to tile
 * (min((y / p) / T, TY0 - 1), min((x / p) / T, TX0 - 1)); its sample from frame i is frames[i][y + p dy][x + p dx], PRESENT iff that lies inside
 * the frame.  Displacements are whole CFA periods: every sample is a raw code of the site's own colour, nothing is resampled.  With M present
 * samples the rule, mean and kept of eld_burst_stack_u16 apply as written with N replaced by M (rejection needs M >= 4; M = 0 writes mean 0,
 * kept 0).  present (may be NULL) [Hm][Wm] uint8 = M (256 as 0).  ptc: the eligible sites are those of eld_burst_stack_u16 with M == N besides.
 * With an all-zero field mean, kept and ptc equal eld_burst_stack_u16's bit for bit.  A displacement outside [-60, 60] is ELD_EINVAL: the call
 * checks the field on the device and waits for that one flag before the stack is launched (it synchronises the stream once).
 * 32-bit loads when frames and mean are 4-byte aligned, kept and present 2-byte aligned and Wm is even (a shifted row is only 2 p bytes
 * aligned: there is no 16-byte path), 2-byte loads otherwise.  Workspace: eld_burst_stack_aligned_workspace_bytes bytes, 4-byte aligned. */
size_t eld_burst_stack_aligned_workspace_bytes(int N, int Hm, int Wm);
int eld_burst_stack_aligned_u16(const uint16_t* frames, int N, int Hm, int Wm, int p, const int* group, int G, const int32_t* black, int white,
                                const uint32_t* bitmap, int k2q, int min_dev, const int16_t* disp, int TY0, int TX0, uint16_t* mean, uint8_t* kept,
                                uint8_t* present, int64_t* ptc, void* ws, size_t ws_bytes, void* stream);

/* Dev tool (tools/conv_phase_profile.py; a no-op unless built with -DELD_DEV_TOOLS=1): device buffer of 8 x 4 x 128 x 6 uint64 that conv_x3_kernel fills with s_memtime
 * stamps of its stage phases (first 8 workgroups, first 128 stages); NULL switches it off (default). */
void eld_debug_conv_prof(void* buf);
/* Test hook: route the bf16 launches that normally run on a specialised kernel back to the generic one, so that the parity tests can demand
 * BIT-IDENTICAL results from the two kernel families on the same inputs (same k order, same MFMA): mask bit 0 = conv_bfs_kernel (32-output-channel
 * 3x3 layers) off, bit 1 = conv_bfg_kernel (transposed convolutions) off, bit 2 = conv_bfd_kernel (the other bf16 3x3 layers) off, bit 3 = conv_bfw_kernel off (the 64-output-channel layers with K <= 64 then run on conv_bfd_kernel<64>; conv_bfw sums K in another order, so it equals the others up to fp32 summation order, not bit for bit), bit 4 = wgrad8d_kernel off (the bf16 weight gradient of the 128 x 64 blocks then runs the register-staged wgrad8_kernel<bf16>: other tile shape, so equal up to the fp32 summation order over pixels); bit 5 = eld_quality_assess with one window column per lane instead of two, bit 6 = eld_quality_assess on the round-2 tile kernels (three
 * implementations of the same sums: tests/test_model_gpu.py runs the oracle comparison under each); bit 7 = the U-Net forwards write no slope codes (the backward-data
 * epilogues of levels 0 / 1 then read the saved activations, as before round 5: same slopes, bit-identical gradients); bit 8 = no pool-argmax codes
 * (the backward of the two full-size pools then reads the saved un-pooled tensors: same winners, bit-identical gradients).  Returns the previous mask.  Process-wide; production never calls it. */
int eld_debug_kernel_mask(int mask);
/* Test hook: live entries of the per-workspace host bookkeeping (which forward last filled a workspace: fused head, slope codes); bounded, evicted
 * one least-recently-touched entry at a time. */
int eld_debug_ws_state_entries(void);

/* ---- single layers on NHWC float32 tensors with reference-layout weights; used by the parity tests ---- */
size_t eld_layer_workspace_bytes(int N, int H, int W, int Cin, int Cout);
/* out = [lrelu](conv3x3(cat[in0,in1]) + bias).  nn.Conv2d(k=3,p=1) + torch.max(0.2x,x)  (Unet.py:11-44,102-104) */
int eld_conv3x3_forward(const float* in0, int C0, const float* in1, int C1, const float* w_oihw, const float* bias,
                        float* out, int N, int H, int W, int Cout, int lrelu, void* ws, size_t ws_bytes, void* stream);
/* din = conv3x3_backward_data(g); channels [0,split) -> din0, [split,Cin) -> din1; optionally times the LeakyReLU
 * slope of the saved post-activation tensors act0/act1 (NULL = no activation in front). */
int eld_conv3x3_backward_data(const float* g, const float* w_oihw, float* din0, float* din1, int split, const float* act0,
                              const float* act1, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
/* dw (OIHW), db from g (grad of the pre-activation output) and the layer input cat[x0,x1]. */
int eld_conv3x3_backward_weight(const float* g, const float* x0, int C0, const float* x1, int C1, float* dw, float* db,
                                int N, int H, int W, int Cout, void* ws, size_t ws_bytes, void* stream);
/* nn.ConvTranspose2d(Cin,Cout,2,stride=2) (Unet.py:30,34,38,42): in [N,H,W,Cin] -> out [N,2H,2W,Cout]. */
int eld_convt2x2_forward(const float* in, const float* w, const float* bias, float* out, int N, int H, int W, int Cin, int Cout,
                         void* ws, size_t ws_bytes, void* stream);
int eld_convt2x2_backward_data(const float* dout, const float* w, const float* act, float* din, int N, int H, int W, int Cin,
                               int Cout, void* ws, size_t ws_bytes, void* stream);
int eld_convt2x2_backward_weight(const float* in, const float* dout, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                 void* ws, size_t ws_bytes, void* stream);
/* nn.MaxPool2d(2) (Unet.py:13): in [N,2Ho,2Wo,C] -> out [N,Ho,Wo,C]; backward = (routed dp + skip) * slope(act). */
int eld_maxpool2x2_forward(const float* in, float* out, int N, int Ho, int Wo, int C, void* stream);
int eld_maxpool2x2_backward(const float* act, const float* dp, const float* skip, float* g, int N, int Ho, int Wo, int C, void* stream);

/* ---- the same single layers with bf16 activations (test hooks of the bf16 network) ----
 * Activations and gradients are NHWC bf16 device buffers (uint16_t bit patterns); weights come in the reference fp32 layout, bias is fp32,
 * dw / db are fp32.  Each call packs the weights to bf16 (round to nearest even) in the layout the U-Net's packer would choose for the same
 * launch and runs the dispatcher the bf16 U-Net runs, so the launch lands on the kernel family the network would use for that shape
 * (eld_debug_last_conv_kernel names it).  Workspace: eld_layer_workspace_bytes.  Channel counts: multiples of 32 (weight gradients: C0, C1
 * multiples of 8, C0 of 32 when C1 > 0; transposed convs: Cout a multiple of 8 forward and for the weight gradient). */
int eld_conv3x3_forward_bf16(const uint16_t* in0, int C0, const uint16_t* in1, int C1, const float* w_oihw, const float* bias, uint16_t* out,
                             uint16_t* pool_out, int N, int H, int W, int Cout, int lrelu, void* ws, size_t ws_bytes, void* stream);
/* pool_out (optional): also the 2x2 max-pool of out, fused into the epilogue; ELD_ENOTSUP where the dispatcher would not fuse it (conv_igemm). */
int eld_conv3x3_backward_data_bf16(const uint16_t* g, const float* w_oihw, uint16_t* din0, uint16_t* din1, int split, const uint16_t* act0,
                                   const uint16_t* act1, int N, int H, int W, int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
int eld_conv3x3_backward_weight_bf16(const uint16_t* g, const uint16_t* x0, int C0, const uint16_t* x1, int C1, float* dw, float* db,
                                     int N, int H, int W, int Cout, void* ws, size_t ws_bytes, void* stream);
int eld_convt2x2_forward_bf16(const uint16_t* in, const float* w, const float* bias, uint16_t* out, int N, int H, int W, int Cin, int Cout,
                              void* ws, size_t ws_bytes, void* stream);
int eld_convt2x2_backward_data_bf16(const uint16_t* dout, const float* w, const uint16_t* act, uint16_t* din, int N, int H, int W, int Cin,
                                    int Cout, void* ws, size_t ws_bytes, void* stream);
int eld_convt2x2_backward_weight_bf16(const uint16_t* in, const uint16_t* dout, float* dw, float* db, int N, int H, int W, int Cin, int Cout,
                                      void* ws, size_t ws_bytes, void* stream);
int eld_maxpool2x2_forward_bf16(const uint16_t* in, uint16_t* out, int N, int Ho, int Wo, int C, void* stream);
int eld_maxpool2x2_backward_bf16(const uint16_t* act, const uint16_t* dp, const uint16_t* skip, uint16_t* g, int N, int Ho, int Wo, int C, void* stream);

/* Test hook: the family name of the most recent convolution or weight-gradient launch of this process, recorded by the launcher that chose it
 * (a dispatcher that falls through to another family records nothing itself); host-side only, "" before the first launch.
 *   bf16: "conv_bfs", "conv_bfw", "conv_bfd<128>", "conv_bfd<64>", "conv_bfg<128>", "conv_bfg<64,gather>", "conv_bfg<128,gather>", "conv_igemm<bf16>",
 *         "conv_igemm<bf16,1x1>", "conv_igemm<bf16,gather>", "wgrad8d", "wgrad8<bf16>", "wgrad<bf16>", "wgrad<bf16,gather>";
 *   fp32, three-piece scheme (tile width in output channels, waves per workgroup): "conv_x3w", "conv_x3<32>", "conv_x3d<128,8>", "conv_x3d<64,8>",
 *         "conv_x3d<64,4>", "conv_x3d<64,4,splitk>" (K split over workgroups, inside a U-Net entry point only),
 *         "conv_x3_gemm<1x1>", "conv_x3_gemm<gather>" (transposed convs), "wgrad8<f32,128x64>", "wgrad8<f32,64x64>", "wgrad8<f32,64x32>",
 *         "wgrad8<f32,32x64>", "wgrad8<f32,32x32>" (block = output x input channels), "wgradt8";
 *   fp32, other schemes and shapes: "conv_igemm<f32>", "conv_igemm<f32,h2>", "wgrad<f32>", "wgrad<f32,gather>".
 * A launch of a non-default variant of a family -- one that an ELD_* switch of the process environment selected (DESIGN.md section 6a lists them) --
 * answers "family/suffix[,suffix]" instead: "conv_x3<32>/cut" (ELD_X3W=0: fp32 packed weights cut per stage; also what layers of 96, 160, ... output
 * channels record), "conv_x3d<...>/tiles-f" and "conv_bfd<...>/tiles-f" (-p, -m, -q, -t: ELD_CONV_TILES), "wgrad<bf16,gather>/f32mma" (ELD_WGRAD_BF16_MMA=0); with
 * ELD_FIRST_MMA=0 the first layer of 4 planes records "conv_first/mma0" (it records nothing otherwise).  With no switch set the names are the ones above. */
const char* eld_debug_last_conv_kernel(void);
/* Test hook: how many launches this process has recorded under a family name (0 for a name never seen): what a test of a whole-network entry
 * point compares before and after the call to see which families the dispatcher chose inside it.  The table holds 64 names; once a 65th has
 * been launched, a name outside the table answers ELD_CONV_KERNEL_COUNT_UNKNOWN instead of 0.
 * Added without a change of ELD_ABI_VERSION (no existing signature changed), so the Python binding, which binds every symbol, needs a library
 * built from this header or a later one: an older ABI-8 library fails at bind with this symbol missing, not with the version message. */
#define ELD_CONV_KERNEL_COUNT_UNKNOWN 0xFFFFFFFFu
unsigned eld_debug_conv_kernel_count(const char* family);
/* Test hook: where the U-Net workspace of problem (N, H, W, in_ch, out_ch, precision) holds a region after a forward (eld_unet_forward_ex /
 * eld_unet_forward_bf16) or, for ELD_REGION_GRAD_CONV1_1, after a bf16 backward: *offset in bytes, *channels, *dtype = 0 fp32 NHWC, 1 bf16 NHWC,
 * 2 fp32 NCHW.  level: the U-Net level (pool: the level of the tensor it pools), 0 for X16 and GRAD_CONV1_1.  X16 = the first layer's input as the
 * forward kept it; GRAD_CONV1_1 = the gradient of conv1_1's output that its weight gradient consumed (bf16 only). */
enum { ELD_REGION_EA = 0, ELD_REGION_EB = 1, ELD_REGION_POOL = 2, ELD_REGION_UP = 3, ELD_REGION_DA = 4, ELD_REGION_DB = 5, ELD_REGION_X16 = 6,
       ELD_REGION_GRAD_CONV1_1 = 7 };
int eld_debug_unet_region(int N, int H, int W, int in_ch, int out_ch, int precision, int region, int level, size_t* offset, int* channels,
                          int* dtype);
/* Test hook: a tap on the activation gradients of the U-Net backward (tests/test_backward_layers_gpu.py; DESIGN.md sections 6 / 6a).  Appended
 * without a change of ELD_ABI_VERSION, as eld_debug_conv_kernel_count above.  Process-global; buf == NULL switches it off (the default).  While
 * set, eld_unet_backward_ex (both precisions) enqueues one device-to-device hipMemcpyAsync on the call's own stream right after each stage that
 * writes an activation gradient -- before the gradient buffers swap and the next stage overwrites the other one -- copying that tensor to
 * buf + offset(stage).  No kernel differs; with the tap unset the backward enqueues exactly what it always did (one host branch per stage).
 * The ELD_TAP_NSTAGES = 30 stages, numbered in backward order (l = U-Net level, conv(9-l)_x the decoder layers of level l):
 *   0                 g_head     gradient of conv9_2's pre-activation output, written by the head backward or by the fused training head
 *   1 + 4l, l = 0..3  d_da[l]    conv(9-l)_2 backward-data times slope(da[l]): gradient of conv(9-l)_1's pre-activation output
 *   2 + 4l            d_up[l]    first output of conv(9-l)_1's backward-data (raw: the transposed conv has no activation)
 *   3 + 4l            skip[l]    its second output (raw): the skip connection's share of eb[l]'s gradient
 *   4 + 4l            d_src[l]   transposed-conv backward-data times slope(db[l+1]) (l = 3: slope(eb[4])), at level l + 1
 *   17 + 3(4-l), l = 4..0   d_ea[l]      conv(l+1)_2 backward-data times slope(ea[l]); l = 0 (stage 29) is what conv1_1's weight gradient reads
 *   18 + 3(4-l), l = 4..1   d_pool[l-1]  conv(l+1)_1 backward-data (raw), at level l with the channels of level l - 1
 *   19 + 3(4-l), l = 4..1   d_eb[l-1]    the pool backward's output (route(d_pool) + skip[l-1]) * slope(eb[l-1]), at level l - 1
 * eld_debug_unet_grad_tap_layout is a pure query: *offset in bytes into buf (256-byte aligned), *channels, *level (the tensor is NHWC
 * [N][H >> level][W >> level][channels]) and *dtype = 0 fp32 / 1 bf16 (= precision); ELD_EINVAL for a stage outside [0, 30) or a shape
 * eld_unet_workspace_bytes rejects.  eld_debug_unet_grad_tap_bytes: the size the buffer needs for that problem (0: bad arguments).
 * A backward with the tap set returns, before any launch, ELD_EINVAL when the buffer is smaller than that and ELD_ENOTSUP when the stream is
 * being captured (a graph must not bake the debug copies in). */
#define ELD_TAP_NSTAGES 30
void eld_debug_unet_grad_tap(void* buf, size_t bytes);
int eld_debug_unet_grad_tap_layout(int N, int H, int W, int in_ch, int out_ch, int precision, int stage, size_t* offset, int* channels, int* level,
                                   int* dtype);
size_t eld_debug_unet_grad_tap_bytes(int N, int H, int W, int in_ch, int out_ch, int precision);
/* Test hook: which slope- / pool-code regions the LAST forward on workspace ws filled (what the next backward on it will read instead of the saved
 * activations): an OR of the bits below.  ELD_CODES_EBl = the slope codes of eb[l] AND the argmax codes of pool[l]; ELD_CODES_INFER = the
 * forward was eld_unet_infer_ex (nothing kept for a backward).  -1: the library holds no code state for ws -- no forward ran on it, its last
 * forward filled no region (fp32 scheme other than 1, a problem too small for the 8-wave level-1 kernels, eld_debug_kernel_mask bit 7), or the
 * bounded host table evicted the entry; a backward then reads the saved activations.  Never 0.  Host bookkeeping only. */
enum { ELD_CODES_EA0 = 1, ELD_CODES_EA1 = 2, ELD_CODES_DA0 = 4, ELD_CODES_DA1 = 8, ELD_CODES_EB0 = 16, ELD_CODES_EB1 = 32, ELD_CODES_INFER = 256 };
int eld_debug_unet_codes(const void* ws);

/* ---- flat-field maps: what multiplies the signal, from the flat frames (csrc/flatfield.hip, eld_amd/flatfield.py) -----------
 * Appended without a change of ELD_ABI_VERSION (no existing signature changed), as eld_debug_conv_kernel_count above.  tests/flatfield_ref.py
 * restates every line below in NumPy; the first two passes are integer arithmetic and defined bit for bit whatever the launch geometry.
 *
 * eld_flat_sums_u16: pool, pool_elems, frames as eld_shading_fit_u16 takes them (a frame pool and its EldPoolFrame table); the F table entries
 * are the flat frames, entries 2k and 2k + 1 a pair; F even, 2 <= F <= 65536; Hm * Wm < 2^31, Wm even.  Per site, over the F codes u_f:
 *   S   [Hm,Wm] uint32 = sum of u_f
 *   D   [Hm,Wm] uint64 = sum over the pairs of (u_2k - u_2k+1)^2
 *   bad [Hm,ceil(Wm/32)] uint32, bit x & 31 of word [y][x >> 5] (the layout of the defect bitmap), fully written, pad bits zero: set iff the
 *       site is set in bitmap (may be NULL) or some u_f >= white_level (1..65536; 65536: no code saturates)
 * A table entry that is not an Hm x Wm frame inside the pool contributes zeros; nothing outside the pool is read.  pool, bitmap, S, bad 4-byte
 * aligned, frames and D 8-byte; 16-byte loads and stores where the pool, S and D are 16-byte aligned and Wm % 8 == 0.
 *
 * eld_flat_box_u32: S and bad as written above; period p = 2 or 6; 0 <= radius <= 64.  The window of site (y, x) is the sites
 * (y + p dy, x + p dx), |dy|, |dx| <= radius, that lie inside the frame: its position plane (y % p, x % p), clipped at the border.
 *   Bsum [Hm,Wm] uint64 = sum of S over the window's sites whose bad bit is clear;  Bcnt [Hm,Wm] uint32 = their number
 * Two separable running-sum passes through a workspace of eld_flat_box_workspace_bytes(Hm, Wm) bytes (8 per site; 0: bad shape), 8-byte
 * aligned; ELD_EWS when ws_bytes is smaller.  eld_flat_box_tile reports the mosaic columns a workgroup of the row pass covers and the mosaic
 * rows a workgroup of the column pass covers, for tests that place a shape across both.
 *
 * eld_flat_apply_u16: codes [N,Hm,Wm]; gain [Hm,Wm] float32; black: HOST array of p * p float32 in [0, 65535], one per cell (y % p, x % p).
 * Per site in float32, one rounding per operation, no fused multiply-add:
 *   v = float(u) - black;  w = v * gain;  out = clamp(rint(w + black), 0, 65535)     (rint: ties to even)
 * A site set in bitmap (may be NULL) or with u >= white_level passes through unchanged.  in and out may be the same buffer.
 *
 * eld_pack_raw_bayer_u16_flat / eld_pack_raw_xtrans_u16_flat: eld_pack_raw_*_u16_shaded with a gain plane [Hm,Wm] (Bayer: [2h,2w]):
 *   clip((((float(u) - black) - (a + b t)) * gain) / (white - black), 0, 1), then min(max(. * ratio[n], 0), 1)
 * ma and mb may both be NULL (no subtraction: the operation order of eld_pack_raw_*_u16_gain) and ratios may be NULL (no ratio step: the order
 * of eld_pack_raw_*_u16).  A gain plane of ones gives the bits of those entry points.  ma, mb and gain 4-byte aligned. */
int eld_flat_sums_u16(const uint16_t* pool, size_t pool_elems, const EldPoolFrame* frames, int F, int Hm, int Wm, int white_level,
                      const uint32_t* bitmap, uint32_t* S, uint64_t* D, uint32_t* bad, void* stream);
size_t eld_flat_box_workspace_bytes(int Hm, int Wm);
int eld_flat_box_tile(int period, int* row_pass_columns, int* column_pass_rows);
int eld_flat_box_u32(const uint32_t* S, const uint32_t* bad, int Hm, int Wm, int period, int radius, uint64_t* Bsum, uint32_t* Bcnt, void* ws,
                     size_t ws_bytes, void* stream);
int eld_flat_apply_u16(const uint16_t* in, uint16_t* out, int N, int Hm, int Wm, const float* gain, const float* black, int period,
                       int white_level, const uint32_t* bitmap, void* stream);
int eld_pack_raw_bayer_u16_flat(const uint16_t* mosaic, float* packed, int N, int h, int w, const int* raw_pattern, const float* black_level,
                                float white_point, const float* ratios, const float* ma, const float* mb, float t, const float* gain, void* stream);
int eld_pack_raw_xtrans_u16_flat(const uint16_t* mosaic, float* packed, int N, int Hm, int Wm, float black_level, float white_point,
                                 const float* ratios, const float* ma, const float* mb, float t, const float* gain, void* stream);

/* ---- a classical baseline: non-local means on variance-stabilised codes (csrc/nlm.hip, eld_amd/classical.py) ----------------
 * Appended without a change of ELD_ABI_VERSION (no existing signature changed).  Integer arithmetic from the table lookup on: the result is
 * defined bit for bit whatever the launch geometry, and tests/nlm_ref.py restates every line below in NumPy.
 *
 * eld_nlm_vst_f32: x [N][C][h][w] float32 (device; 4-byte aligned, nothing more), fwd [C][65536] uint16 (device): the forward transform of
 * plane c as a table over the sensor codes; wtab: HOST array of 256 uint16 weights; out [N][C][h][w] int32 (device).
 *   codes     i = clamp(rintf(x * qscale), 0, 65535): one float32 multiply, round half to even, NaN -> 0;  v_c = min(fwd[c][i], 32767)
 *   extension V_c = v_c extended beyond the plane by edge replication
 *   distance  for an offset d = (dy, dx), |dy|, |dx| <= S:
 *               D_d(q) = sum over c, sum over |u|_inf <= P of clamp(V_c(q + u) - V_c(q + u + d), -1023, 1023)^2
 *             a candidate counts only when q + d lies inside the plane (d = 0 always does)
 *   weight    wt = wtab[min(D_d(q) >> sh, 255)]
 *   output    num_c = sum of wt * v_c(q + d), den = sum of wt over the counted offsets;
 *             out_c(q) = (2 * (num_c << frac) + den) / (2 * den), floor division: the weighted mean in units of 2^-frac of a code
 * Ranges: 1 <= N; 1 <= C <= 16; 1 <= h, w; 0 <= S <= 10; 0 <= P <= 3; 0 <= sh <= 24; 0 <= frac <= 8; wtab[k] <= 255; wtab[0] >= 1; no null
 * pointer; fwd 2-byte, x and out 4-byte aligned.  Anything else is ELD_EINVAL before any device work.  They make every width provable:
 * D <= 1023^2 * 16 * 49 < 2^31, num <= 255 * 32767 * 441 < 2^32; only the last shift needs more than 32 bits.
 * The distance is a box sum of the per-position squared difference (row sums, then running column sums): the work per site and offset does not
 * grow with the patch area. */
int eld_nlm_vst_f32(const float* x, int N, int C, int h, int w, float qscale, const uint16_t* fwd, int S, int P, int sh, const uint16_t* wtab,
                    int frac, int32_t* out, void* stream);

/* ---- BM3D on variance-stabilised codes, grouped across the CFA planes (csrc/bm3d.hip, eld_amd/classical.py) -------------------
 * Appended without a change of ELD_ABI_VERSION.  Integers from the table lookup on, and the aggregation is integer addition: the result is
 * defined bit for bit whatever the launch geometry and the order of the adds; tests/bm3d_ref.py restates every line below in NumPy.
 *
 * eld_bm3d_vst_f32: x, fwd, qscale and out as for eld_nlm_vst_f32; guide NULL (step 1: hard threshold) or [N][C][h][w] int32 (device), the output
 * of step 1 in units of 2^-frac (step 2: Wiener); par: HOST, 5 uint32, one per group size 1, 2, 4, 8, 16; win: HOST, 64 uint8, the 8 x 8
 * aggregation window; ws: device workspace of eld_bm3d_vst_workspace_bytes(N, C, h, w) bytes (0 for a shape out of range), 8-byte aligned, any
 * contents.
 *   codes      i = clamp(rintf(x * qscale), 0, 65535), NaN -> 0;  v_c = min(fwd[c][i], 32767)
 *   guide      g_c = v_c without a guide, else clamp((guide + ((1 << frac) >> 1)) >> frac, 0, 32767)
 *   blocks     8 x 8; reference corners y in {0, step, 2 step, ... <= h - 8} and h - 8, likewise x: every site is covered
 *   matching   shared by the planes.  A candidate is an offset d = (dy, dx), |dy|, |dx| <= S, whose whole block lies inside the plane (no
 *              replication).  D_d = sum over c, sum over u in 8 x 8 of clamp(g_c(p + u) - g_c(p + d + u), -1023, 1023)^2; it counts when
 *              D_d <= tau.  Order: the key (D_d << 11) | r with r = 0 for d = 0 and 1 + (dy + S)(2S + 1) + (dx + S) otherwise: unique, and d = 0
 *              is first even where other blocks are exact duplicates (a saturated region), so a reference block is always in its own group
 *              and every site has a denominator.  With n counted the group is the first G = 2^lg, lg = floor(log2(min(n, Gmax))).
 *   sets       mix = 1: one set of all C planes; mix = 0: every plane its own set.  M planes per set, lm = log2 M.
 *   transform  per set, [M][G][8][8] of v at the group's blocks through the unnormalised Walsh-Hadamard transform (Sylvester, natural order)
 *              along all four axes: T.
 *   step 1     T' = T if |T| > par[lg] else 0; nnz kept coefficients in the set; W = 2^20 / max(nnz, 1)
 *   step 2     Tb the same transform of the g blocks, E = Tb^2; R = floor(4096 E / (E + par[lg])); T' = (T R + 2048) >> 12 (arithmetic: floor);
 *              W = 2^44 / max(sum of R^2 over the set, 2^24)
 *   inverse    I the same transform of T'; sh = 6 + lg + lm - frac; est = clamp((I + (1 << (sh - 1))) >> sh, 0, 32767 << frac)
 *   aggregate  for every member block at p', plane c of the set and u: num_c(p' + u) += W win[u] est, den(p' + u) += W win[u], one den per set
 *   output     out_c(q) = (2 num_c + den) / (2 den), floor
 * Ranges: 1 <= N; 1 <= C <= 16; 8 <= h, w; 0 <= S <= 16; 1 <= step <= 8; Gmax in {1, 2, 4, 8, 16}; mix in {0, 1}, 1 only with C a power of two;
 * 0 <= frac <= 4; tau < 2^30; par[k] >= 1 in step 2; 1 <= win[u] <= 16; no null pointer but guide; fwd 2-byte, x, guide and out 4-byte, ws 8-byte
 * aligned.  Anything else is ELD_EINVAL before any device work; then ws_bytes below the size function is ELD_EWS.
 * Widths: D <= 1023^2 * 16 * 64 < 2^30, so a key has 41 bits.  A set holds L = 64 M G <= 2^14 codes: |T|, |Tb| <= 32767 L < 2^29, as is every
 * partial sum on the way.  E < 2^58: the ratio is formed as 4096 - ceil(4096 par / (E + par)), 44 bits over 59, never as the 70-bit E << 12.
 * T R + 2048 < 2^43.  |T'| <= |T|, but I and its partial sums are bounded by sum |T'| only, up to 2^36 for constructed inputs: I is the exact
 * integer (the kernel sums in 32 bits when sum |T'| < 2^31 and in 64 bits otherwise).  W <= 2^20, win <= 16, est < 2^19: a contribution is
 * below 2^43, and at most ((2S + 8) / step + 2)^2 * 16 < 2^15 of them reach a site: num < 2^58, den < 2^39, 64-bit accumulators, and
 * 2 num + den < 2^60.  W >= 2^20 / 2^14 resp. 2^44 / 2^38 = 64 and win >= 1, so den >= 64 at every site. */
size_t eld_bm3d_vst_workspace_bytes(int N, int C, int h, int w);
int eld_bm3d_vst_f32(const float* x, int N, int C, int h, int w, float qscale, const uint16_t* fwd, const int32_t* guide, int S, int step, int Gmax,
                     int mix, uint32_t tau, const uint32_t* par, const uint8_t* win, int frac, int32_t* out, void* ws, size_t ws_bytes, void* stream);

/* ---- DNG raw decode: packed bits and lossless JPEG (csrc/dng.hip, csrc/dng_dev.h, eld_amd/dng.py) ------------------------------
 * Appended without a change of ELD_ABI_VERSION: two new symbols, no existing call changed.  The host (eld_amd/dng.py) parses the TIFF container
 * and every JPEG marker segment; the device sees one contiguous byte range of the file (blob), one record per strip or tile (a stream) and, for
 * lossless JPEG, the canonical Huffman decode tables.  Both entry points write the visible mosaic out[Hm][Wm]: the site (y, x) of the full
 * H x W image goes to out[y - top][x - left] when it lies inside the active area [top, top + Hm) x [left, left + Wm); tile samples beyond
 * the image are dropped; with lin, the value written is lin[min(v, lin_len - 1)].
 *
 * A record the kernel cannot trust is never followed: every read is checked against the stream's byte range (and that against blob_bytes),
 * every write against the tile and the image, every table index against the table.  A stream stops at its first violation and reports it
 * in status[stream] (ELD_DNG_*); streams are independent, the others decode. */
#define ELD_DNG_OK 0
#define ELD_DNG_TRUNCATED 1        /* the data ended before the last sample */
#define ELD_DNG_BADCODE 2          /* bits that are no code of the table, or a symbol above 16 */
#define ELD_DNG_TOOMANY 3          /* the stream holds more samples than its tile */
#define ELD_DNG_BADRECORD 4        /* a field of the record out of range (data beyond the blob, table index, geometry, row buffer) */
#define ELD_DNG_FAST_BITS 9

typedef struct EldDngStream {      /* 64 bytes */
    uint32_t data_off, data_len;   /* the byte range in blob: entropy-coded data (after the SOS header) / the packed rows */
    int32_t x0, y0, tw, th;        /* the tile's origin in the full image, its stored width and length (a last strip: the rows it has) */
    int32_t P, X, Y, Nf, pred;     /* lossless JPEG only: precision 2..16, samples per line, lines, components 1..4, predictor 1..7 */
    uint16_t table[4];             /* lossless JPEG only: the decode table of each component */
    uint32_t ws_off;               /* lossless JPEG, predictors 2..7: where this stream's row of X * Nf samples starts in ws (elements) */
    uint32_t reserved[2];
} EldDngStream;

typedef struct EldDngHuff {        /* 1196 bytes: one canonical Huffman table, symbols 0..16, codes of 1..16 bits */
    uint16_t fast[1 << ELD_DNG_FAST_BITS];  /* indexed by the next 9 bits: (length << 8) | symbol for a code of <= 9 bits, else 0 */
    int32_t maxcode[17];           /* [l]: the largest code of l bits, -1 where there is none */
    int32_t valoff[17];            /* [l]: the code c of l bits has the symbol vals[c + valoff[l]] */
    uint8_t vals[32];              /* the symbols in code order */
    int32_t nvals;
} EldDngHuff;

/* eld_dng_unpack_u16: compression 1.  bits in {8, 10, 12, 14, 16}, samples MSB-first, every row of a stream starts on a byte boundary (a row
 * takes ceil(tw * bits / 8) bytes); 16-bit samples are little-endian unless big_endian.  One lane per four samples.
 * eld_dng_ljpeg_u16: compression 7 (ITU-T T.81 process 14).  One lane per stream; `lanes` streams share a wave (1..64; 0: chosen from nstreams
 * and the device's size).  The decoded samples are laid into the tile linearly (sample i -> row i / tw, column i % tw) while prediction runs
 * in the JPEG's own X x Y x Nf geometry; SSSS = 16 is the difference 32768 without extra bits; sums are modulo 65536.  ws: ws_elems uint16
 * of scratch (the previous line of the streams whose predictor looks up), may be NULL when ws_elems is 0.
 * ELD_EINVAL before any device work: a null blob / streams / tables / out / status with nstreams > 0; nstreams or ntables < 0 (ntables < 1
 * with streams); bits outside the set; H, W, Hm, Wm < 1, top or left < 0, top + Hm > H, left + Wm > W, H * W >= 2^31; lin_len outside
 * [0, 65536] or lin null with lin_len > 0; lanes outside [0, 64]; ws null with ws_elems > 0; out, lin or ws not 2-byte, streams, tables or
 * status not 4-byte aligned.  nstreams == 0 is a successful no-op. */
int eld_dng_unpack_u16(const uint8_t* blob, size_t blob_bytes, const EldDngStream* streams, int nstreams, int bits, int big_endian, int H, int W,
                       int top, int left, int Hm, int Wm, const uint16_t* lin, int lin_len, uint16_t* out, int32_t* status, void* stream);
int eld_dng_ljpeg_u16(const uint8_t* blob, size_t blob_bytes, const EldDngStream* streams, int nstreams, const EldDngHuff* tables, int ntables,
                      int H, int W, int top, int left, int Hm, int Wm, const uint16_t* lin, int lin_len, uint16_t* ws, size_t ws_elems, int lanes,
                      uint16_t* out, int32_t* status, void* stream);

/* ---- DNG raw encode: lossless-JPEG tiles (csrc/dng_enc.hip, csrc/dng_enc_dev.h, eld_amd/dng.py) --------------------------------
 * Appended without a change of ELD_ABI_VERSION: four new symbols, no existing call changed.  The mosaic[H][W] is cut into tiles of th x tw,
 * th and tw multiples of 16; stream s = ty * ceil(W / tw) + tx is the tile at (ty * th, tx * tw), stored whole: its sample (r, c) is
 * mosaic[min(y0 + r, H - 1)][min(x0 + c, W - 1)].  A stream is ITU-T T.81 process 14 with two components of tw / 2 samples per line (the sample
 * sequence is the tile's raster), predictor 1, no point transform: sample (r, c) is predicted by (r, c - 2), the first two of a row by
 * (r - 1, c), the first two of the tile by 2^(bits - 1); differences are modulo 65536 and SSSS = 16 carries no extra bits.
 *
 * Units.  `segment` is in SAMPLES: a stream's th * tw samples are cut into ceil(th * tw / segment) segments, one workgroup each; a multiple of
 * 64 in [64, ELD_DNG_ENC_MAX_SEGMENT], 0: ELD_DNG_ENC_SEGMENT.  `chunk` is in BYTES of a stream's unstuffed entropy data, one workgroup each; a
 * multiple of 16 in [16, ELD_DNG_ENC_MAX_CHUNK], 0: ELD_DNG_ENC_CHUNK.  With nstreams = ceil(H / th) * ceil(W / tw) and nseg = segments per
 * stream:
 *   eld_dng_enc_hist_u16    hist[(s * nseg + g) * 17 + ssss]: how many samples of segment g of stream s fall into each category; maxcode[s]:
 *                           the largest code of the stream (bits is not looked at here beyond its range: the caller compares).
 *   eld_dng_enc_pack_u16    tables[s * 17 + ssss] = (code length << 16) | code, length 0 for a category the stream does not hold;
 *                           seg_bit[s * (nseg + 1) + g]: the first bit of segment g inside stream s, [.. + nseg]: the stream's bit count;
 *                           raw_dword[s]: the dword of `raw` at which stream s starts.  raw (raw_dwords dwords) is zeroed here, then every
 *                           segment writes its bits MSB-first; the last one pads the stream's last byte with 1-bits.  A segment whose bit count
 *                           differs from seg_bit's writes nothing.  The first and last dword of a segment go out as atomic ORs, so the result
 *                           does not depend on the order of execution.
 *   eld_dng_enc_ffcount_u8  count[k]: the FF bytes among the nbytes (<= chunk) bytes of raw at chunks[k].src.
 *   eld_dng_enc_stuff_u8    byte i of chunk k goes to out[chunks[k].dst + ffbefore[k] + i + (the FF bytes of the chunk before i)], a 00 behind
 *                           every FF; with ffbefore the exclusive running sum of count, the streams come out stuffed and back to back.
 * Every write is compared with raw_dwords resp. out_bytes, every read with raw_bytes and the mosaic.
 * ELD_EINVAL before any device work: a null pointer; H or W < 1, H * W >= 2^31; th or tw < 16 or no multiple of 16 (so tw is even), th * tw > 2^24;
 * more than 65535 tiles; bits outside [8, 16]; segment resp. chunk outside its set; nchunks < 0; mosaic not 2-byte, the uint32 arrays, raw and out not 4-byte aligned.
 * nchunks == 0 is a successful no-op. */
#define ELD_DNG_ENC_SEGMENT 2048
#define ELD_DNG_ENC_MAX_SEGMENT 8192
#define ELD_DNG_ENC_CHUNK 4096
#define ELD_DNG_ENC_MAX_CHUNK 4096

typedef struct EldDngEncChunk {    /* 16 bytes */
    uint32_t src;                  /* byte offset of the chunk in raw (a multiple of 16 reads fastest) */
    uint32_t nbytes;               /* 1 .. chunk */
    uint32_t dst;                  /* byte offset in out of the chunk's first byte were no FF in front of it */
    uint32_t reserved;
} EldDngEncChunk;

int eld_dng_enc_hist_u16(const uint16_t* mosaic, int H, int W, int th, int tw, int bits, int segment, uint32_t* hist, uint32_t* maxcode, void* stream);
int eld_dng_enc_pack_u16(const uint16_t* mosaic, int H, int W, int th, int tw, int bits, int segment, const uint32_t* tables, const uint32_t* seg_bit,
                         const uint32_t* raw_dword, uint32_t* raw, size_t raw_dwords, void* stream);
int eld_dng_enc_ffcount_u8(const uint8_t* raw, size_t raw_bytes, const EldDngEncChunk* chunks, int nchunks, int chunk, uint32_t* count, void* stream);
int eld_dng_enc_stuff_u8(const uint8_t* raw, size_t raw_bytes, const EldDngEncChunk* chunks, int nchunks, int chunk, const uint32_t* ffbefore,
                         uint8_t* out, size_t out_bytes, void* stream);

/* ---- DNG opcode lists: the mosaic-domain opcodes per site (csrc/dng_opcodes.hip, csrc/dng_opcodes_dev.h, eld_amd/dng_opcodes.py) ----
 * Appended without a change of ELD_ABI_VERSION: two new symbols, no existing call changed.  A program is at most ELD_DNG_MAX_OPS operation
 * records in HOST memory (they are validated here and travel as kernel arguments) and one parameter blob of at most ELD_DNG_MAX_BLOB bytes in
 * DEVICE memory, 8-byte aligned.  A record's area is already clipped to the Hm x Wm image (0 <= top < bottom <= Hm, 0 <= left < right <= Wm),
 * its pitches are >= 1, and data_off (a multiple of 4) is where its parameters start in the blob:
 *   MAPTABLE     n0 = table size 1..65536; n0 uint16.               out = float32(table[min(rint(v * 65535), n0 - 1)]) / 65535
 *   MAPPOLY      n0 = degree 0..8; n0 + 1 float32 c0..cn.           out = clip(Horner from cn, product and sum rounded apart)
 *   GAINMAP      n0 x n1 map points (plane 0 of the file's map), n0 * n1 <= 2^24; n0 * n1 float32, row-major.  p[0..3] = MapSpacingV,
 *                MapSpacingH, MapOriginV, MapOriginH.             out = clip(v * bilinear gain)
 *   DELTAPERROW / DELTAPERCOL / SCALEPERROW / SCALEPERCOL   n0 = entries; n0 float32; the area's last addressed line must index below n0.
 *                                                                  out = clip(v + d[k]) resp. clip(v * s[k]), k = (y - top) / row_pitch
 *   VIGNETTE     (gain entry point only) p[0..4] = k0..k4, p[5], p[6] = the centre cx, cy in relative coordinates; no blob data.
 * A site (y, x) is addressed when top <= y < bottom, (y - top) % row_pitch == 0, and likewise in x.  clip is to [0, 1].  The arithmetic -- the
 * float64 map coordinate at pixel centres, the order and rounding of every float32 operation -- is the contract of DESIGN.md sec. 29, restated
 * by tests/dng_opcodes_ref.py bit for bit.
 *   eld_dng_opcodes_apply_f32   out[n][y][x] = the program run in record order on in[n][y][x]; one pass, 4 B read and 4 B written per site.
 *                               in == out (in place) or no overlap.  A NaN site passes through unchanged.  VIGNETTE is ELD_EINVAL here.
 *   eld_dng_opcodes_gain_f32    out[y][x] = the float32 product, in record order from 1, of the factors of the GAINMAP, SCALEPERROW,
 *                               SCALEPERCOL and VIGNETTE records that address the site; unclipped; any other kind is ELD_EINVAL.
 * map_lds_bytes: how many bytes of GAINMAP gains the kernel may copy into LDS (taken in record order while they fit; the rest is read from
 * the blob); < 0: the default, 32 KiB; at most 64 KiB.  The result does not depend on it.
 * ELD_EINVAL before any device work: a null or misaligned pointer (float32 arrays 4-byte, the blob 8-byte); N < 0 or > 65535; Hm, Wm < 1 or
 * Hm * Wm >= 2^31; nops outside [0, ELD_DNG_MAX_OPS]; blob_bytes > ELD_DNG_MAX_BLOB; in and out overlapping without being equal; any record
 * that fails the checks above or points beyond the blob.  N == 0 is a successful no-op; nops == 0 copies resp. writes 1. */
#define ELD_DNG_MAX_OPS 32
#define ELD_DNG_MAX_BLOB (64u << 20)
#define ELD_DNG_OP_VIGNETTE 3
#define ELD_DNG_OP_MAPTABLE 7
#define ELD_DNG_OP_MAPPOLY 8
#define ELD_DNG_OP_GAINMAP 9
#define ELD_DNG_OP_DELTAPERROW 10
#define ELD_DNG_OP_DELTAPERCOL 11
#define ELD_DNG_OP_SCALEPERROW 12
#define ELD_DNG_OP_SCALEPERCOL 13

typedef struct EldDngOp {          /* 104 bytes */
    int32_t kind;                  /* ELD_DNG_OP_*: the DNG opcode id */
    int32_t top, left, bottom, right;  /* the area, clipped to the image */
    int32_t row_pitch, col_pitch;
    int32_t n0, n1;                /* see above; n1: GAINMAP only */
    uint32_t data_off;             /* byte offset of the parameters in the blob, a multiple of 4 */
    uint32_t reserved[2];
    double p[7];                   /* GAINMAP: spacing V, H, origin V, H; VIGNETTE: k0..k4, cx, cy */
} EldDngOp;

int eld_dng_opcodes_apply_f32(const float* in, float* out, int N, int Hm, int Wm, const EldDngOp* ops, int nops, const uint8_t* blob,
                              size_t blob_bytes, int map_lds_bytes, void* stream);
int eld_dng_opcodes_gain_f32(float* out, int Hm, int Wm, const EldDngOp* ops, int nops, const uint8_t* blob, size_t blob_bytes,
                             int map_lds_bytes, void* stream);

/* ---- DNG WarpRectilinear: lens distortion and lateral CA on demosaiced camera RGB (csrc/warp.hip, csrc/warp_dev.h) ----
 * Appended without a change of ELD_ABI_VERSION: one new symbol, no existing call changed.
 *   rgb   (N,3,Hm,Wm) float32 camera RGB in DEVICE memory, as eld_render_* write it with ELD_RENDER_LINEAR_F32 and ccms NULL; 16-byte aligned.
 *   out   (N,3,Hm,Wm) uint8 (ELD_RENDER_SRGB8) or float32 (ELD_RENDER_LINEAR_F32), as the renders write it; it must not overlap rgb.
 *   warp  one EldWarp record in HOST memory (it is validated here and travels by value as a kernel argument).
 *   ccms, gamma, crf_E, crf_f, crf_n: the tail of eld_render_*, unchanged, applied to the three resampled values of a pixel.
 * The map (float64, every operation rounded on its own, no FMA), for destination pixel (x, y), set s = plane (nsets 3) or 0 (nsets 1),
 * k = warp->k[s] = kr0 - 1, kr1, kr2, kr3, kt0, kt1:
 *   dx = (x + 0.5) - cxp   dy = (y + 0.5) - cyp   r2 = (dx*dx + dy*dy) / m2   g = k[0] + r2*(k[1] + r2*(k[2] + r2*k[3]))
 *   nx = dx / m   ny = dy / m   tx = k[4]*(2*nx*ny) + k[5]*(r2 + 2*nx*nx)   ty = k[5]*(2*nx*ny) + k[4]*(r2 + 2*ny*ny)
 *   u = ((x + 0.5) + (g*dx + m*tx)) - 0.5        v = ((y + 0.5) + (g*dy + m*ty)) - 0.5
 * u is clamped to [-1, Wm] and v to [-1, Hm], NaN becoming -1; j0 = floor(u), t = float32(u - j0), likewise i0 from v; the taps j0-1 .. j0+2 and
 * i0-1 .. i0+2 are each clamped to the image (the edge is replicated).  No address is formed from a coordinate before these clamps.
 * Catmull-Rom in float32, every product and sum rounded on its own:
 *   w0 = t*(t*(-0.5*t + 1) - 0.5)   w1 = t*t*(1.5*t - 2.5) + 1   w2 = t*(t*(-1.5*t + 2) + 0.5)   w3 = t*t*(0.5*t - 0.5)
 *   h_i = ((w0x*p[i][0] + w1x*p[i][1]) + w2x*p[i][2]) + w3x*p[i][3]      val = ((w0y*h_0 + w1y*h_1) + w2y*h_2) + w3y*h_3      (unclamped)
 * With k = 0 the map is u = x, v = y exactly and the output is the tail of the input.  tests/warp_ref.py restates all of it bit for bit.
 * lds_bytes: the LDS a workgroup may use to stage the source boxes of its 32 x 64 tile (all three planes, halo included); a tile whose boxes
 * do not fit reads its taps from global memory.  < 0: the default, which is 0 (reading from global memory measured faster: DESIGN.md sec. 30);
 * 0: always from global memory; at most 65536.  The result does not depend on it.
 * ELD_EINVAL before any device work: rgb, out or warp NULL; rgb not 16-byte aligned, a float32 out not 4-byte aligned; N < 0 or > 65535;
 * Hm, Wm < 1, Hm * Wm >= 2^31 or more than 65535 * 32 rows; nsets not 1 or 3; a field of a used set, cxp, cyp, m or m2 not finite; m2 <= 0;
 * an unknown out_mode; the tail's rules (ccms 4-byte aligned, gamma > 0, crf_n 0 or >= 2 with both tables); lds_bytes > 65536; rgb and out
 * overlapping.  N == 0 is a successful no-op. */
typedef struct EldWarp {           /* 184 bytes */
    int32_t nsets;                 /* 1: one coefficient set for the three planes; 3: one per plane, R, G, B */
    int32_t reserved;
    double k[3][6];                /* per set kr0 - 1, kr1, kr2, kr3, kt0, kt1; sets beyond nsets are not read */
    double cxp, cyp;               /* the centre in pixels: cx * Wm, cy * Hm */
    double m, m2;                  /* m2 = mx*mx + my*my with mx = max(|cxp|, |Wm - cxp|), my = max(|cyp|, |Hm - cyp|); m = sqrt(m2) */
} EldWarp;

int eld_warp_rgb_f32(const float* rgb, void* out, int out_mode, int N, int Hm, int Wm, const EldWarp* warp, const float* ccms, float gamma,
                     const float* crf_E, const float* crf_f, int crf_n, int lds_bytes, void* stream);

/* ---- Baseline JPEG encode of an sRGB render (csrc/jpeg.hip, csrc/jpeg_dev.h, eld_amd/jpeg.py) -------------------------------
 * Appended without a change of ELD_ABI_VERSION: three new symbols, no existing call changed.  rgb is planar uint8 (3, H, W) in DEVICE memory.
 * The picture is ITU-T T.81 process 1 (baseline sequential DCT, 8 bits), components Y, Cb, Cr in one interleaved scan; subsampling is
 * ELD_JPEG_444 (every component 1 x 1, MCU 8 x 8, 3 blocks) or ELD_JPEG_420 (Y 2 x 2, MCU 16 x 16, 6 blocks: Y00 Y01 Y10 Y11 Cb Cr).  With
 * mcux = ceil(W / MCU width), mcuy likewise, nblocks = mcux * mcuy * blocks per MCU; block b = MCU (b / blocks per MCU, row-major) and its
 * k-th block.  The arithmetic is libjpeg's, integer throughout (DESIGN.md sec. 31 states it; tests/jpeg_ref.py restates it bit for bit): colour
 * conversion with 16 fraction bits, edges by replication, the h2v2 downsampler with its alternating bias, the "slow integer" forward DCT,
 * the quantiser sign(c) * ((|c| + 4q) / 8q), and libjpeg's dummy blocks: a Y block of a 4:2:0 MCU wholly outside ceil(W / 8) x ceil(H / 8) has no
 * AC terms and the DC of the block in front of it in the MCU (both blocks of a dummy bottom row: the DC of the MCU's top-right block).
 *   eld_jpeg_coef_u8    coef[b * 64 + k]: quantised coefficient k (zigzag order) of block b.  qtables: 2 x 64 divisors in natural (row-major)
 *                       order in HOST memory, luma then chroma, each 1..255.  coef_elems must be nblocks * 64.
 *   eld_jpeg_hist_i16   `segment` is in BLOCKS: the nblocks are cut into nseg = ceil(nblocks / segment) segments, one workgroup each; a multiple of
 *                       ELD_JPEG_MIN_SEGMENT up to ELD_JPEG_MAX_SEGMENT, 0: ELD_JPEG_SEGMENT.  hist[g * ELD_JPEG_HIST + i]: how often segment g uses
 *                       symbol i of the four alphabets laid end to end: luma DC sizes (12), chroma DC sizes (12), luma AC run/size bytes (256),
 *                       chroma AC (256).  A DC difference takes the previous block of the same component in scan order (0 for the first); sizes
 *                       beyond 11 (DC) or 10 (AC) do not arise from eld_jpeg_coef_u8 and are counted as the largest size.  hist_elems must be
 *                       nseg * ELD_JPEG_HIST.
 *   eld_jpeg_pack_i16   tables[ELD_JPEG_TABLE]: (code length << 16) | code per symbol, 0 for a symbol without a code, laid out as luma DC (17
 *                       entries, 12 used), chroma DC (17), luma AC (256), chroma AC (256).  seg_bit[g]: the first bit of segment g, [nseg]: the bit
 *                       count of the scan (uint64).  raw (raw_dwords dwords) is zeroed here, then every segment writes its bits MSB-first; the last one
 *                       pads the last byte with 1-bits.  A segment whose bit count differs from seg_bit's writes nothing.  A segment's bits are
 *                       assembled in an LDS image when they fit lds_bytes (< 0: the default, 32 KiB; at most 61440) and leave as whole dwords, the
 *                       first and last one by atomic OR; a segment that does not fit ORs every dword into raw directly.  Either way the result does
 *                       not depend on lds_bytes or on the order of execution.  The bytes still lack their FF stuffing: eld_dng_enc_ffcount_u8 and
 *                       eld_dng_enc_stuff_u8 do that for any byte buffer.
 * Every read is compared with coef_elems resp. the picture, every write with coef_elems, hist_elems resp. raw_dwords.
 * ELD_EINVAL before any device work: a null pointer; rgb is any address, coef must be 16-byte, hist, tables and raw 4-byte, seg_bit 8-byte
 * aligned; H or W outside [1, 65535]; H * W >= 2^31; a subsampling other than the two; a segment outside its set; a quantisation divisor outside
 * [1, 255]; coef_elems or hist_elems other than stated; raw_dwords < 1; lds_bytes > 61440. */
#define ELD_JPEG_444 0
#define ELD_JPEG_420 2
#define ELD_JPEG_SEGMENT 1024
#define ELD_JPEG_MIN_SEGMENT 8
#define ELD_JPEG_MAX_SEGMENT 2048
#define ELD_JPEG_HIST 536
#define ELD_JPEG_TABLE 546

int eld_jpeg_coef_u8(const uint8_t* rgb, int H, int W, int subsampling, const uint16_t* qtables, int16_t* coef, size_t coef_elems, void* stream);
int eld_jpeg_hist_i16(const int16_t* coef, size_t coef_elems, int H, int W, int subsampling, int segment, uint32_t* hist, size_t hist_elems,
                      void* stream);
int eld_jpeg_pack_i16(const int16_t* coef, size_t coef_elems, int H, int W, int subsampling, int segment, const uint32_t* tables,
                      const uint64_t* seg_bit, uint32_t* raw, size_t raw_dwords, int lds_bytes, void* stream);

/* ---- Edge-directed Bayer demosaic for the full-resolution render (csrc/demosaic_edge.hip, csrc/demosaic_edge_dev.h) --------
 * Appended without a change of ELD_ABI_VERSION: two new symbols, no existing call changed.  eld_render_bayer_edge is eld_render_bayer with
 * another step 2: the same arguments, output modes, step 1 (v = min(max(p * gain, 0), 1)) and step 3 (the matrix, then for ELD_RENDER_SRGB8 the
 * clamp, the gamma table / pow / CRF and the quantiser of eld_isp_process; camera RGB when ccms is NULL with ELD_RENDER_LINEAR_F32).
 * Step 2, per mosaic site, float32, one rounding per operation, evaluated exactly as written (no FMA; the division is correctly rounded).
 * Every stage is evaluated on v extended by mirroring without repeating the edge (index -1 -> 1, H -> H - 2, period 2 (H - 1), as NumPy's
 * pad mode 'reflect'), which preserves CFA parity for any h, w >= 1; the stages address the extension up to 4 sites.  c is the site's own
 * value, W E N S its 4-neighbours, WW EE NN SS those at distance 2:
 *   A, every site:     a_h = (2*c - WW) - EE             a_v = (2*c - NN) - SS
 *                      d_h = |W - E| + |a_h|             d_v = |N - S| + |a_v|
 *   B, every site:     S_h, S_v = the sums of d_h, d_v over the 3x3 window; the nine terms are added to a zero in raster order (rows top to
 *                      bottom, left to right)
 *   C:                 G^ = c at G sites; at R and B sites
 *                      g_h = (W + E)*0.5 + a_h*0.25      g_v = (N + S)*0.5 + a_v*0.25
 *                      w_h = S_v*S_v + 1e-6f             w_v = S_h*S_h + 1e-6f
 *                      G^  = g_h + (g_v - g_h) * (w_v / (w_h + w_v))
 *   D:                 delta = c - G^ at R and B sites; for k in {R, B}:
 *                      at a k site                                  c
 *                      at the other colour's site                   G^ + ((delta_NW + delta_NE) + (delta_SW + delta_SE))*0.25
 *                      at a G site with k to its left and right     G^ + (delta_W + delta_E)*0.5
 *                      at a G site with k above and below           G^ + (delta_N + delta_S)*0.5
 * Sampled values pass through unchanged; a frame of one colour on a dyadic grid comes back exact (equal gradients make the weight exactly
 * 0.5, and it multiplies a zero); the output is finite for p * gain of any finite value (w_h + w_v >= 2e-6).
 * ELD_EINVAL before any launch: as eld_render_bayer, except that h and w may be 1 (mosaic sides from 2) and must not exceed 2^28.
 * eld_render_bayer_edge_tile (HOST, no device work): the tile of mosaic sites one workgroup owns and, when lds_bytes is not NULL, the LDS the
 * kernel declares; ELD_EINVAL for a null tile_h or tile_w. */
int eld_render_bayer_edge(const float* packed, const int* raw_pattern, const float* wbs, const float* ccms, void* out, int out_mode,
                          int N, int h, int w, float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream);
int eld_render_bayer_edge_tile(int* tile_h, int* tile_w, int* lds_bytes);

/* ---- Directional X-Trans demosaic for the full-resolution render (csrc/demosaic_xdir.hip, csrc/demosaic_xdir_dev.h) -------
 * Appended without a change of ELD_ABI_VERSION: two new symbols, no existing call changed.  eld_render_xtrans_dir is eld_render_xtrans with
 * another step 2: the same arguments, output modes, step 1 (v = min(max(p * gain, 0), 1), the gain by plane colour) and step 3 (the matrix,
 * then for ELD_RENDER_SRGB8 the clamp, the gamma table / pow / CRF and the quantiser of eld_isp_process; camera RGB when ccms is NULL with
 * ELD_RENDER_LINEAR_F32).
 * Step 2, per mosaic site, float32, one rounding per operation, evaluated exactly as written (no FMA; the division is correctly rounded).
 * Every stage is evaluated with full windows on v extended by 6 sites (one cell) with the mirror that keeps every site's colour: the 6x6 cell
 * (row 0 = R B G B R G) is symmetric about the rows = 0 (mod 3) and the columns = 2 (mod 3) only, so
 *     y < 0 -> -y      y >= H -> 2*(H - 3) - y      x < 0 -> 4 - x      x >= W -> 2*(W - 1) - x,
 * repeated until the index is inside (a 6-site side needs two rounds).  v(k) is the value k sites along an axis from the site:
 *   A, every site:     G0 = v at G sites; elsewhere sum(wt * v) / sum(wt) over the G sites of the 3x3 window, wt = [1 2 1] x [1 2 1]: the
 *                      products are added to a zero in raster order (rows top to bottom, left to right), then one division
 *   B, every site:     d_h = |G0_W - G0_E| + |(2*G0 - G0_WW) - G0_EE|          d_v likewise with N, S
 *                      S_h, S_v = the sums of d_h, d_v over the 3x3 window, the nine terms added to a zero in raster order
 *   C:                 G^ = v at G sites.  An R or B site has one solitary axis (both neighbours and both second neighbours are G) and one
 *                      paired axis (one neighbour, a = -1 or +1, is G; the site at 2a has the site's colour, the one at -2a is G):
 *                      solitary:  s1 = v(-1) + v(1)    s2 = v(-2) + v(2)    g = s1*0.5f + (s1 - s2)*(46/256)
 *                      paired:    g = (v(a) + (v(-2a) - v(a))*(33/256)) + (v(0) - v(2a))*(92/256)
 *                      with g_h along the row and g_v along the column:
 *                      w_h = S_v*S_v + 1e-6f             w_v = S_h*S_h + 1e-6f
 *                      G^  = g_h + (g_v - g_h) * (w_v / (w_h + w_v))
 *   D:                 delta = v - G^ at R and B sites; for k in {R, B}: v at a k site, elsewhere
 *                      G^ + sum(wt * delta) / sum(wt) over the k sites of the 5x5 window, wt = [1 2 3 2 1] x [1 2 3 2 1], added as in A
 * Sampled values pass through unchanged; a frame of one colour comes back exact where the sums of stages A and D are (dyadic values: the
 * axis estimates are a mean plus differences that vanish); the output is finite for p * gain of any finite value (w_h + w_v >= 2e-6).
 * ELD_EINVAL before any launch: as eld_render_xtrans; h and w must not exceed 2^28.
 * eld_render_xtrans_dir_tile (HOST, no device work): the tile of mosaic sites one workgroup owns (whole cells) and, when lds_bytes is not
 * NULL, the LDS the kernel declares; ELD_EINVAL for a null tile_h or tile_w. */
int eld_render_xtrans_dir(const float* packed, const float* wbs, const float* ccms, void* out, int out_mode, int N, int h, int w, float gamma,
                          const float* crf_E, const float* crf_f, int crf_n, void* stream);
int eld_render_xtrans_dir_tile(int* tile_h, int* tile_w, int* lds_bytes);

/* ---- The frame of the full-resolution render: crop, antialiased resize, orientation (csrc/frame.hip, csrc/frame_dev.h) ----
 * Appended without a change of ELD_ABI_VERSION: two new symbols, no existing call changed.
 *   rgb   (N,3,Hs,Ws) float32 camera RGB in DEVICE memory, as eld_render_* write it with ELD_RENDER_LINEAR_F32 and ccms NULL, or
 *         eld_warp_rgb_f32 with the same; 4-byte aligned.
 *   out   (N,3,Ho,Wo) uint8 (ELD_RENDER_SRGB8) or float32 (ELD_RENDER_LINEAR_F32): the UPRIGHT picture.  orientation (TIFF / Exif, 1 .. 8)
 *         says how it is turned: the unoriented grid is Hc x Wc = Ho x Wo for orientation <= 4 and Wo x Ho for orientation >= 5, and upright
 *         pixel (Y, X) is unoriented pixel (i, j) =
 *           1 (Y, X)             2 (Y, Wc-1-X)        3 (Hc-1-Y, Wc-1-X)   4 (Hc-1-Y, X)
 *           5 (X, Y)             6 (Hc-1-X, Y)        7 (Hc-1-X, Wc-1-Y)   8 (X, Wc-1-Y)
 *   ystart, ycount (Hc int32), yw (Hc x Ty float32), xstart, xcount (Wc int32), xw (Tx x Wc float32): the tap tables, in DEVICE memory,
 *         4-byte aligned.  Unoriented row i is the weighted sum of the source rows ystart[i] .. ystart[i] + ycount[i] - 1 with the weights
 *         yw[i * Ty + 0 ..]; unoriented column j likewise from xstart[j], xcount[j] and the weights xw[0 * Wc + j], xw[1 * Wc + j], ...
 *         (tap-major: the row pass reads one tap of 64 neighbouring columns at a time).  The crop and the filter are in the tables alone (eld_amd.isp.Frame.taps builds them: 'area'
 *         and 'lanczos').  Every count is clamped to [1, T] and every tap index to the plane before an address is formed from it, so no
 *         table content reads or writes outside the buffers; padding behind a row's count is never read.
 *   row0, rows: the source rows the vertical tables use, row0 .. row0 + rows - 1 (the caller takes min(ystart) and max(ystart + ycount));
 *         a vertical tap outside them is clamped into them.
 *   workspace: float32 (N,3,rows,Wc) in DEVICE memory, workspace_bytes of it; it holds the horizontal sums between the two kernels and
 *         overlaps neither rgb nor out.
 *   ccms, gamma, crf_E, crf_f, crf_n: the tail of eld_render_*, unchanged, applied to the three resampled values of a pixel.
 * The sums, float32, strictly ascending tap order, every product and sum rounded on its own (no FMA), no initial zero:
 *   h[r][j] = ((xw0*p[r][s] + xw1*p[r][s+1]) + xw2*p[r][s+2]) + ...      s = xstart[j]
 *   v[i][j] = ((yw0*h[t][j] + yw1*h[t+1][j]) + yw2*h[t+2][j]) + ...      t = ystart[i]
 * A single tap of weight 1.0 on both axes hands the source value to the tail unchanged (-0.0 and NaN included): with the full rectangle at
 * its own size and orientation 1 the output is the render's own.  tests/frame_ref.py restates all of it bit for bit.
 * ELD_EINVAL before any device work: a NULL or misaligned pointer; N < 0 or > 21845; Hs, Ws, Ho, Wo < 1; Hs * Ws, Ho * Wo or rows * Wc
 * >= 2^31; orientation outside 1 .. 8; Ty or Tx outside 1 .. 4096; row0 < 0, rows < 1 or row0 + rows > Hs; rows > 262140; an unknown
 * out_mode; the tail's rules; rgb, out and workspace overlapping.  ELD_EWS: workspace_bytes < N * 3 * rows * Wc * 4.  N == 0 is a
 * successful no-op.
 * eld_frame_rgb_tile (HOST, no device work): the tile of unoriented outputs one workgroup of the column pass owns and, when lds_bytes is not
 * NULL, the most LDS an instantiation declares; ELD_EINVAL for a null tile_h or tile_w. */
int eld_frame_rgb_f32(const float* rgb, void* out, int out_mode, int N, int Hs, int Ws, int Ho, int Wo, int orientation,
                      const int* ystart, const int* ycount, const float* yw, int Ty, const int* xstart, const int* xcount,
                      const float* xw, int Tx, int row0, int rows, float* workspace, size_t workspace_bytes, const float* ccms,
                      float gamma, const float* crf_E, const float* crf_f, int crf_n, void* stream);
int eld_frame_rgb_tile(int* tile_h, int* tile_w, int* lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ELD_AMD_H */
