"""ctypes binding of include/eld_amd.h (the drop-in C ABI).  No torch types cross the ABI:
device pointers travel as integers, the stream as the raw hipStream_t."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('ELD_AMD_LIB') or os.path.join(_HERE, 'libeld_amd.so')      # ELD_AMD_LIB: developer builds (tools/build_dev.sh)

# flags / enums of include/eld_amd.h
SHOT_POISSON, SHOT_GAUSS, READ_GAUSS, READ_TL, ROW, QUANT, CBIAS, CLIP = 1, 2, 4, 8, 16, 32, 64, 128
AUG_NOTRANSPOSE = 256
CFA_XTRANS = 512
DARK = 1024             # 'D': signal-independent noise read from a pool of dark frames (eld_noise_forward_dark only)
COL = 2048              # 'C': per-sensor-column Gaussian; its scale travels as the float bits of EldNoiseParams.reserved[0]
IN_F32, IN_U16 = 0, 1
ROUND_TRUNC, ROUND_NEAREST, ROUND_TRUNC_F32 = 0, 1, 2      # write-back rounding (eld_unpack_raw_*_u16)
RENDER_SRGB8, RENDER_LINEAR_F32 = 0, 1                      # out_mode of eld_render_bayer / eld_render_xtrans
NPLANES = 6
PAIRSTATS_BINS = 61                                           # ELD_PAIRSTATS_BINS
PLANE = {'counts': 0, 'n_shot': 1, 'n_read': 2, 't_tl': 3, 'n_row': 4, 'u_q': 5}
PLANE_NCOL = 6          # ELD_PLANE_NCOL: the column normal; the inject / dump buffers hold NPLANES_COL planes when COL is in the flags
NPLANES_COL = 7

# numpy mirror of struct EldNoiseParams (64 bytes)
NOISE_PARAMS_DTYPE = np.dtype([
    ('K', '<f4'), ('g_scale', '<f4'), ('tl_lambda', '<f4'), ('tl_scale', '<f4'), ('row_scale', '<f4'),
    ('q_step', '<f4'), ('saturation', '<f4'), ('ratio', '<f4'), ('color_bias', '<f4', (4,)),
    ('sample_id_lo', '<u4'), ('sample_id_hi', '<u4'), ('reserved', '<u4', (2,))])
assert NOISE_PARAMS_DTYPE.itemsize == 64
# numpy mirrors of struct EldPoolFrame and struct EldCropRecord (16 bytes each)
POOL_FRAME_DTYPE = np.dtype([('offset', '<u8'), ('Hm', '<i4'), ('Wm', '<i4')])
CROP_RECORD_DTYPE = np.dtype([('frame', '<i4'), ('y0', '<i4'), ('x0', '<i4'), ('ratio', '<f4')])
assert POOL_FRAME_DTYPE.itemsize == 16 and CROP_RECORD_DTYPE.itemsize == 16
# numpy mirrors of struct EldDngStream (64 bytes) and struct EldDngHuff (1196 bytes); the status words of the two DNG decoders
DNG_STREAM_DTYPE = np.dtype([('data_off', '<u4'), ('data_len', '<u4'), ('x0', '<i4'), ('y0', '<i4'), ('tw', '<i4'), ('th', '<i4'), ('P', '<i4'),
                             ('X', '<i4'), ('Y', '<i4'), ('Nf', '<i4'), ('pred', '<i4'), ('table', '<u2', (4,)), ('ws_off', '<u4'),
                             ('reserved', '<u4', (2,))])
DNG_FAST_BITS = 9
DNG_HUFF_DTYPE = np.dtype([('fast', '<u2', (1 << DNG_FAST_BITS,)), ('maxcode', '<i4', (17,)), ('valoff', '<i4', (17,)), ('vals', 'u1', (32,)),
                           ('nvals', '<i4')])
assert DNG_STREAM_DTYPE.itemsize == 64 and DNG_HUFF_DTYPE.itemsize == 1196
# struct EldDngEncChunk (16 bytes) and the segment / chunk lengths of the lossless-JPEG encoder (samples resp. bytes)
DNG_ENC_CHUNK_DTYPE = np.dtype([('src', '<u4'), ('nbytes', '<u4'), ('dst', '<u4'), ('reserved', '<u4')])
DNG_ENC_SEGMENT, DNG_ENC_MIN_SEGMENT, DNG_ENC_MAX_SEGMENT = 2048, 64, 8192
DNG_ENC_CHUNK, DNG_ENC_MIN_CHUNK, DNG_ENC_MAX_CHUNK = 4096, 16, 4096
# struct EldDngOp (104 bytes): one operation record of a compiled opcode program (eld_amd/dng_opcodes.py); the limits of a program
DNG_OP_DTYPE = np.dtype([('kind', '<i4'), ('top', '<i4'), ('left', '<i4'), ('bottom', '<i4'), ('right', '<i4'), ('row_pitch', '<i4'),
                         ('col_pitch', '<i4'), ('n0', '<i4'), ('n1', '<i4'), ('data_off', '<u4'), ('reserved', '<u4', (2,)), ('p', '<f8', (7,))])
assert DNG_OP_DTYPE.itemsize == 104
DNG_MAX_OPS, DNG_MAX_BLOB = 32, 64 << 20
# struct EldWarp (184 bytes): DNG WarpRectilinear for eld_warp_rgb_f32 (eld_amd/dng_opcodes.py Warp.record); k holds kr0 - 1 in place of kr0
WARP_DTYPE = np.dtype([('nsets', '<i4'), ('reserved', '<i4'), ('k', '<f8', (3, 6)), ('cxp', '<f8'), ('cyp', '<f8'), ('m', '<f8'), ('m2', '<f8')])
assert WARP_DTYPE.itemsize == 184
WARP_MAX_LDS = 64 << 10
# the baseline-JPEG encoder: subsampling codes, segment lengths in blocks, the bins of a histogram and the entries of the code tables
JPEG_444, JPEG_420 = 0, 2
JPEG_SEGMENT, JPEG_MIN_SEGMENT, JPEG_MAX_SEGMENT = 1024, 8, 2048
JPEG_HIST, JPEG_TABLE, JPEG_MAX_LDS = 536, 546, 60 << 10
DNG_STATUS = {0: 'ok', 1: 'truncated: the data ended before the last sample', 2: 'invalid code: bits that are no code of the Huffman table',
              3: 'too many samples: the stream holds more samples than its tile', 4: 'bad record: a field out of range'}

_vp, _i, _u32, _u64, _f, _d, _sz = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float, C.c_double, C.c_size_t

# name -> (restype, argtypes): exactly the prototypes of include/eld_amd.h
SIGNATURES = {
    'eld_abi_version': (_i, []),
    'eld_build_info': (C.c_char_p, []),
    'eld_error_string': (C.c_char_p, [_i]),
    'eld_noise_forward': (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _i, _u32, _u64, _vp, _vp, _vp]),
    'eld_noise_forward_strided': (_i, [_vp, _i, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _u32, _u64, _vp, _vp, _vp]),
    'eld_noise_forward_dark': (_i, [_vp, _i, _sz, _vp, _sz, _vp, _i, _i, _i, _i, _u32, _u64, _vp, _vp,
                                    _vp, _sz, _vp, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _vp]),
    'eld_augment_u16': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _u32, _vp]),
    'eld_philox_rounds': (_i, []),
    'eld_philox_words': (_i, [_vp, _u32, _u32, _u64, _u32, _u32, _u64, _vp]),
    'eld_pack_bayer': (_i, [_vp, _vp, _i, _i, _i, _vp]),
    'eld_unpack_bayer': (_i, [_vp, _vp, _i, _i, _i, _vp]),
    'eld_pack_xtrans': (_i, [_vp, _vp, _i, _i, _i, _vp]),
    'eld_unpack_xtrans': (_i, [_vp, _vp, _i, _i, _i, _vp]),
    'eld_pack_raw_bayer_u16': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _f, _vp]),
    'eld_pack_raw_xtrans_u16': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp]),
    'eld_pack_raw_bayer_u16_gain': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _f, _vp, _vp]),
    'eld_pack_raw_xtrans_u16_gain': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp, _vp]),
    'eld_unpack_raw_bayer_u16': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _f, _i, _vp]),
    'eld_unpack_raw_xtrans_u16': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _i, _vp]),
    'eld_crop_pack_raw_bayer_u16': (_i, [_vp, _sz, _vp, _i, _i, _i, _vp, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _f, _vp, _vp]),
    'eld_crop_pack_raw_xtrans_u16': (_i, [_vp, _sz, _vp, _i, _i, _i, _vp, _i, _i, _i, _f, _f, _vp, _vp]),
    'eld_augment': (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _u32, _vp]),
    'eld_calib_bias_stats_workspace_bytes': (_sz, [_i, _i]),
    'eld_calib_bias_stats': (_i, [_vp, _i, _i, _i, C.POINTER(C.c_int), _vp, _vp, _vp, _sz, _vp]),
    'eld_calib_bias_residual': (_i, [_vp, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_double), _vp, _vp, _vp, _vp]),
    'eld_calib_flat_stats_workspace_bytes': (_sz, [_i, _i]),
    'eld_calib_flat_stats': (_i, [_vp, _i, _i, _i, C.POINTER(C.c_int), _i, _vp, _vp, _sz, _vp]),
    'eld_calib_ppcc_workspace_bytes': (_sz, [_i, _sz, _i]),
    'eld_calib_ppcc': (_i, [_vp, _i, _sz, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    'eld_calib_cell_stats_workspace_bytes': (_sz, [_i, _i, _i]),
    'eld_calib_cell_stats': (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    'eld_calib_cell_residual': (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_double), _vp, _vp, _vp, _vp]),
    'eld_calib_cell_flat_stats_workspace_bytes': (_sz, [_i, _i, _i]),
    'eld_calib_cell_flat_stats': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    'eld_unet_param_offsets': (_i, [_i, _i, _vp]),
    'eld_unet_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'eld_unet_forward': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    'eld_unet_forward_bf16': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    'eld_unet_backward': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    'eld_unet_backward_bf16': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _vp]),
    'eld_unet_backward_buckets': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    'eld_unet_forward_ex': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'eld_unet_infer_ex': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'eld_unet_backward_ex': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    'eld_unet_forward_loss_ex': (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _f, _vp]),
    'eld_conv_fp32_algo': (_i, [_i]),
    'eld_debug_conv_prof': (None, [_vp]),
    'eld_debug_kernel_mask': (_i, [_i]),
    'eld_debug_ws_state_entries': (_i, []),
    'eld_isp_process': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _i, _vp]),
    'eld_isp_process_xtrans': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp, _vp, _i, _vp]),
    'eld_render_bayer': (_i, [_vp, C.POINTER(C.c_int), _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp]),
    'eld_render_xtrans': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp]),
    'eld_debug_xtrans_demosaic_tables': (_i, [C.POINTER(C.c_int), _i]),
    'eld_defect_deviation_workspace_bytes': (_sz, [_i, _i]),
    'eld_defect_deviation': (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int), _vp, _vp, _sz, _vp]),
    'eld_defect_flags': (_i, [_vp, _i, _i, C.c_int32, C.c_int32, _vp, _vp]),
    'eld_defect_repair_u16': (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_int), _vp, _vp]),
    'eld_debug_xtrans_defect_tables': (_i, [C.POINTER(C.c_int), _i]),
    'eld_hist_u16': (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int32), _i, _vp, _vp, _vp]),
    'eld_hist_f32': (_i, [_vp, _vp, _i, _i, _i, _i, C.POINTER(C.c_int), _i, _vp, _i, _vp, _vp]),
    'eld_struct_sums_u16': (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int32), _vp, _vp, _vp, _vp, _vp]),
    'eld_struct_cross_u16': (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int32), _vp, C.POINTER(C.c_int32), _i, _vp, _vp]),
    'eld_shading_fit_u16': (_i, [_vp, _sz, _vp, _i, _i, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_int32), _i, _vp, _vp, _vp, _vp]),
    'eld_shading_apply_u16': (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _f, _vp, _vp]),
    'eld_pack_raw_bayer_u16_shaded': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _f, _vp, _vp, _vp, _f, _vp]),
    'eld_pack_raw_xtrans_u16_shaded': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _f, _vp]),
    'eld_pair_level_stats_workspace_bytes': (_sz, [_i, _i, _i]),
    'eld_pair_level_stats_u16': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int32), _i, _vp, _vp, _vp, _sz, _vp]),
    'eld_tile_noise_workspace_bytes': (_sz, [_i, _i, _i]),
    'eld_tile_noise_sums_u16': (_i, [_vp, _i, _i, _i, _i, _i, _i, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int32), _i, _vp, _vp, _vp, _sz, _vp]),
    'eld_burst_stack_workspace_bytes': (_sz, [_i, _i, _i]),
    'eld_burst_stack_u16': (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int32), _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    'eld_burst_luma_pyramid_elems': (_sz, [_i, _i, _i, _i, _i]),
    'eld_burst_luma_pyramid_u16': (_i, [_vp, _i, _i, _i, _i, _i, _vp, _vp]),
    'eld_burst_align_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'eld_burst_align_u16': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    'eld_burst_stack_aligned_workspace_bytes': (_sz, [_i, _i, _i]),
    'eld_burst_stack_aligned_u16': (_i, [_vp, _i, _i, _i, _i, C.POINTER(C.c_int), _i, C.POINTER(C.c_int32), _i, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp,
                                         _vp, _vp, _sz, _vp]),
    'eld_quality_assess_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'eld_quality_assess': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _f, _vp]),
    'eld_quality_assess_images': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _i, _i, _f, _vp]),
    'eld_illuminance_correct_workspace_bytes': (_sz, [_i]),
    'eld_illuminance_correct': (_i, [_vp, _vp, _vp, _vp, _sz, _i, _i, _sz, _vp]),
    'eld_l1_workspace_bytes': (_sz, []),
    'eld_l1_loss': (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _f, _vp]),
    'eld_mse_loss': (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _f, _vp]),
    'eld_adam_step': (_i, [_vp, _vp, _vp, _vp, _sz, _d, _d, _d, _d, _d, _i, _d, _vp]),
    'eld_layer_workspace_bytes': (_sz, [_i, _i, _i, _i, _i]),
    'eld_conv3x3_forward': (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_conv3x3_backward_data': (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_conv3x3_backward_weight': (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_convt2x2_forward': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_convt2x2_backward_data': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_convt2x2_backward_weight': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_maxpool2x2_forward': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'eld_maxpool2x2_backward': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'eld_conv3x3_forward_bf16': (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_conv3x3_backward_data_bf16': (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_conv3x3_backward_weight_bf16': (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_convt2x2_forward_bf16': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_convt2x2_backward_data_bf16': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_convt2x2_backward_weight_bf16': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_maxpool2x2_forward_bf16': (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    'eld_maxpool2x2_backward_bf16': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    'eld_debug_last_conv_kernel': (C.c_char_p, []),
    'eld_debug_conv_kernel_count': (C.c_uint, [C.c_char_p]),
    'eld_debug_unet_region': (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i), C.POINTER(_i)]),
    'eld_debug_unet_grad_tap': (None, [_vp, _sz]),
    'eld_debug_unet_grad_tap_layout': (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(_sz), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    'eld_debug_unet_grad_tap_bytes': (_sz, [_i, _i, _i, _i, _i, _i]),
    'eld_debug_unet_codes': (_i, [_vp]),
    'eld_flat_sums_u16': (_i, [_vp, _sz, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'eld_flat_box_workspace_bytes': (_sz, [_i, _i]),
    'eld_flat_box_tile': (_i, [_i, C.POINTER(_i), C.POINTER(_i)]),
    'eld_flat_box_u32': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    'eld_flat_apply_u16': (_i, [_vp, _vp, _i, _i, _i, _vp, C.POINTER(C.c_float), _i, _i, _vp, _vp]),
    'eld_pack_raw_bayer_u16_flat': (_i, [_vp, _vp, _i, _i, _i, C.POINTER(C.c_int), C.POINTER(C.c_float), _f, _vp, _vp, _vp, _f, _vp, _vp]),
    'eld_pack_raw_xtrans_u16_flat': (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp, _vp, _vp, _f, _vp, _vp]),
    'eld_nlm_vst_f32': (_i, [_vp, _i, _i, _i, _i, _f, _vp, _i, _i, _i, C.POINTER(C.c_uint16), _i, _vp, _vp]),
    'eld_bm3d_vst_workspace_bytes': (_sz, [_i, _i, _i, _i]),
    'eld_bm3d_vst_f32': (_i, [_vp, _i, _i, _i, _i, _f, _vp, _vp, _i, _i, _i, _i, _u32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8), _i, _vp, _vp,
                              _sz, _vp]),
    'eld_dng_unpack_u16': (_i, [_vp, _sz, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp]),
    'eld_dng_ljpeg_u16': (_i, [_vp, _sz, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _vp, _sz, _i, _vp, _vp, _vp]),
    'eld_dng_enc_hist_u16': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    'eld_dng_enc_pack_u16': (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    'eld_dng_enc_ffcount_u8': (_i, [_vp, _sz, _vp, _i, _i, _vp, _vp]),
    'eld_dng_enc_stuff_u8': (_i, [_vp, _sz, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    'eld_dng_opcodes_apply_f32': (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp, _sz, _i, _vp]),
    'eld_dng_opcodes_gain_f32': (_i, [_vp, _i, _i, _vp, _i, _vp, _sz, _i, _vp]),
    'eld_warp_rgb_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _f, _vp, _vp, _i, _i, _vp]),
    'eld_jpeg_coef_u8': (_i, [_vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    'eld_jpeg_hist_i16': (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _sz, _vp]),
    'eld_jpeg_pack_i16': (_i, [_vp, _sz, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _i, _vp]),
    'eld_render_bayer_edge': (_i, [_vp, C.POINTER(C.c_int), _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp]),
    'eld_render_bayer_edge_tile': (_i, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'eld_render_xtrans_dir': (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _f, _vp, _vp, _i, _vp]),
    'eld_render_xtrans_dir_tile': (_i, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'eld_frame_rgb_f32': (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp, _f, _vp, _vp, _i,
                               _vp]),
    'eld_frame_rgb_tile': (_i, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
}


ABI_VERSION = 8         # ELD_ABI_VERSION of include/eld_amd.h this binding was written against
PHILOX_ROUNDS = 7      # the sampler's generator: Philox4x32-7 (csrc/philox.h); checked against the library at load


class LibraryMissing(RuntimeError):
    pass


_lib = None


def load_library(path=None):
    """Load libeld_amd.so and bind every prototype.  Fails loudly -- there is no fallback path."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise LibraryMissing(
            '%s not found: the HIP extension has not been built.  Run `python __graft_entry__.py` '
            '(hipcc --offload-arch=gfx950) first; eld_amd has no CPU fallback.' % p)
    # PyTorch-ROCm ships its own copy of the HIP runtime; device memory, streams and events are torch's, so libeld_amd must
    # bind to THAT runtime instance: import torch first (a libamdhip64 loaded by us before torch's is a second runtime with
    # no device context -- every launch then fails with hipErrorNoDevice).
    import torch  # noqa: F401
    lib_ = C.CDLL(p)
    any_philox = bool(os.environ.get('ELD_AMD_ANY_PHILOX'))
    lib_.eld_abi_version.restype = C.c_int
    if lib_.eld_abi_version() != ABI_VERSION and not any_philox:      # before binding: an older library fails here, not with a missing-symbol AttributeError
        raise RuntimeError('libeld_amd ABI version %d, this package binds version %d of include/eld_amd.h: rebuild with `python __graft_entry__.py`'
                           % (lib_.eld_abi_version(), ABI_VERSION))
    for name, (res, args) in SIGNATURES.items():
        if name == 'eld_philox_rounds' and any_philox and not hasattr(lib_, name):
            continue                      # dev A/B runs against a library older than the symbol (tools/build_variant.sh <old rev>)
        try:
            fn = getattr(lib_, name)
        except AttributeError:            # same ABI number, older build (eld_noise_forward_dark came without a new number)
            raise RuntimeError('%s does not export %s: it was built from older sources; rebuild with `python __graft_entry__.py`' % (p, name))
        fn.restype = res
        fn.argtypes = args
    if not any_philox and lib_.eld_philox_rounds() != PHILOX_ROUNDS:
        # the noise stream of a (seed, sample id) pair depends on the round count: a library built with another -DELD_PHILOX_ROUNDS replays
        # different noise for the same checkpoint / seed ("noise streams")
        raise RuntimeError('libeld_amd runs Philox4x32-%d, this package expects %d rounds (set ELD_AMD_ANY_PHILOX=1 to accept)'
                           % (lib_.eld_philox_rounds(), PHILOX_ROUNDS))
    _lib = lib_
    return lib_


def lib():
    return load_library()


def build_src_hash():
    """The source hash compiled into the loaded library (eld_build_info: "... src=<16 hex digits>"; "unknown" for builds that did not pass one)."""
    info = lib().eld_build_info().decode()
    return info.rsplit('src=', 1)[1].strip() if 'src=' in info else 'unknown'


class EldError(RuntimeError):
    pass


def check(rc, what=''):
    if rc != 0:
        msg = lib().eld_error_string(int(rc)).decode()
        raise EldError('%s failed: %s (code %d)' % (what or 'libeld_amd call', msg, rc))


def dptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def cur_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
