"""ctypes binding of libdanhip.so (the C ABI declared in include/danhip.h).

The product path has NO fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# 16-bit activation type of this process: DANHIP_DTYPE=bf16 (default) | fp16 selects the library build (include/danhip.h)
ACT_NAME = os.environ.get("DANHIP_DTYPE", "bf16").lower()
if ACT_NAME not in ("bf16", "fp16"):
    raise ValueError("DANHIP_DTYPE must be bf16 or fp16, got %r" % ACT_NAME)
ACT_DTYPE = torch.float16 if ACT_NAME == "fp16" else torch.bfloat16
SO_PATH = os.path.join(_HERE, "libdanhip_f16.so" if ACT_NAME == "fp16" else "libdanhip.so")
if os.environ.get("DANHIP_LIB_PATH"):          # diagnosis: A/B another in-tree build of the same library (tools/build_one.sh variants)
    SO_PATH = os.path.abspath(os.environ["DANHIP_LIB_PATH"])

F32, BF16 = 0, 1      # BF16 = "the build's 16-bit activation type" in out_dtype arguments
SPLIT3 = 3            # fp16 build, forward convolutions: the [hi | lo | hi] half-limb layout of csrc/split_infer.hip


# ---- struct mirrors: field for field the typedefs of include/danhip.h (tests/test_abi_header_cpu.py compares them with the header)
class ConvDesc(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("N", "H", "W", "Cin", "Ho", "Wo", "Cout", "kh", "kw", "stride")]


class ConvPitch(ctypes.Structure):
    """danhip_conv_pitch: pixel pitches (elements) of a call's input / output operand and of a data gradient's mask (channel-slice views)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("x_pitch", "y_pitch", "aux_pitch")]


class PackEntry(ctypes.Structure):
    _fields_ = [("w_hwio", ctypes.c_void_p), ("wf_packed", ctypes.c_void_p), ("wb_packed", ctypes.c_void_p)] + \
               [(n, ctypes.c_int32) for n in ("kh", "kw", "cin", "cin_real", "cout", "rows_f", "cols_f", "rows_b", "cols_b", "co8", "first_block", "pad_")]


HEADS_MAX_LEVELS = 8


class HeadLevel(ctypes.Structure):
    """danhip_head_level: one pyramid level of danhip_heads_split_fwd / danhip_heads_grad_pad."""
    _fields_ = [("h", ctypes.c_void_p), ("dy", ctypes.c_void_p)] + [(n, ctypes.c_int32) for n in ("HW", "Ch", "nneg", "npos", "off", "co_pad")]


class JpegInfo(ctypes.Structure):
    """danhip_jpeg_info"""
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "ncomp", "mode", "reason", "reserved")] + [("coef_count", ctypes.c_int64)]


class JpegDesc(ctypes.Structure):
    """danhip_jpeg_desc: one image of a decode batch (filled by danhip_jpeg_entropy_decode_batch, read by the two device launches)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "ncomp", "mode")] + \
               [(n, ctypes.c_int32 * 3) for n in ("blocks_w", "blocks_h", "comp_w", "comp_h", "quant_index")] + \
               [(n, ctypes.c_int32) for n in ("status", "idct_groups", "rgb_groups")] + [("reserved", ctypes.c_int32 * 2)] + \
               [("coef_offset", ctypes.c_int64), ("coef_count", ctypes.c_int64), ("plane_offset", ctypes.c_int64 * 3),
                ("out_offset", ctypes.c_int64), ("quant", (ctypes.c_uint16 * 64) * 4)]


class ResizeItem(ctypes.Structure):
    """danhip_resize_item: one resized / mirrored copy of danhip_resize_u8_linear_batch (filled by danhip_resize_item_init)."""
    _fields_ = [("src_offset", ctypes.c_int64), ("dst_offset", ctypes.c_int64)] + \
               [(n, ctypes.c_int32) for n in ("H", "W", "pitch", "Ho", "Wo", "mirror", "first_tile", "tiles")] + \
               [(n, ctypes.c_double) for n in ("fx", "fy", "scale_x", "scale_y")]


class CrcSegment(ctypes.Structure):
    """danhip_crc_segment: one device byte range of danhip_crc32c_batch."""
    _fields_ = [("ptr", ctypes.c_void_p), ("bytes", ctypes.c_uint64)]


class JpegEncDesc(ctypes.Structure):
    """danhip_jpeg_enc_desc: one image of an encode batch (filled by danhip_jpeg_encode_prepare)."""
    _fields_ = [("src", ctypes.c_void_p)] + [(n, ctypes.c_int32) for n in ("width", "height", "mode", "quality")] + \
               [(n, ctypes.c_int32 * 3) for n in ("blocks_w", "blocks_h", "comp_w", "comp_h")] + \
               [(n, ctypes.c_int32) for n in ("real_bw", "real_bh", "color_groups", "fdct_groups")] + \
               [("coef_offset", ctypes.c_int64), ("coef_count", ctypes.c_int64), ("plane_offset", ctypes.c_int64 * 3),
                ("file_offset", ctypes.c_int64), ("file_capacity", ctypes.c_int64),
                ("recip", (ctypes.c_uint16 * 64) * 2), ("corr", (ctypes.c_uint16 * 64) * 2),
                ("shift", (ctypes.c_uint8 * 64) * 2), ("qtable", (ctypes.c_uint8 * 64) * 2)]


class DrawItem(ctypes.Structure):
    """danhip_draw_item: one image of danhip_draw_boxes_u8."""
    _fields_ = [("image", ctypes.c_void_p)] + [(n, ctypes.c_int32) for n in ("width", "height", "first_box", "num_boxes", "groups", "reserved")]


DETECT_SELECT_LAUNCHES = 7     # DANHIP_DETECT_SELECT_LAUNCHES
CRC32C_BATCH_LAUNCHES = 3      # DANHIP_CRC32C_BATCH_LAUNCHES
JPEG_ENCODE_LAUNCHES = 2       # DANHIP_JPEG_ENCODE_LAUNCHES
JPEG_ENCODE_ENTROPY_LAUNCHES = 6   # DANHIP_JPEG_ENCODE_ENTROPY_LAUNCHES
JPEG_ENCODE_OPTIMIZE_LAUNCHES = 3  # DANHIP_JPEG_ENCODE_OPTIMIZE_LAUNCHES
JPEG_ENC_OPTIMIZE = 1              # DANHIP_JPEG_ENC_OPTIMIZE
JPEG_HOSTONLY = -1             # DANHIP_JPEG_HOSTONLY

P = ctypes.c_void_p
I32 = ctypes.c_int32
I64 = ctypes.c_int64
FL = ctypes.c_float
DESC = ctypes.POINTER(ConvDesc)
INT = ctypes.c_int
U32 = ctypes.c_uint32
U64 = ctypes.c_uint64
DBL = ctypes.c_double
SZ = ctypes.c_size_t
STR = ctypes.c_char_p
PI32 = ctypes.POINTER(I32)
PFL = ctypes.POINTER(FL)
PITCH = ctypes.POINTER(ConvPitch)
LEVELS = ctypes.POINTER(HeadLevel)
JINFO = ctypes.POINTER(JpegInfo)
STATUS = "status"     # return class of the table below: an int that is 0 or a negative DANHIP_E* code (bound as INT, listed in SIGNATURES)

# name -> (return type, argtypes): ONE line per function include/danhip.h declares, in the header's order.  tests/test_abi_header_cpu.py
# parses the header and holds every return type, parameter and struct field here to it.
_TABLE = {
    # ---- library state
    "danhip_last_error": (STR, []),
    "danhip_version": (INT, []),
    "danhip_set_option": (STATUS, [STR, INT]),
    "danhip_get_option": (INT, [STR]),
    "danhip_act_dtype": (INT, []),
    # ---- deterministic mode
    "danhip_deform_sample_bwd_ordered_workspace_bytes": (SZ, [I32] * 5),
    "danhip_deform_conv_bwd_ordered_workspace_bytes": (SZ, [I32] * 9),
    "danhip_deform_far_ordered": (STATUS, [P, P, I32, I32, I32, I32, I32, I32, P, SZ, P]),
    "danhip_deform_far_ordered_emulate": (STATUS, [P, P, P, I64, I32, I32, I32, I32, I32, I32, P, P]),
    "danhip_ordered_reduce_f32": (STATUS, [P, I32, I64, P, INT, P]),
    "danhip_reduce_workspace_bytes": (SZ, [I64, I32]),
    "danhip_loss_workspace_bytes": (SZ, []),
    "danhip_sgd_workspace_bytes": (SZ, []),
    # ---- dense convolution
    "danhip_conv_packed_dims": (STATUS, [DESC, INT, ctypes.POINTER(I64), ctypes.POINTER(I64)]),
    "danhip_pack_conv_weight": (STATUS, [DESC, P, I32, P, P, P]),
    "danhip_pack_entry_init": (STATUS, [ctypes.POINTER(PackEntry), DESC, P, I32, P, P, I32, PI32]),
    "danhip_pack_conv_weights_batched": (STATUS, [P, I32, I32, P]),
    "danhip_conv2d_fwd": (STATUS, [DESC, P, P, P, P, INT, INT, P, P]),
    "danhip_conv2d_fwd_pool": (STATUS, [DESC, P, P, P, P, P, P]),
    "danhip_conv2d_fwd_pool_arg": (STATUS, [DESC, P, P, P, P, P, P, P]),
    "danhip_conv2d_fwd_relu_bits_arg": (STATUS, [DESC, P, P, P, P, P, P, P, P, P]),
    "danhip_conv2d_fwd_pool_only": (INT, [DESC]),                       # 0 / 1
    "danhip_conv2d_bwd_data": (STATUS, [DESC, P, P, P, P, INT, P]),
    "danhip_conv2d_workspace_bytes": (SZ, [DESC, INT]),
    "danhip_conv2d_fwd_ws": (STATUS, [DESC, P, P, P, P, INT, INT, P, P, SZ, P]),
    "danhip_conv2d_bwd_data_ws": (STATUS, [DESC, P, P, P, P, INT, P, SZ, P]),
    "danhip_relu_bits": (STATUS, [P, P, I64, I32, P]),
    "danhip_conv2d_fwd_emits_bits": (INT, [DESC, INT]),                 # 0 / 1
    "danhip_conv2d_fwd_relu_bits": (STATUS, [DESC, P, P, P, P, P, P, P, P]),
    "danhip_conv2d_bwd_data_takes_bits": (INT, [DESC]),                 # 0 / 1
    "danhip_conv2d_bwd_data_first_supported": (INT, [DESC]),            # 0 / 1
    "danhip_conv2d_bwd_data_bits_first": (STATUS, [DESC, P, P, P, P, I32, P, P, P]),
    "danhip_conv2d_bwd_data_bits": (STATUS, [DESC, P, P, P, P, INT, P]),
    "danhip_conv2d_fwd_concat2_supported": (INT, [DESC, I32, I32]),     # 0 / 1
    "danhip_conv2d_fwd_concat2": (STATUS, [DESC, P, P, I32, I32, P, P, P, INT, P]),
    "danhip_conv2d_fwd_strided": (STATUS, [DESC, P, P, P, P, INT, I32, PITCH, P, SZ, P]),
    "danhip_conv2d_bwd_data_strided": (STATUS, [DESC, P, P, P, P, INT, PITCH, P, SZ, P]),
    "danhip_conv2d_bwd_weight_strided": (STATUS, [DESC, P, P, P, P, I32, PITCH, P, SZ, P]),
    "danhip_conv2d_bwd_weight": (STATUS, [DESC, P, P, P, P, I32, P]),
    "danhip_conv2d_bwd_weight_workspace_bytes": (SZ, [DESC]),
    "danhip_conv2d_bwd_weight_ws": (STATUS, [DESC, P, P, P, P, I32, P, SZ, P]),
    "danhip_relu_bwd_bias_grad": (STATUS, [P, P, P, I64, I32, P]),
    "danhip_relu_bwd_bias_grad_ws": (STATUS, [P, P, P, I64, I32, P, SZ, P]),
    "danhip_conv_kernel_label": (STR, [DESC, INT]),
    "danhip_conv_wgrad_kernel_label": (STR, [DESC]),
    "danhip_conv_last_launch_label": (STR, []),
    # ---- HBM-bound layer kernels
    "danhip_maxpool2x2_fwd": (STATUS, [P, P, I32, I32, I32, I32, P]),
    "danhip_maxpool2x2_bwd": (STATUS, [P, P, P, I32, I32, I32, I32, INT, P]),
    "danhip_maxpool2x2_fwd_arg": (STATUS, [P, P, P, I32, I32, I32, I32, P]),
    "danhip_maxpool2x2_bwd_arg": (STATUS, [P, P, P, I32, I32, I32, I32, INT, P]),
    "danhip_l2norm_fwd": (STATUS, [P, P, P, I64, I32, P]),
    "danhip_l2norm_bwd": (STATUS, [P, P, P, P, P, I64, I32, INT, INT, P]),
    "danhip_l2norm_bwd_ws": (STATUS, [P, P, P, P, P, I64, I32, INT, INT, P, SZ, P]),
    "danhip_l2norm_bwd_pool_scatter": (STATUS, [P, P, P, P, P, P, P, I32, I32, I32, I32, INT, INT, INT, P]),
    "danhip_l2norm_bwd_pool_scatter_ws": (STATUS, [P, P, P, P, P, P, P, I32, I32, I32, I32, INT, INT, INT, P, SZ, P]),
    "danhip_resize_bilinear_add_fwd": (STATUS, [P, P, P, I32, I32, I32, I32, I32, I32, P]),
    "danhip_resize_bilinear_add_bwd": (STATUS, [P, P, I32, I32, I32, I32, I32, I32, INT, P]),
    "danhip_avgpool2x2s1_same_fwd": (STATUS, [P, P, I32, I32, I32, I32, P]),
    "danhip_avgpool2x2s1_same_bwd": (STATUS, [P, P, P, I32, I32, I32, I32, INT, P]),
    "danhip_add16": (STATUS, [P, P, P, I64, P]),
    "danhip_residual_bwd": (STATUS, [P, P, P, P, P, INT, I64, P]),
    "danhip_avgpool2x2s1_same_fwd_strided": (STATUS, [P, I32, P, I32, I32, I32, I32, I32, INT, P]),
    "danhip_avgpool2x2s1_same_bwd_strided": (STATUS, [P, I32, P, I32, I32, I32, I32, I32, P]),
    "danhip_slice_deliver": (STATUS, [P, I32, I32, I32, P, I32, P, I32, INT, I64, P]),
    "danhip_batchnorm_fwd_train": (STATUS, [P, P, P, P, P, P, P, P, I64, I32, FL, FL, INT, P, P]),
    "danhip_batchnorm_fwd_infer": (STATUS, [P, P, P, P, P, P, I64, I32, INT, P]),
    "danhip_batchnorm_bwd": (STATUS, [P, P, P, P, P, P, P, P, I64, I32, P]),
    "danhip_preprocess_u8": (STATUS, [P, P, I64, P]),
    "danhip_cast_pad_f32_to_bf16": (STATUS, [P, P, P, I64, I32, I32, P]),
    # ---- detection heads, hard-negative mining, losses, optimizer
    "danhip_head_split_fwd": (STATUS, [P, P, P, I32, I32, I32, I32, I32, I32, I32, P]),
    "danhip_head_split_bwd": (STATUS, [P, P, P, P, I32, I32, I32, I32, I32, I32, I32, P]),
    "danhip_heads_split_fwd": (STATUS, [LEVELS, I32, P, P, I32, I32, P]),
    "danhip_heads_grad_pad": (STATUS, [LEVELS, I32, P, P, I32, I32, P]),
    "danhip_hard_neg_select": (STATUS, [P, P, P, P, P, P, I32, I32, FL, INT, P]),
    "danhip_detection_loss_fwd": (STATUS, [P, P, P, P, P, P, P, P, I32, I32, P]),
    "danhip_detection_loss_fwd_ws": (STATUS, [P, P, P, P, P, P, P, P, I32, I32, P, SZ, P]),
    "danhip_detection_loss_bwd": (STATUS, [P, P, P, P, P, P, P, FL, FL, I32, I32, P]),
    "danhip_cls_accuracy": (STATUS, [P, P, P, P, I32, I32, P]),
    "danhip_sgd_momentum_flat": (STATUS, [P, P, P, P, P, P, I32, I64, FL, FL, FL, P, P]),
    "danhip_sgd_momentum_flat_ws": (STATUS, [P, P, P, P, P, P, I32, I64, FL, FL, FL, P, P, SZ, P]),
    "danhip_sgd_momentum_flat_dynamic": (STATUS, [P, P, P, P, P, P, I32, I64, FL, FL, P, P, P]),
    # ---- anchors and boxes
    "danhip_anchors_generate": (STATUS, [P, P, P, P, P, P, I32, I32, I32, FL, FL, FL, I32, P]),
    "danhip_iou_matrix": (STATUS, [P, P, P, P, P, P, P, I32, I32, P]),
    "danhip_match_workspace_bytes": (SZ, [I32, I32]),
    "danhip_dual_max_match": (STATUS, [P, I32, I32, FL, FL, INT, P, P, P, SZ, P]),
    "danhip_small_mining_match": (STATUS, [P, I32, I32, FL, FL, FL, I32, FL, P, P, P, SZ, P]),
    "danhip_encode_anchors": (STATUS, [P, P, P, P, P, P, P, P, P, I32, FL, FL, FL, FL, FL, P]),
    "danhip_encode_anchors_batched_workspace_bytes": (SZ, [I32, I32, I32]),
    "danhip_encode_anchors_batched": (STATUS, [P] * 11 + [I32, I32, I32, I32, I32, FL, FL, FL, I32, FL, FL, FL, FL, FL, FL, P, P, P, P, P, SZ, P]),
    "danhip_decode_anchors": (STATUS, [P, P, P, P, P, P, I32, I32, FL, FL, FL, FL, P]),
    "danhip_face_scores": (STATUS, [P, P, P, FL, I64, P]),
    # ---- deformable convolution
    "danhip_deform_sample_fwd": (STATUS, [P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, P]),
    "danhip_deform_sample_bwd_workspace_bytes": (SZ, [I32, I32, I32, I32]),
    "danhip_deform_sample_bwd": (STATUS, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, INT, P, SZ, P]),
    "danhip_deform_conv_workspace_bytes": (SZ, [I32, I32, I32, I32, I32, I32, I32, INT]),
    "danhip_deform_conv_fused": (INT, [I32] * 9),                       # 0 / 1
    "danhip_deform_conv_fwd": (STATUS, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, INT, P, SZ, P]),
    "danhip_deform_conv_bwd": (STATUS, [P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, INT, P, SZ, P]),
    "danhip_deform_conv_bwd_with_col": (STATUS, [P, P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, INT, P, SZ, P]),
    "danhip_deform_conv_bwd_deliver": (STATUS, [P, P, P, P, P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, INT, INT, P, SZ, P]),
    # ---- anchor routing, NMS, arg-sort, PS-ROI pooling, the 3x3 pool
    "danhip_routing_workspace_bytes": (SZ, [I64, I32, INT]),
    "danhip_dynamic_anchor_routing_eval": (STATUS, [P, P, P, P, I64, I32, I32, I32, I32, I32, P, P, P, SZ, P]),
    "danhip_dynamic_anchor_routing_train": (STATUS, [P, P, P, P, I64, I32, I32, I32, I32, I32, FL, FL, U64, U64, P, P, P, P, SZ, P]),
    "danhip_nms": (STATUS, [P, I32, I32, I32, FL, P, P, P]),
    "danhip_argsort_workspace_bytes": (SZ, [I64]),
    "danhip_argsort_desc_f32": (STATUS, [P, I64, I32, P, P, SZ, P]),
    "danhip_deform_psroi_pool_fwd": (STATUS, [P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, FL, FL, I32, I32, P]),
    "danhip_deform_psroi_pool_bwd": (STATUS, [P, P, P, P, P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, I32, FL, FL, I32, I32, P]),
    "danhip_maxpool3x3s2_same_fwd": (STATUS, [P, P, I32, I32, I32, I32, P]),
    "danhip_maxpool3x3s2_same_bwd": (STATUS, [P, P, P, I32, I32, I32, I32, P]),
    # ---- test-time pipeline
    "danhip_resize_u8_linear": (STATUS, [P, I32, I32, P, I32, I32, I32, DBL, DBL, P]),
    "danhip_bbox_vote_workspace_bytes": (SZ, [I32, I32]),
    "danhip_bbox_vote": (STATUS, [P, P, I32, I32, DBL, I32, P, P, P, SZ, P]),
    # ---- WIDER FACE evaluation
    "danhip_wider_quantize": (STATUS, [P, INT, P, P, I32, I32, I32, P, P, I32, I32, P, P]),
    "danhip_wider_score_range_workspace_bytes": (SZ, []),
    "danhip_wider_score_range": (STATUS, [P, I64, P, P, SZ, P]),
    "danhip_wider_eval_workspace_bytes": (SZ, [I32, I32, I32]),
    "danhip_wider_eval": (STATUS, [P, P, I64, P, P, P, I64, P, I32, I32, I32, I32, DBL, P, SZ, P, P]),
    "danhip_wider_ap": (STATUS, [P, SZ, P, I64, I32, I32, I32, P, P, P, P, P, P]),
    # ---- training input pipeline
    "danhip_augment_workspace_bytes": (SZ, []),
    "danhip_augment_preprocess": (STATUS, [P, I32, I32, I32, PI32, PFL, I32, I32, I32, I32, I32, P, I32, I32, P, SZ, P]),
    "danhip_augment_item_bytes": (SZ, []),
    "danhip_augment_item_init": (STATUS, [P, P, I32, I32, I32, PI32, PFL, I32, I32, I32, I32, I32, I32, PI32]),
    "danhip_augment_batch_workspace_bytes": (SZ, [I32]),
    "danhip_augment_preprocess_batch": (STATUS, [P, I32, I32, P, I32, I32, P, SZ, P]),
    # ---- test-time pipeline for images of different sizes
    "danhip_resize_item_bytes": (SZ, []),
    "danhip_resize_item_init": (STATUS, [P, I64, I32, I32, I32, I64, I32, I32, DBL, DBL, I32, I32, PI32]),
    "danhip_resize_u8_linear_batch": (STATUS, [P, P, I32, P, I64, P, I64, P]),
    "danhip_detect_select_workspace_bytes": (SZ, [I64]),
    "danhip_detect_select": (STATUS, [P, P, I32, I32, FL, I32, FL, P, P, P, SZ, PI32, P]),
    # ---- JPEG decode: host entropy stage and the two device launches
    "danhip_jpeg_inspect": (INT, [P, I64, JINFO]),                      # a reason code (>= 0), not a status
    "danhip_jpeg_entropy_decode_batch": (STATUS, [P, P, I32, I32, P, I64, P, P]),
    "danhip_jpeg_workspace_bytes": (SZ, [P, I32]),
    "danhip_jpeg_output_bytes": (I64, [P, I32]),
    "danhip_jpeg_reconstruct_batch": (STATUS, [P, I64, P, P, I32, P, I64, P, SZ, P, P]),
    # ---- JPEG decode: Huffman stage on the device
    "danhip_jpeg_scan_staging_bytes": (SZ, [P, P, I32]),
    "danhip_jpeg_scan_prepare_batch": (STATUS, [P, P, I32, P, SZ, I64, P, P]),
    "danhip_jpeg_scan_device_bytes": (SZ, [P]),
    "danhip_jpeg_scan_workspace_bytes": (SZ, [P]),
    "danhip_jpeg_huffman_decode_batch": (STATUS, [P, P, SZ, I32, P, I64, P, P, P, SZ, P, P, P]),
    "danhip_jpeg_entropy_emulate_batch": (STATUS, [P, SZ, I32, P, P, I64, I32, P, P]),
    # ---- JPEG decode: progressive streams
    "danhip_jpeg_inspect_ex": (INT, [P, I64, U32, JINFO]),              # a reason code likewise (DANHIP_EINVAL for unknown flag bits)
    "danhip_jpeg_entropy_decode_batch_ex": (STATUS, [P, P, I32, I32, U32, P, I64, P, P]),
    "danhip_jpeg_scan_prepare_batch_ex": (STATUS, [P, P, I32, U32, P, SZ, I64, P, P]),
    # ---- data-parallel gradient exchange
    "danhip_comm_load": (STATUS, [STR]),
    "danhip_comm_rccl_version": (STATUS, [ctypes.POINTER(INT)]),
    "danhip_comm_unique_id": (STATUS, [P]),
    "danhip_comm_create": (STATUS, [P, I32, I32, I32, ctypes.POINTER(P)]),
    "danhip_comm_destroy": (STATUS, [P]),
    "danhip_comm_info": (STATUS, [P, PI32, PI32, PI32]),
    "danhip_comm_async_error": (STATUS, [P, PI32]),
    "danhip_comm_abort": (STATUS, [P]),
    "danhip_comm_allreduce_sum": (STATUS, [P, P, I64, INT, P]),
    "danhip_comm_reduce_scatter_sum": (STATUS, [P, P, P, I64, INT, P]),
    "danhip_comm_allgather": (STATUS, [P, P, P, I64, INT, P]),
    # ---- split-operand inference
    "danhip_split_set_range_flag": (STATUS, [P]),
    "danhip_split3_f32": (STATUS, [P, P, I64, I32, I32, INT, I32, P]),
    "danhip_unsplit3_f32": (STATUS, [P, P, I64, I32, I32, P]),
    "danhip_unsplit3_scaled_f32": (STATUS, [P, P, I64, I32, I32, I32, P]),
    "danhip_maxpool2x2_split3": (STATUS, [P, P, I32, I32, I32, I32, P]),
    "danhip_l2norm_split3": (STATUS, [P, P, P, I64, I32, I32, I32, P]),
    "danhip_conv3x3_c3_f32_split3": (STATUS, [P, P, P, P, I32, I32, I32, I32, INT, I32, P]),
    "danhip_conv2d_fwd_split": (STATUS, [DESC, P, P, P, P, INT, INT, I32, P, SZ, P]),
    # ---- fp32 inference path
    "danhip_conv2d_fwd_f32": (STATUS, [DESC, P, P, P, P, INT, P, P]),
    "danhip_maxpool2x2_fwd_f32": (STATUS, [P, P, I32, I32, I32, I32, P]),
    "danhip_l2norm_fwd_f32": (STATUS, [P, P, P, I64, I32, P]),
    "danhip_resize_bilinear_add_fwd_f32": (STATUS, [P, P, P, I32, I32, I32, I32, I32, I32, P]),
    "danhip_avgpool2x2s1_same_fwd_f32": (STATUS, [P, P, I32, I32, I32, I32, P]),
    "danhip_deform_sample_fwd_f32": (STATUS, [P, P, P, I32, I32, I32, I32, I32, I32, I32, I32, I32, P]),
    # ---- CRC-32C (the three host functions make no GPU call)
    "danhip_crc32c_host": (U32, [P, SZ, U32]),
    "danhip_crc32c_host_form": (U32, [P, SZ, U32, I32]),
    "danhip_crc32c_combine": (U32, [U32, U32, U64]),
    "danhip_crc_segment_bytes": (SZ, []),
    "danhip_crc32c_chunk_bytes": (I32, []),
    "danhip_crc32c_group_bytes": (I32, []),
    "danhip_crc32c_batch_last_launches": (I32, []),
    "danhip_crc32c_batch_workspace_bytes": (SZ, [I32, U64]),
    "danhip_crc32c_batch": (STATUS, [P, I32, P, I32, P, SZ, P]),
    # ---- JPEG encode (csrc/jpeg_encode.cpp: all but danhip_jpeg_encode_pixels_batch make no GPU call)
    "danhip_jpeg_enc_desc_bytes": (SZ, []),
    "danhip_jpeg_encode_file_bound": (I64, [I32, I32, I32]),
    "danhip_jpeg_encode_prepare": (STATUS, [P, P, P, I32, I32, I32, P, P]),
    "danhip_jpeg_encode_pixels_batch": (STATUS, [P, P, I32, P, I64, P, SZ, P, P]),
    "danhip_jpeg_encode_pixels_host": (STATUS, [P, I32, P, I64]),
    "danhip_jpeg_encode_entropy_batch": (STATUS, [P, I64, P, I32, I32, P, I64, P]),
    "danhip_jpeg_encode_host": (STATUS, [P, I32, I32, I32, I32, P, I64, P]),
    # ---- JPEG encode: Huffman stage on the device
    "danhip_jpeg_encode_scan_staging_bytes": (SZ, [I32]),
    "danhip_jpeg_encode_scan_prepare": (STATUS, [P, I32, I64, I64, P, SZ, P]),
    "danhip_jpeg_encode_scan_workspace_bytes": (SZ, [P]),
    "danhip_jpeg_encode_huffman_batch": (STATUS, [P, P, SZ, P, I32, P, I64, P, I64, P, P, P, SZ, P, P]),
    "danhip_jpeg_encode_entropy_emulate_batch": (STATUS, [P, SZ, P, I32, P, I64, P, I64, P, P, P]),
    # ---- JPEG encode, optimize=True (csrc/jpeg_encode.cpp; the launch in csrc/jpeg_encode_huffman_exact.hip)
    "danhip_jpeg_optimal_table_host": (STATUS, [P, P, P]),
    "danhip_jpeg_encode_entropy_batch_ex": (STATUS, [P, I64, P, I32, I32, I32, P, I64, P]),
    "danhip_jpeg_encode_scan_prepare_ex": (STATUS, [P, I32, I64, I64, I32, P, SZ, P]),
    "danhip_jpeg_encode_optimize_layout": (INT, [P]),
    "danhip_jpeg_optimal_tables_device": (STATUS, [P, I32, P]),
    # ---- box drawing
    "danhip_draw_item_bytes": (SZ, []),
    "danhip_draw_boxes_u8": (STATUS, [P, P, I32, P, P, I64, I32, P]),
    "danhip_draw_boxes_labels_u8": (STATUS, [P, P, I32, P, P, P, I64, I32, P]),
    "danhip_draw_glyph": (STATUS, [I32, P]),
    "danhip_draw_format_score": (STATUS, [FL, P]),
    # ---- transposed convolution 4x4 / stride 2 (the LFPN's learnable upsampling)
    "danhip_conv_transpose4x4s2_pack_weight": (STATUS, [P, P, P, I32, I32, P]),
    "danhip_conv_transpose4x4s2_add_fwd": (STATUS, [P, P, P, P, P] + [I32] * 7 + [P]),
    "danhip_conv_transpose4x4s2_dgrad": (STATUS, [P, P, P] + [I32] * 7 + [INT, P]),
    "danhip_conv_transpose4x4s2_wgrad_workspace_bytes": (SZ, [I32] * 7),
    "danhip_conv_transpose4x4s2_wgrad_slabs": (I32, [I32] * 7),
    "danhip_conv_transpose4x4s2_wgrad": (STATUS, [P, P, P, P] + [I32] * 7 + [P, SZ, P]),
    "danhip_conv_transpose4x4s2_add_fwd_f32": (STATUS, [P, P, P, P, P] + [I32] * 7 + [P]),
    # ---- fused batch-norm tails (batch norm + residual add + ReLU)
    "danhip_bn_act_fwd_train": (STATUS, [P, P, P, P, P, P, P, P, P, I64, I32, FL, FL, INT, P, P]),
    "danhip_bn_act_fwd_infer": (STATUS, [P, P, P, P, P, P, P, I64, I32, INT, P]),
    "danhip_bn_act_bwd": (STATUS, [P, P, P, P, P, P, P, P, P, P, I64, I32, INT, P]),
    # ---- face chips
    "danhip_face_chips_workspace": (STATUS, [I32, I32, ctypes.POINTER(SZ)]),
    "danhip_face_chips_u8": (STATUS, [P, P, I32, P, I64, P, P, I32, I32, I32, I32, FL, P, P, P, I32, P, SZ, P]),
    "danhip_face_chips_ex_workspace": (STATUS, [I32, I32, I32, I32, ctypes.POINTER(SZ)]),
    "danhip_face_chips_u8_ex": (STATUS, [P, P, I32, P, I64, P, P, I32, I32, I32, I32, FL, P, P, P, I32, P, SZ, P, I32, I32, P]),   # + filter, pad, fill_rgb
    # ---- face redaction (the last six make no GPU call: csrc/redact_walk.h's index arithmetic)
    "danhip_redact_workspace": (STATUS, [I32, I32, ctypes.POINTER(SZ)]),
    "danhip_redact_u8": (STATUS, [P, P, I32, P, I64, P, P, I32, I32, I32, I32, I32, FL, P, P, P, P, I64, P, P, SZ, P]),
    "danhip_redact_extent": (INT, [I32, I32, I32]),                     # e (>= 1), or DANHIP_EINVAL
    "danhip_redact_item_count": (I64, [I32, P, I32, I32, I32]),         # -1 for arguments outside the rule
    "danhip_redact_tile": (STATUS, [I32, I32, P, I32, I32, I32, I64, P]),
    "danhip_redact_window": (STATUS, [I32, I32, I32, I32, I32, P]),
    "danhip_redact_cell": (STATUS, [P, I32, I64, P]),
    "danhip_redact_in_shape": (INT, [I32, P, I32, I32]),                # 1 / 0, or DANHIP_EINVAL
}
PROTOTYPES = {name: (INT if res is STATUS else res, args) for name, (res, args) in _TABLE.items()}
SIGNATURES = {name: args for name, (res, args) in _TABLE.items() if res is STATUS}      # the calls `call` / `check` are for


def bind(handle, names=None):
    """Sets restype and argtypes from PROTOTYPES on a ctypes.CDLL handle: of every function, or of `names` alone (a handle of the other
    build, a stand-in library, another commit's build)."""
    for name in PROTOTYPES if names is None else names:
        fn = getattr(handle, name)          # AttributeError if the export is missing
        fn.restype, fn.argtypes = PROTOTYPES[name]
    return handle


_lib = None


class DanhipError(RuntimeError):
    pass


def lib():
    """Loads libdanhip.so; raises loudly when it is missing (no CPU / eager fallback exists)."""
    global _lib
    if _lib is None:
        _lib = _load(SO_PATH, ACT_NAME)
    return _lib


_lib_f16 = None


def lib_f16():
    """The fp16 build (libdanhip_f16.so) whatever DANHIP_DTYPE says: the split-operand evaluation path (csrc/split_infer.hip) runs its
    three-limb-product convolutions on v_mfma_f32_16x16x32_f16 also inside a bf16 process.  The two libraries share nothing (separate
    option tables, error strings, RCCL binding); this one is used for forward convolutions and weight packing only."""
    global _lib_f16
    if _lib_f16 is None:
        _lib_f16 = lib() if ACT_NAME == "fp16" else _load(os.path.join(_HERE, "libdanhip_f16.so"), "fp16")
    return _lib_f16


def call_f16(name, *args):
    L = lib_f16()
    rc = getattr(L, name)(*args)
    if rc != 0:
        raise DanhipError("%s (fp16 build) failed (%d): %s" % (name, rc, L.danhip_last_error().decode()))


def _load(so_path, act_name):
    if not os.path.exists(so_path):
        raise DanhipError("libdanhip.so not found at %s — run `python -m dan_amd.build` (there is no fallback path)" % so_path)
    L = bind(ctypes.CDLL(so_path))
    if L.danhip_act_dtype() != (2 if act_name == "fp16" else 1):
        raise DanhipError("%s was built for another activation dtype than %s" % (so_path, act_name))
    return L


def check(rc, what):
    if rc != 0:
        raise DanhipError("%s failed (%d): %s" % (what, rc, lib().danhip_last_error().decode()))


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    if t is None:
        return None
    assert t.is_contiguous(), "danhip needs contiguous tensors"
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(name, *args):
    check(getattr(lib(), name)(*args), name)
