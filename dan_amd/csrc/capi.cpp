// Error plumbing of the C ABI: thread-local message, never throws.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>

#include <hip/hip_runtime.h>

#include "../../include/danhip.h"

static thread_local char g_err[512] = "";

void danhip_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char* danhip_last_error(void) { return g_err; }
extern "C" int danhip_version(void) { return 24; }   // 2: danhip_deform_sample_bwd takes workspace_bytes; 3: danhip_comm_* (RCCL called directly); 4: danhip_comm_async_error / danhip_comm_abort; 5: danhip_wider_* (WIDER FACE AP); 6: danhip_jpeg_* (baseline JPEG decode); 7: danhip_jpeg_scan_* / danhip_jpeg_huffman_decode_batch (Huffman stage on the device); 8: danhip_jpeg_*_ex (opt-in progressive streams on the host entropy stage); 9: danhip_heads_split_fwd / danhip_heads_grad_pad (all head levels in one launch); 10: option "deterministic", danhip_ordered_reduce_f32, danhip_reduce_workspace_bytes and the _ws forms of the L2-norm / bias-gradient / loss / optimizer entry points; 11: danhip_augment_item_init / danhip_augment_preprocess_batch (the training input pass for a whole batch in a constant number of launches); 12: danhip_resize_item_init / danhip_resize_u8_linear_batch / danhip_detect_select (the test-time pipeline for images of different sizes); 13: danhip_cls_accuracy (the training metric, counted on the device); 14: danhip_crc32c_host / _combine / _batch (CRC-32C of checkpoint tensors on the host and on the device); 15: danhip_jpeg_encode_* (baseline JPEG encode, byte for byte Pillow's) and danhip_draw_boxes_u8 (box drawing on device images); 16: danhip_jpeg_encode_scan_* / _huffman_batch / _entropy_emulate_batch (the encoder's Huffman stage on the device); 17: the deformable backward in deterministic mode (ordered far corners): danhip_deform_sample_bwd_ordered_workspace_bytes / danhip_deform_conv_bwd_ordered_workspace_bytes / danhip_deform_far_ordered / danhip_deform_far_ordered_emulate; 18: danhip_draw_boxes_labels_u8 / danhip_draw_glyph / danhip_draw_format_score (the score label of the debug images); 19: danhip_conv_transpose4x4s2_* (transposed convolution 4x4 / stride 2: the LFPN's learnable upsampling); 20: danhip_jpeg_optimal_table_host / danhip_jpeg_encode_entropy_batch_ex / danhip_jpeg_encode_scan_prepare_ex / danhip_jpeg_encode_optimize_layout / danhip_jpeg_optimal_tables_device (the JPEG encoder's optimize=True, on the host and on the device); 21: danhip_bn_act_* (fused batch-norm tails: batch norm + residual add + ReLU in one apply pass, masked backward); 22: danhip_face_chips_workspace / danhip_face_chips_u8 (face chips: every detection cropped and resized on the device in two launches); 23: danhip_face_chips_u8_ex / danhip_face_chips_ex_workspace (zero-padded chips, area downscale); 24: danhip_redact_* (face redaction: blur, mosaic, fill)
extern "C" int danhip_act_dtype(void) {
#ifdef DANHIP_FP16
  return DANHIP_F16;
#else
  return DANHIP_BF16;
#endif
}

// ---- kernel-selection switches (process-wide; initial values from the environment): danhip_set_option / danhip_get_option.
//   "splitk"     DANHIP_SPLITK      1 (default) / 0: split-K for maps with too few output tiles (when the caller passes scratch)
//   "wgrad_slab" DANHIP_WGRAD_SLAB  1 (default: short launches) / 0 (never) / 2 (always): weight-gradient partials as stores + combine pass
//   "halo_b2"    DANHIP_HALO_B2     0 (default) / 1: second workgroup barrier per step in conv_halo.hip (the round-2 form; A/B switch)
//   "wgrad_b2"   DANHIP_WGRAD_B2    0 (default) / 1: the same for conv_wgrad_rows.hip / conv_wgrad_pw.hip
//   "halo_general_epilogue" DANHIP_HALO_GENERAL_EPILOGUE  0 (default) / 1: conv_halo.hip always takes its general epilogue (A/B of the lean one)
//   "wgrad_c8"   DANHIP_WGRAD_C8    1 (default) / 0: the first layer's weight gradient on conv_wgrad_c8.hip (0: the general kernel; A/B and tests)
//   "deform_dx_untiled" DANHIP_DEFORM_DX_UNTILED  0 (default) / 1: the deformable backward's +-1 px gather as the wave-per-pixel kernel (A/B, tests)
//   "pw_dgrad_ld_bn" DANHIP_PW_DGRAD_LD_BN  128 (default) / 256: widest tile of conv_pointwise.hip's data gradient WITH epilogue inputs (A/B:
//                the 256-wide form reads dY once but measured no faster - S3FD 1198.6 vs 1197.6 img/s, DAN 433.9 vs 436.2)
//   "deterministic" DANHIP_DETERMINISTIC  0 (default) / 1: every cross-workgroup fp32 sum of the S3FD training step in a fixed order (partials
//                as plain stores into the caller's workspace + ordered_reduce.hip) instead of float atomics: bit-reproducible per (library build,
//                CU count).  Entry points that would need atomics return DANHIP_EINVAL (danhip.h "Deterministic mode")
//   "crc_table"  DANHIP_CRC_TABLE   1 (default) / 0: danhip_crc32c_batch walks its chunks with a slicing-by-4 table in LDS (1) or with the
//                table-free shift form (0) (crc32c_exact.hip; same bits; measured 1153 vs 764 GB/s on the S3FD shard)
namespace {
// Thread safety ("no mutable globals" on the data path): the table is filled from the environment exactly once
// (std::call_once, before the first read or write), every value is a relaxed atomic, and the kernels' host launchers read an option
// once per call into their argument struct - a concurrent danhip_set_option changes which FORM later launches take (all forms are
// result-equivalent up to fp32 summation order), never a launch already being assembled.
struct Opt { const char* name; const char* env; int def; std::atomic<int> value; };
Opt g_opts[] = {{"splitk", "DANHIP_SPLITK", 1, {0}}, {"wgrad_slab", "DANHIP_WGRAD_SLAB", 1, {0}}, {"halo_b2", "DANHIP_HALO_B2", 0, {0}},
                {"wgrad_b2", "DANHIP_WGRAD_B2", 0, {0}}, {"halo_general_epilogue", "DANHIP_HALO_GENERAL_EPILOGUE", 0, {0}},
                {"deform_bwd_form", "DANHIP_DEFORM_BWD_FORM", 0, {0}}, {"pw_dgrad_ld_bn", "DANHIP_PW_DGRAD_LD_BN", 128, {0}},
                {"wgrad_c8", "DANHIP_WGRAD_C8", 1, {0}}, {"deform_dx_untiled", "DANHIP_DEFORM_DX_UNTILED", 0, {0}},
                {"deterministic", "DANHIP_DETERMINISTIC", 0, {0}}, {"crc_table", "DANHIP_CRC_TABLE", 1, {0}}};
std::once_flag g_opts_once;
Opt* find_opt(const char* name) {
  std::call_once(g_opts_once, [] {
    for (Opt& o : g_opts) { const char* e = getenv(o.env); o.value.store(e ? atoi(e) : o.def, std::memory_order_relaxed); }
  });
  if (!name) return nullptr;
  for (Opt& o : g_opts)
    if (strcmp(o.name, name) == 0) return &o;
  return nullptr;
}
}  // namespace

int danhip_option(const char* name) {
  Opt* o = find_opt(name);
  return o ? o->value.load(std::memory_order_relaxed) : 0;
}
extern "C" int danhip_get_option(const char* name) { return danhip_option(name); }

// Compute units of the current device: asked once per process, 256 (the MI355X's count) when there is no device.
int dh_cu_count() {
  static const int n = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) return 256;
    return v;
  }();
  return n;
}
extern "C" int danhip_set_option(const char* name, int value) {
  Opt* o = find_opt(name);
  if (!o) { danhip_set_error("set_option: unknown option '%s'", name ? name : "(null)"); return DANHIP_EINVAL; }
  o->value.store(value, std::memory_order_relaxed);
  return DANHIP_OK;
}
