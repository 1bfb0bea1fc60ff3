// Which kernel form the last call of a bf16 auxiliary dispatcher launched (dl_lab_last_aux_path, not in the header:
// tests/test_bf16_aux_paths_gpu.py mirrors these names).  As in gemm_paths.h, attn_paths.h, gn_paths.h and f32_paths.h the entry
// points store the code right before their launch with one relaxed host-side store; nothing on the device.
// conv3x3_wgrad_fold_batched_k picks its form (staged tile, image-sum tile, tap split) on the device from the descriptor's n_img:
// the host cannot note it, the tests assert it through n_img and DL_FOLD_TAP_SPLIT_MIN_IMAGES.
#pragma once

enum DlAuxPath {
  DL_AUX_PATH_NONE = 0,
  // dl_im2col3x3
  AUX_IM2COL_VEC = 1,           // im2col3x3_k: C % 8 == 0, ldx % 8 == 0, 16-byte base
  AUX_IM2COL_SCALAR,            // im2col3x3_scalar_k
  // dl_cast_conv3x3_weight
  AUX_CAST_CONV_TILED,          // cast_conv3x3_tiled_k: whole 32 x 32 channel tiles, dense shadows
  AUX_CAST_CONV_DIRECT,         // cast_conv3x3_k
  // dl_conv3x3_wgrad_fold
  AUX_FOLD_TILED,               // conv3x3_wgrad_fold_tiled_k
  AUX_FOLD_DIRECT,              // conv3x3_wgrad_fold_k
  // dl_resample2x2_pair
  AUX_RESAMPLE_VEC_PAIR,        // resample2x2_vec_k, two tensors (grid.y = 2)
  AUX_RESAMPLE_VEC_SINGLE,      // resample2x2_vec_k, one tensor
  AUX_RESAMPLE_SCALAR,          // dl_reduce2x2 / dl_expand2x2 per tensor (C % 8 != 0 or a base off the 16-byte grid)
  // dl_colsum / dl_colsum_det
  AUX_COLSUM_BF16_VEC,          // colsum_vec_k
  AUX_COLSUM_BF16_SCALAR,       // colsum_k<bf16_t> / colsum_part_k<bf16_t>
  AUX_COLSUM_F32,               // colsum_k<float> / colsum_part_k<float>
  // dl_colsum_batched (noted after the list is walked; a fallback entry's dl_colsum notes its own code first)
  AUX_COLSUM_BATCHED,           // every descriptor went through colsum_batched_k
  AUX_COLSUM_BATCHED_FALLBACK,  // at least one descriptor took a dl_colsum launch of its own
  DL_AUX_PATH_COUNT
};
void dl_note_aux_path(int path);  // embed.hip
