// Which kernel the last 3x3 weight-gradient call (dl_conv3x3_wgrad_tn, dl_conv3x3_wgrad_tn_parts) launched (dl_lab_last_wgrad_path,
// not in the header: tests/test_conv_wgrad_paths_gpu.py mirrors these names).  As in gemm_paths.h, gn_paths.h and attn_paths.h the
// dispatcher stores the code right before its launch with one relaxed host-side store; nothing on the device.  A refused call leaves
// the code of the call before it.
#pragma once

enum DlConvWgradPath {
  WG_NONE = 0,
  // conv3x3_wgrad_halo_k (conv_wgrad.hip): all nine taps from one staged halo, by map width
  WG_HALO_W32 = 1,  // conv3x3_wgrad_halo_k<5, 2>: W = 32, two image rows per 64-pixel step
  WG_HALO_W16,      // conv3x3_wgrad_halo_k<4, 4>: W = 16, four image rows per step
  WG_HALO_W8,       // conv3x3_wgrad_halo_k<3, 8>: 8 x 8, one image per step
  WG_HALO_W4,       // conv3x3_wgrad_halo_k<2, 4>: 4 x 4, four images per step
  // the implicit-GEMM kernels of gemm.hip: every map the halo kernel does not take
  WG_IGEMM_BIG,     // gemm_tn_big_k<true>: 384 x 128 tiles (R >= 4096, Co % 128 == 0)
  WG_IGEMM_SMALL,   // gemm_tn_k<true>: 128 x 128 tiles
  WG_PATH_COUNT
};

void dl_note_wgrad_path(int path);  // conv_wgrad.hip
