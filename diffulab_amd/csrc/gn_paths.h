// Which kernel the last GroupNorm call launched (dl_lab_last_gn_path, not in the header: tests/test_gn_paths_gpu.py mirrors these
// names).  As in gemm_paths.h and attn_paths.h the entry points store the code right before their launch with one relaxed host-side
// store; nothing on the device.  dl_gn_fwd in its two-launch form goes through dl_gn_stats and dl_gn_apply_fwd: the code left behind is
// GN_APPLY_FWD.
#pragma once

enum DlGnPath {
  DL_GN_PATH_NONE = 0,
  // dl_gn_fwd, one launch (unet.hip)
  GN_FWD_FUSED_16_4 = 1,  // gn_fwd_fused_k<16, 4>: 128-channel slabs, HW <= 64
  GN_FWD_FUSED_12_4,      // gn_fwd_fused_k<12, 4>: 96-channel slabs, HW <= 84
  GN_FWD_FUSED_12_12,     // gn_fwd_fused_k<12, 12>: 96-channel slabs, HW <= 252
  GN_FWD_FUSED_8_4,       // gn_fwd_fused_k<8, 4>: 64-channel slabs, HW <= 128
  GN_FWD_FUSED_8_8,       // gn_fwd_fused_k<8, 8>: 64-channel slabs, HW <= 256
  GN_FWD_FUSED_8_32,      // gn_fwd_fused_k<8, 32>: 64-channel slabs, HW <= 1024
  // dl_gn_stats / dl_gn_apply_fwd (and dl_gn_fwd where no fused form takes the shape)
  GN_STATS,               // gn_stats_k, C <= 2048: one LDS row per pixel lane, fixed order
  GN_STATS_ATOMIC,        // gn_stats_k, C > 2048: LDS float atomics
  GN_APPLY_FWD,           // gn_apply_fwd_k
  // dl_gn_bwd, one launch
  GN_BWD_FUSED_16_4,      // gn_bwd_fused_k<16, 4>: 128-channel slabs, HW <= 64, C >= 512
  GN_BWD_FUSED_8_0,       // gn_bwd_fused_k<8, 0>: 64-channel slabs, 64 < HW <= 1024
  GN_BWD_FUSED_12_4,      // gn_bwd_fused_k<12, 4>: 96-channel slabs, HW <= 84
  GN_BWD_FUSED_12_0,      // gn_bwd_fused_k<12, 0>: 96-channel slabs, 84 < HW <= 1024
  GN_BWD_FUSED_64_0,      // gn_bwd_fused_k<64, 0>: 512-channel slabs, HW <= 64, C >= 512
  // dl_gn_bwd, three launches: reduce + gn_group_sums_k + gn_bwd_apply_k
  GN_BWD_REDUCE_64,       // gn_bwd_reduce_k<64>: HW <= 64, C >= 512, one pixel range
  GN_BWD_REDUCE_8,        // gn_bwd_reduce_k<8>: 1 .. DL_GN_BWD_MAX_RANGES pixel ranges
  DL_GN_PATH_COUNT
};
