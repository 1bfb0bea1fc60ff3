// Which kernel the last GEMM-family call launched (dl_lab_last_path, not in the header: tests/test_gemm_paths_gpu.py mirrors these
// names).  The dispatchers store the code right before their launch with one relaxed host-side store; nothing on the device.
#pragma once

enum DlGemmPath {
  DL_PATH_NONE = 0,
  // dl_gemm_nt (and dl_gemm_nt_swiglu: its persistent tilings are the same kernels with EPI 2)
  NT_BIG_384 = 1,    // gemm_nt_big_k<384, 2, EPI>
  NT_BIG_256,        // gemm_nt_big_k<256, 2, EPI>
  NT_BIG_192,        // gemm_nt_big_k<192, 2, EPI>
  NT_BIG_128,        // gemm_nt_big_k<128, 3, EPI>
  NT_SMALL_RING2,    // gemm_nt_k<false, 2>, one split
  NT_SMALL_RING4,    // gemm_nt_k<false, 4>, one split
  NT_SPLITK_RING2,   // gemm_nt_k<false, 2>, split contraction meeting in f32 atomics on C zeroed by hipMemset(2D)Async
  NT_SPLITK_RING4,   // gemm_nt_k<false, 4>, the same
  // dl_gemm_nt_f32_det
  NT_DET,            // gemm_nt_k<false, 2>, one split, f32 out
  NT_DET_SPLITK,     // gemm_nt_k<false, 2> partial images in scratch + fold_partials_k
  // dl_gemm_nt_pair
  NT_PAIR_RING2,     // gemm_nt_k<false, 2> running both products (second from ep.tiles0)
  NT_PAIR_RING4,     // gemm_nt_k<false, 4> running both products
  NT_PAIR_FALLBACK,  // two dl_gemm_nt calls
  // dl_gemm_tn_ex
  TN_W4,             // gemm_tn_w4_k: 384 x 192 tiles, four-slot ring, f32 atomics
  TN_BIG,            // gemm_tn_big_k<false>: 384 x 128 tiles, f32 atomics
  TN_SMALL,          // gemm_tn_k<false>, one split, f32 atomics
  TN_SMALL_SPLITK,   // gemm_tn_k<false>, split contraction meeting in f32 atomics
  // dl_gemm_tn_det (shapes the ring kernel does not take)
  TN_DET,            // gemm_tn_k<false> partial images in scratch + fold_partials_k
  // dl_gemm_tn_group (and dl_gemm_tn_det on the shapes it forwards there)
  TN_GROUP_384,      // gemm_tn_group_k<384, 192> + tn_group_fold_k
  TN_GROUP_256,      // gemm_tn_group_k<256, 256> + tn_group_fold_k, whole tiles
  TN_GROUP_256_EDGE, // gemm_tn_group_k<256, 256> + tn_group_fold_k, last tile of a row / column shifted back to the edge
  // dl_conv3x3_nt
  CONV_HALO_256_2,   // conv3x3_halo_k<256, 2>
  CONV_HALO_128_4,   // conv3x3_halo_k<128, 4>
  CONV_HALO_128_3,   // conv3x3_halo_k<128, 3>
  CONV_HALO_128_2,   // conv3x3_halo_k<128, 2>
  CONV_BIG_256,      // conv3x3_big_k<256>, one split
  CONV_BIG_128,      // conv3x3_big_k<128>, one split
  CONV_BIG_256_SPLITK,  // conv3x3_big_k<256> partial images + conv_splitk_finalize_k
  CONV_BIG_128_SPLITK,  // conv3x3_big_k<128> partial images + conv_splitk_finalize_k
  CONV_SMALL_RING2,  // gemm_nt_k<true, 2>, one split
  CONV_SMALL_RING4,  // gemm_nt_k<true, 4>, one split
  CONV_SPLITK_RING2, // gemm_nt_k<true, 2> partial images + conv_splitk_finalize_k
  CONV_SPLITK_RING4, // gemm_nt_k<true, 4> partial images + conv_splitk_finalize_k
  DL_PATH_COUNT
};

void dl_note_path(int path);  // gemm.hip
