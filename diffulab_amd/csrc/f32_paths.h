// Which kernel form the last fp32-regime GEMM or softmax call launched (dl_lab_last_f32_path, not in the header:
// tests/test_f32_paths_gpu.py mirrors these names).  As in gemm_paths.h, attn_paths.h and gn_paths.h the entry points store the code
// right before their launch with one relaxed host-side store; nothing on the device.  A split-K product launches the GEMM kernel and
// then f32_gemm_fold_k: the code left behind names the GEMM form and the split.
#pragma once

enum DlF32Path {
  DL_F32_PATH_NONE = 0,
  // dl_f32_gemm
  F32_GEMM_SCALAR = 1,     // f32_gemm_k<.., VEC = false>: element-wise guarded operand loads
  F32_GEMM_VEC,            // f32_gemm_k<.., VEC = true>: float4 operand loads (16-byte bases, ld / strides / contiguous extents % 4 == 0)
  F32_GEMM_SCALAR_SPLITK,  // ... partial images into the caller's scratch + f32_gemm_fold_k
  F32_GEMM_VEC_SPLITK,
  // dl_f32_softmax_fwd / _bwd / _keymask_fwd
  F32_SOFTMAX_FWD_VEC,     // f32_softmax_fwd_k: cols % 4 == 0, cols <= 4096, 16-byte base; the row lives in registers
  F32_SOFTMAX_FWD_ANY,     // f32_softmax_fwd_any_k: three passes over the row
  F32_SOFTMAX_BWD_VEC,     // f32_softmax_bwd_k
  F32_SOFTMAX_BWD_ANY,     // f32_softmax_bwd_any_k
  F32_SOFTMAX_KEYMASK,     // f32_softmax_keymask_fwd_k
  DL_F32_PATH_COUNT
};
