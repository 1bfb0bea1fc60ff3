// Which kernel the last attention call launched (dl_lab_last_attn_path, not in the header: tests/test_attn_paths_gpu.py mirrors these
// names).  As in gemm_paths.h the entry points store the code right before their launch with one relaxed host-side store; nothing on
// the device.  A separate enum from DlGemmPath: each table of cases asserts that it reaches every code of its own enum.
#pragma once

enum DlAttnPath {
  DL_ATTN_PATH_NONE = 0,
  // DiT family, head_dim 64 (attention.hip)
  ATTN_FWD_RESIDENT = 1,  // attn_fwd_k: dl_attn_fwd / _sv, N <= 256
  ATTN_FWD_TILED,         // attn_fwd_tiled_k: dl_attn_fwd_ex (and dl_attn_fwd for N > 256) up to 2048 tokens
  ATTN_FWD_QKN_CHAIN,     // attn_fwd_qkn_k: dl_attn_fwd_qkn, one workgroup per (sample, head)
  ATTN_FWD_QKN_PIPE,      // attn_fwd_qkn_pipe_k: dl_attn_fwd_qkn, persistent + pipelined (N = 256, B * H >= 3 CUs)
  ATTN_BWD_RESIDENT,      // attn_bwd_k: dl_attn_bwd / _sv / _tok, N <= 256 (one kernel, three output layouts)
  ATTN_BWD_TILED,         // attn_bwd_tiled_k: dl_attn_bwd_ex (and dl_attn_bwd for N > 256) up to 2048 tokens
  // UNet small attention (n <= 64): MFMA forms in attention.hip, VALU forms in unet.hip
  ATTN_SMALL_FWD_MFMA,    // attn_small_mfma_fwd_k: head_dim % 64 == 0 up to 512
  ATTN_SMALL_FWD_VALU,    // attn_small_fwd_k: every other head width
  ATTN_SMALL_BWD_MFMA,    // attn_small_mfma_bwd_k
  ATTN_SMALL_BWD_VALU,    // attn_small_bwd_k
  // UNet masked cross-attention (L <= 512)
  ATTN_CROSS_FWD_MFMA,    // attn_cross_mfma_fwd_k: Nq <= 64, head_dim % 64 == 0 up to 512
  ATTN_CROSS_FWD_VALU,    // attn_cross_fwd_k: every other shape
  ATTN_CROSS_BWD_MFMA,    // attn_cross_mfma_bwd_k
  ATTN_CROSS_BWD_VALU,    // attn_cross_bwd_q_k + attn_cross_bwd_kv_k
  // beyond 2048 tokens (checked by tests/test_attn_long_gpu.py)
  ATTN_FWD_LONG_BIAS,     // attn_fwd_long_k<true>
  ATTN_FWD_LONG_NOBIAS,   // attn_fwd_long_k<false>
  ATTN_BWD_LONG,          // attn_bwd_delta_k + attn_bwd_dkdv_long_k + attn_bwd_dq_long_k
  DL_ATTN_PATH_COUNT
};

void dl_note_attn_path(int path);  // attention.hip
