"""bit-level fingerprint of the row kernels of csrc/norm.hip: one line `op case output sha256` for every deterministic output of the
six operations over a fixed seeded case list (every width class, every fusion flag on).  Two builds that print the same lines
compute the same bits; select the library with DIFFULAB_HIP_LIB.
    python scripts/row_kernel_bits.py > bits.txt
Left out: the sums that meet in global float atomics, whose order is not fixed even within one build (dscale / dshift / dgate / dwb
of dl_ln_modulate_bwd, dwb of the per-token form, dscale of dl_qk_norm_rope_bwd); the bounds of tests/test_row_paths_gpu.py and
tests/test_wide_rows_gpu.py cover them."""
import hashlib, os, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import torch
from diffulab_amd import ops
import row_bounds as rb

WIDTHS = (64, 384, 520, 1024, 1088, 2048, 3072, 4096)
ROWS = ((2, 100), (4, 256))


def emit(op, case, res, keys):
    for k in keys:
        h = hashlib.sha256(res[k].contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
        print(f"{op} {case} {k} {h}", flush=True)


for D in WIDTHS:
    dh = 64 if D % 64 == 0 else 40  # 520 = 13 heads of 40
    for B, N in ROWS:
        case, seed = f"D={D},B={B},N={N}", D + N
        emit("ln_modulate_fwd", case, rb.run_ln_fwd(ops, D, B, N, True, True, seed=seed, check=False), ("out", "x_out", "mean", "rstd"))
        emit("ln_modulate_bwd", case, rb.run_ln_bwd(ops, D, B, N, True, True, True, seed=seed, check=False), ("dx", "dt"))
        emit("ln_modulate_bwd_tok", case, rb.run_ln_bwd_tok(ops, D, B * N, True, True, seed=seed, check=False),
             ("dx", "dt", "dscale", "dshift", "dgate"))
        emit("gate_bwd", case, rb.run_gate_bwd(ops, D, B, N, seed=seed, check=False), ("dt", "dgate"))
        # partly rotary heads, a row window into longer q / k / v and a position table
        emit("qk_norm_rope", case, rb.run_qk(ops, B, N, D // dh, dh, dh // 2 // 8 * 8, True, seed=seed, check=False),
             ("q", "k", "v", "rrms", "dqkv"))
