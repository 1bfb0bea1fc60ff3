"""dl_dropout alone at the MNIST UNet's largest site, [64 * 32 * 32, 128], in bf16 and f32: achieved GB/s (bytes the algorithm needs:
one read and one write of the buffer, plus one read of the residual) against the strided copy of the same buffer (dl_copy2d_bf16 /
dl_f32_copy2d: the neighbouring elementwise kernels, one read and one write).  Device events around `iters` back-to-back launches,
after a warm-up; the two kernels alternate, three rounds each.  DESIGN.md section 6, "Dropout".

    python scripts/dropout_bench.py [--rows 65536] [--cols 128] [--iters 200]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from diffulab_amd import ops  # noqa: E402


def timed(fn, iters: int) -> float:
    """seconds per call"""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=64 * 32 * 32)
    ap.add_argument("--cols", type=int, default=128)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--p", type=float, default=0.1)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    state = torch.tensor([1234, 0], dtype=torch.int64, device="cuda")
    T, scale = ops.dropout_threshold(a.p), ops.dropout_scale(a.p)
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.randn(a.rows, a.cols, device="cuda").to(dtype)
        r = torch.randn(a.rows, a.cols, device="cuda").to(dtype)
        out = torch.empty_like(x)
        nbytes = x.numel() * x.element_size()
        copy = ops.copy2d_bf16 if dtype == torch.bfloat16 else ops.f32_copy2d
        forms = {
            "copy": (lambda: copy(x, out, a.rows, a.cols), 2 * nbytes),
            "dropout_inplace": (lambda: ops.dropout(x, x, state, 3, T, 1.0), 2 * nbytes),  # (scale 1: the values stay bounded)
            "dropout_resid": (lambda: ops.dropout(x, out, state, 3, T, scale, resid=r), 3 * nbytes),
        }
        best = {k: float("inf") for k in forms}
        for _ in range(3):
            for k, (fn, _) in forms.items():
                best[k] = min(best[k], timed(fn, a.iters))
        print(json.dumps({"dtype": str(dtype), "rows": a.rows, "cols": a.cols,
                          **{k + "_us": round(best[k] * 1e6, 2) for k in forms},
                          **{k + "_GBps": round(forms[k][1] / best[k] / 1e9, 1) for k in forms}}))


if __name__ == "__main__":
    main()
