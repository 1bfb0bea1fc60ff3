"""Cost of the two post-hoc EMA kernels (csrc/ema.hip) on one MI355X, over flat f32 buffers of the size of the parameter arenas of
DiT-S/2 and of the MNIST-DDPM UNet (configs/train_mnist_ddpm.yaml):
    python scripts/posthoc_ema_bench.py [--arena dit_s2 unet_mnist_ddpm] [--iters 50] [--rounds 3] [--sources 32]

Two pairs of variants, the members of a pair alternating `rounds` times in one process on the same buffers:
    update_multi   one dl_ema_update_multi launch over two profiles          5 arena transfers (read p, read + write 2 profiles)
    update_two     two dl_ema_update launches (what two EMA objects would do)  6 arena transfers
    lincomb        one dl_arena_lincomb launch over K sources                 K + 1 transfers
    torch_adds     out.zero_() + K out.add_(src, alpha=w) passes              3 K + 1 transfers
Expected from the byte counts alone: update_multi / update_two = 5 / 6, lincomb / torch_adds ~ (K + 1) / 3 K.

Device events around each repetition; `iters` repetitions back to back per timing, so one timed window is many launches long.
The K sources are distinct buffers (K = 32: 5 GB at the DiT-S/2 size, 35 GB at the UNet's), so the sources always come from HBM;
the DiT-S/2 arena itself (160 MB) fits the 256 MiB last-level cache, which torch's `out` and part of the update's buffers then
live in, and the reported rates include that.  Reported per
variant and round: microseconds per repetition and the rate its byte count implies, next to the share of the 8 TB/s HBM peak.  The
results of the two members of a pair are compared once (bit for bit for the update; to the chain's rounding for the sum)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffulab_amd import MMDiT, ops  # noqa: E402
from diffulab_amd.config import instantiate, load_config  # noqa: E402

S2 = dict(input_channels=4, output_channels=4, inner_dim=384, embedding_dim=384, num_heads=6, mlp_ratio=4, patch_size=2,
          depth=12, n_classes=1000, classifier_free=True)
HBM_PEAK = 8.0e12  # bytes / s
W = (1.7e-5, 0.25)


def arena_size(name: str) -> int:
    """elements of the model's flat parameter arena (the layout's size: parameters plus alignment gaps)"""
    torch.manual_seed(0)
    m = MMDiT(simple_dit=True, **S2) if name == "dit_s2" else instantiate(load_config(os.path.join(ROOT, "configs"), "train_mnist_ddpm").model)
    m = m.to("cuda")
    m.engine  # noqa: B018
    return m._flat.numel()


def timed(fn, iters: int) -> float:
    """microseconds per call of fn, `iters` calls between two device events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def bench(name: str, iters: int, rounds: int, warmup: int, K: int) -> None:
    dev = "cuda"
    n = arena_size(name)
    g = torch.Generator(device=dev).manual_seed(1)
    p = torch.randn(n, device=dev, generator=g)
    e = [torch.randn(n, device=dev, generator=g) for _ in range(2)]
    srcs = [torch.randn(n, device=dev, generator=g) for _ in range(K)]
    w = [(-1.0) ** k * 10.0 / K for k in range(K)]
    out_a, out_b = torch.empty(n, device=dev), torch.empty(n, device=dev)

    def torch_adds():
        out_b.zero_()
        for s, wk in zip(srcs, w):
            out_b.add_(s, alpha=wk)

    variants = {
        "update_multi": (lambda: ops.ema_update_multi(e, p, W), 5),
        "update_two": (lambda: (ops.ema_update(e[0], p, 1.0 - W[0]), ops.ema_update(e[1], p, 1.0 - W[1])), 6),
        "lincomb": (lambda: ops.arena_lincomb(out_a, srcs, w), K + 1),
        "torch_adds": (torch_adds, 3 * K + 1),
    }
    # same results first: the fused update against two single launches bit for bit (0 < w < 1), the sum against torch's passes
    a = [x.clone() for x in e]
    b = [x.clone() for x in e]
    ops.ema_update_multi(a, p, [1.0 - 0.75, 1.0 - 0.9375])
    ops.ema_update(b[0], p, 0.75), ops.ema_update(b[1], p, 0.9375)
    variants["lincomb"][0](), torch_adds()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "fused update differs from two single updates"
    scale = sum(abs(wk) * s.abs() for s, wk in zip(srcs[:4], w)).max().item() * K / 4
    assert float((out_a - out_b).abs().max()) <= (K + 1) * 2.0 ** -23 * scale, "fused sum differs from torch's passes beyond rounding"

    per_variant = {v: [] for v in variants}
    for rnd in range(rounds):
        for v, (fn, passes) in variants.items():
            timed(fn, warmup)
            us = [timed(fn, iters) for _ in range(3)]
            med = statistics.median(us)
            per_variant[v].append(med)
            rate = passes * 4 * n / (med * 1e-6)
            print(json.dumps({"what": "posthoc_ema", "arena": name, "floats": n, "variant": v, "round": rnd, "us": round(med, 1),
                              "us_min": round(min(us), 1), "us_max": round(max(us), 1), "transfers": passes,
                              "GBs": round(rate / 1e9, 1), "hbm_peak_share": round(rate / HBM_PEAK, 3)}), flush=True)
    summary = {"what": "posthoc_ema_summary", "arena": name, "floats": n, "sources": K}
    for v, meds in per_variant.items():
        summary[v + "_us"] = round(statistics.median(meds), 1)
        summary[v + "_spread_us"] = round(max(meds) - min(meds), 1)  # run-to-run spread: between the rounds' medians
    summary["update_multi_over_two"] = round(summary["update_multi_us"] / summary["update_two_us"], 3)
    summary["update_expected"] = round(5 / 6, 3)
    summary["lincomb_over_torch"] = round(summary["lincomb_us"] / summary["torch_adds_us"], 3)
    summary["lincomb_expected"] = round((K + 1) / (3 * K + 1), 3)
    summary["update_multi_GBs"] = round(5 * 4 * n / summary["update_multi_us"] / 1e3, 1)
    summary["lincomb_GBs"] = round((K + 1) * 4 * n / summary["lincomb_us"] / 1e3, 1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arena", nargs="+", default=["dit_s2", "unet_mnist_ddpm"], choices=["dit_s2", "unet_mnist_ddpm"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sources", type=int, default=32)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("posthoc_ema_bench needs a GPU (there is nothing to measure without one)")
    for arena in a.arena:
        bench(arena, a.iters, a.rounds, a.warmup, a.sources)
