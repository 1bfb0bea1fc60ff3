"""Cost of `optimizer.step()` alone with Muon on one MI355X, over the parameter arena of DiT-S/2 (configs/model/dit_s2.yaml, the
benchmark's model):
    python scripts/muon_step_bench.py [--iters 24] [--rounds 3] [--depth 12]

Three variants on the SAME parameters and gradients, alternating `rounds` times in one process:
    adamw        FusedAdamW                     one dl_adamw_step launch over the arena (what the training step pays today)
    fused        FusedMuon                      19 launches: pre pass, norms, scaling, 5 x (Gram, polynomial, apply), post pass
    stock        torch.optim.Muon on the arena views of the Muon matrices + torch.optim.AdamW on the views of the rest
                                                 (what a user could assemble before FusedMuon)
Device events around each step (which covers the gaps in which the device waits for the host's launches); before every timed step
the gradient arena is refilled from a saved copy outside the timed region, so every variant starts from the same cache state.
Reported per variant and round: the median of `iters` steps; the summary has the median and the spread of the rounds' medians, what
FusedMuon adds over FusedAdamW, the stock pair over FusedMuon (per round and overall), and the rate the 0.3 TFLOP of the
Newton-Schulz iterations imply at FusedMuon's time beyond FusedAdamW's."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffulab_amd import MMDiT  # noqa: E402
from diffulab_amd.training import FusedAdamW, FusedMuon  # noqa: E402

S2 = dict(input_channels=4, output_channels=4, inner_dim=384, embedding_dim=384, num_heads=6, mlp_ratio=4, patch_size=2,
          depth=12, n_classes=1000, classifier_free=True)
LR = 1e-5


class StockPair:
    def __init__(self, params):
        mu = [p for p in params if FusedMuon.qualifies(p)]
        ids = {id(p) for p in mu}
        self.opts = [torch.optim.Muon(mu, lr=LR), torch.optim.AdamW([p for p in params if id(p) not in ids], lr=LR)]

    def step(self):
        for o in self.opts:
            o.step()


def ns_flops(params, ns_steps=5) -> float:
    total = 0.0
    for p in params:
        if FusedMuon.qualifies(p):
            m, n = min(p.shape), max(p.shape)
            total += ns_steps * (2.0 * m * m * n * 2 + 2.0 * m * m * m)  # Gram and apply over the long side, the polynomial's A A
    return total


def bench(depth: int, iters: int, rounds: int, warmup: int) -> None:
    dev = "cuda"
    torch.manual_seed(0)
    m = MMDiT(simple_dit=True, **dict(S2, depth=depth)).to(dev)
    m.engine  # flattens the parameters into the arena and attaches the .grad views
    n = m._flat.numel()
    saved = torch.randn(n, device=dev) * 1e-3
    params = [p for p in m.parameters() if p.requires_grad]
    opts = {"adamw": FusedAdamW(params, lr=LR), "fused": FusedMuon(params, lr=LR), "stock": StockPair(params)}
    flops = ns_flops(params)

    def one(variant):
        m._flat_grad.copy_(saved)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        opts[variant].step()
        e1.record()
        return e0, e1

    per_variant = {v: [] for v in opts}
    for rnd in range(rounds):
        for variant in opts:
            for _ in range(warmup):
                one(variant)
            torch.cuda.synchronize()
            ev = [one(variant) for _ in range(iters)]
            torch.cuda.synchronize()
            us = [a.elapsed_time(b) * 1e3 for a, b in ev]
            med = statistics.median(us)
            per_variant[variant].append(med)
            print(json.dumps({"what": "muon_step", "depth": depth, "floats": n, "tensors": len(params), "variant": variant, "round": rnd,
                              "us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1)}), flush=True)
    assert bool(torch.isfinite(m._flat).all())
    summary = {"what": "muon_step_summary", "depth": depth, "floats": n, "muon_matrices": sum(FusedMuon.qualifies(p) for p in params),
               "ns_gflop": round(flops / 1e9, 1)}
    for v, meds in per_variant.items():
        summary[v + "_us"] = round(statistics.median(meds), 1)
        summary[v + "_spread_us"] = round(max(meds) - min(meds), 1)  # run-to-run spread: between the rounds' medians
    summary["fused_minus_adamw_us"] = round(summary["fused_us"] - summary["adamw_us"], 1)
    summary["stock_over_fused_per_round"] = [round(s / f, 2) for s, f in zip(per_variant["stock"], per_variant["fused"])]
    summary["stock_over_fused"] = round(summary["stock_us"] / summary["fused_us"], 2)
    summary["ns_TFLOPs"] = round(flops / max(summary["fused_minus_adamw_us"], 1e-3) / 1e6, 1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--depth", type=int, default=12)
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("muon_step_bench needs a GPU (there is nothing to measure without one)")
    bench(a.depth, a.iters, a.rounds, a.warmup)
