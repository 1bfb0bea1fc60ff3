"""Cost of `optimizer.step()` alone with SGD (momentum 0.9, Nesterov, weight decay 1e-4) on one MI355X, over the parameter arenas
of DiT-S/2 and of the MNIST-DDPM UNet (configs/train_mnist_ddpm.yaml):
    python scripts/sgd_step_bench.py [--arena dit_s2 unet_mnist_ddpm] [--iters 24] [--rounds 3]

Four variants on the SAME parameters and gradients, alternating `rounds` times in one process:
    fused        FusedSGD                          one dl_sgd_step launch over the arena
    fused_clip   FusedSGD(max_grad_norm=1)         + grad_sumsq, clip_coef in front; the update takes the coefficient
    torch        torch.optim.SGD on the arena views      (what `optimizer=sgd` resolved to before FusedSGD)
    torch_clip   training.utils.clip_grad_norm_ (in place) + torch.optim.SGD   (what the trainer did for it with max_grad_norm)
Device events around each step (which covers the gaps in which the device waits for the host's launches); before every timed step
the gradient arena is refilled from a saved copy outside the timed region, so the in-place clipping always has something to scale
and every variant starts from the same cache state.  Reported per variant and round: the median of `iters` steps, and the rate five
passes over the arena (read p, g, buf; write p, buf) imply at that time."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diffulab_amd import MMDiT  # noqa: E402
from diffulab_amd.config import instantiate, load_config  # noqa: E402
from diffulab_amd.training import FusedSGD  # noqa: E402
from diffulab_amd.training.utils import clip_grad_norm_  # noqa: E402

S2 = dict(input_channels=4, output_channels=4, inner_dim=384, embedding_dim=384, num_heads=6, mlp_ratio=4, patch_size=2,
          depth=12, n_classes=1000, classifier_free=True)
HYPER = dict(lr=1e-5, momentum=0.9, nesterov=True, weight_decay=1e-4)


def build(name):
    torch.manual_seed(0)
    if name == "dit_s2":
        return MMDiT(simple_dit=True, **S2)
    return instantiate(load_config(os.path.join(ROOT, "configs"), "train_mnist_ddpm").model)


def bench(name: str, iters: int, rounds: int, warmup: int) -> None:
    dev = "cuda"
    m = build(name).to(dev)
    m.engine  # flattens the parameters into the arena and attaches the .grad views
    n = m._flat.numel()
    saved = torch.randn(n, device=dev) * 1e-3
    params = [p for p in m.parameters() if p.requires_grad]
    opts = {"fused": FusedSGD(params, **HYPER), "fused_clip": FusedSGD(params, max_grad_norm=1.0, **HYPER),
            "torch": torch.optim.SGD(params, **HYPER), "torch_clip": torch.optim.SGD(params, **HYPER)}

    def one(variant):
        m._flat_grad.copy_(saved)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if variant == "torch_clip":
            clip_grad_norm_(params, 1.0)
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
            print(json.dumps({"what": "sgd_step", "arena": name, "floats": n, "tensors": len(params), "variant": variant, "round": rnd,
                              "us_median": round(med, 1), "us_min": round(min(us), 1), "us_max": round(max(us), 1),
                              "five_pass_GBs": round(5 * 4 * n / med / 1e3, 1)}), flush=True)
    assert bool(torch.isfinite(m._flat).all())
    summary = {"what": "sgd_step_summary", "arena": name, "floats": n}
    for v, meds in per_variant.items():
        summary[v + "_us"] = round(statistics.median(meds), 1)
        summary[v + "_spread_us"] = round(max(meds) - min(meds), 1)  # run-to-run spread: between the rounds' medians
    summary["torch_over_fused"] = round(summary["torch_us"] / summary["fused_us"], 2)
    summary["torch_clip_over_fused_clip"] = round(summary["torch_clip_us"] / summary["fused_clip_us"], 2)
    summary["fused_five_pass_GBs"] = round(5 * 4 * n / summary["fused_us"] / 1e3, 1)
    print(json.dumps(summary), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arena", nargs="+", default=["dit_s2", "unet_mnist_ddpm"], choices=["dit_s2", "unet_mnist_ddpm"])
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sgd_step_bench needs a GPU (there is nothing to measure without one)")
    for arena in a.arena:
        bench(arena, a.iters, a.rounds, a.warmup)
