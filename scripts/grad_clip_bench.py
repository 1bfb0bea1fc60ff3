"""Cost of gradient clipping by global norm on one MI355X:
    python scripts/grad_clip_bench.py pass             # grad_sumsq + clip_coef alone at the DiT-S/2 and MNIST-DDPM UNet arena sizes
    python scripts/grad_clip_bench.py step --batch 256 # the DiT-S/2 training step, max_grad_norm off / on, alternating twice

`pass`: every timed call reads a buffer that was NOT the last one read (the buffers of a size rotate and together exceed the 256 MiB
Infinity Cache), as in a training step, where the backward and the update stream several arenas between two norm passes.  Device
events around each call; the median is reported next to the time the bytes need at the achievable HBM read rate.
`step`: host clock around `steps` steps ending in a synchronise, the same optimizer object with `max_grad_norm` None / 1.0."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from diffulab_amd import Diffuser, MMDiT, ops  # noqa: E402
from diffulab_amd.training import FusedAdamW  # noqa: E402

HBM_READ_TBS = 6.3  # achievable HBM read rate of the MI355X (8 TB/s spec)
SIZES = {"dit_s2": 39_900_000, "unet_mnist_ddpm": 276_700_000}
S2 = dict(input_channels=4, output_channels=4, inner_dim=384, embedding_dim=384, num_heads=6, mlp_ratio=4, patch_size=2,
          depth=12, n_classes=1000, classifier_free=True)


def bench_pass(iters: int) -> None:
    dev = "cuda"
    for name, n in SIZES.items():
        nbuf = max(2, -(-(1 << 30) // (4 * n)))  # >= 1 GiB in rotation
        bufs = [torch.randn(n, device=dev) for _ in range(nbuf)]
        partials = torch.zeros(ops.grad_sumsq_slots(n), device=dev)
        out = torch.zeros(2, device=dev)

        def call(i):
            k = ops.grad_sumsq(bufs[i % nbuf], partials, 0)
            ops.clip_coef(partials, k, 1.0, out)

        for i in range(2 * nbuf):
            call(i)
        torch.cuda.synchronize()
        pair, only = [], []
        for i in range(iters):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            k = ops.grad_sumsq(bufs[i % nbuf], partials, 0)
            e[1].record()
            ops.clip_coef(partials, k, 1.0, out)
            e[2].record()
            e[2].synchronize()
            only.append(e[0].elapsed_time(e[1]) * 1e3)
            pair.append(e[0].elapsed_time(e[2]) * 1e3)
        floor = 4 * n / (HBM_READ_TBS * 1e12) * 1e6
        med = statistics.median(pair)
        print(json.dumps({"what": "grad_sumsq+clip_coef", "arena": name, "floats": n, "slots": k, "chain": ops.grad_sumsq_chain(n),
                          "pair_us_median": round(med, 1), "pair_us_min": round(min(pair), 1), "pair_us_max": round(max(pair), 1),
                          "sumsq_us_median": round(statistics.median(only), 1), "floor_us_at_6.3TBs": round(floor, 1),
                          "x_floor": round(med / floor, 3), "read_TBs": round(4 * n / med / 1e6, 3), "norm": out[0].item()}))
        del bufs


def bench_step(batch: int, steps: int, warmup: int) -> None:
    dev = "cuda"
    torch.manual_seed(0)
    m = MMDiT(simple_dit=True, **S2).to(dev)
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=50, extra_args={"logits_normal": True})
    opt = FusedAdamW(m.parameters(), lr=1e-4, weight_decay=0.01)
    x0 = torch.randn(batch, 4, 32, 32, device=dev)
    y = torch.randint(0, 1000, (batch,), device=dev)

    def step():
        opt.zero_grad()
        t = d.draw_timesteps(batch).to(dev, non_blocking=True)
        d.compute_loss({"x": x0, "y": y, "p": 0.1}, timesteps=t)["loss"].backward()
        opt.step()

    res = []
    for rnd in range(2):
        for mode in (None, 1.0):
            opt.max_grad_norm = mode
            for _ in range(warmup):
                step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / steps * 1e3
            res.append((mode, ms))
            print(json.dumps({"what": "dit_s2_step", "batch": batch, "round": rnd, "max_grad_norm": mode, "ms_per_step": round(ms, 3),
                              "grad_norm": None if mode is None else opt.last_grad_norm.item(), "arena_floats": m._flat_grad.numel()}))
    off = statistics.mean(ms for mode, ms in res if mode is None)
    on = statistics.mean(ms for mode, ms in res if mode is not None)
    print(json.dumps({"what": "dit_s2_step_summary", "off_ms": round(off, 3), "on_ms": round(on, 3), "added_us": round((on - off) * 1e3, 1)}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pass", "step"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--iters", type=int, default=60)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grad_clip_bench needs a GPU (there is nothing to measure without one)")
    bench_pass(a.iters) if a.what == "pass" else bench_step(a.batch, a.steps, a.warmup)
