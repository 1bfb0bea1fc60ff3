"""Likelihood of a rectified-flow model on held-out data, on synthetic images: a small DiT is trained for a few steps under the flow
loss and the negative log-likelihood of its probability-flow ODE is evaluated with `Diffuser.evaluate_nll` (instantaneous change of
variables with Hutchinson's divergence estimate, Grathwohl et al. 2019), before and after the training, with the Euler and the Heun
solver at two step counts:

    python examples/evaluate_nll.py
    python examples/evaluate_nll.py --train-steps 400 --steps 8 32 --probes 4 --precision fp32

Printed per evaluation: bits per dimension of the 8-bit data (nll / ln 2 + log2(127.5)), the negative log-likelihood in nats per
dimension and its two parts, the prior term -log N(x1; 0, I) and the integrated divergence.  The same probes and the same
dequantisation noise are used for every evaluation, so the rows differ by the solver and the weights only.  Nothing is downloaded or
written.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffulab_amd import Diffuser, MMDiT
from diffulab_amd.training.optim import FusedAdamW

SIZE, CHANNELS = 16, 4


def synthetic_images(labels: torch.Tensor) -> torch.Tensor:
    """one smooth pattern per class: oriented sinusoids in [-1, 1], a phase per channel"""
    u = torch.linspace(-1.0, 1.0, SIZE)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    angle = labels.float().view(-1, 1, 1, 1) * (torch.pi / 10)
    phase = torch.arange(CHANNELS).float().view(1, -1, 1, 1) * (torch.pi / CHANNELS)
    return torch.sin(3.0 * (xx * torch.cos(angle) + yy * torch.sin(angle)) + phase)


def train(diffuser: Diffuser, model, steps: int, batch: int) -> None:
    diffuser.train()
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    for _ in range(steps):
        y = torch.randint(0, 10, (batch,))
        loss = diffuser.compute_loss({"x": synthetic_images(y).cuda(), "y": y.cuda(), "p": 0.1}, timesteps=diffuser.draw_timesteps(batch))["loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
    if steps > 0:
        print(f"trained {steps} steps, last loss {loss.item():.4f}")
    diffuser.eval()


def report(d: Diffuser, held_out: dict, step_counts: list[int], probes: torch.Tensor, u: torch.Tensor) -> None:
    for method in ("euler", "heun"):
        for n in step_counts:
            d.set_steps(n)
            out = d.evaluate_nll(held_out, method=method, probes=probes, dequant_noise=u)
            assert bool(torch.isfinite(out["nll"]).all())
            print(f"  {method:5s} {n:3d} steps ({out['div_terms'].shape[1]:3d} evaluations): bits/dim {out['total_bpd'].mean().item():.4f}   "
                  f"nll {out['nll'].mean().item():.4f} nats/dim = prior {out['prior'].mean().item():.4f} - divergence "
                  f"{out['div'].mean().item():.4f}")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-steps", type=int, default=100, help="training steps on the synthetic images between the two evaluations")
    ap.add_argument("--steps", type=int, nargs=2, default=[4, 16], help="the two step counts of the ODE grid")
    ap.add_argument("--batch", type=int, default=8, help="held-out images")
    ap.add_argument("--probes", type=int, default=2, help="Hutchinson probes per image")
    ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP kernels: it needs a GPU"
    torch.manual_seed(0)
    model = MMDiT(simple_dit=True, input_channels=CHANNELS, output_channels=CHANNELS, inner_dim=128, embedding_dim=64, num_heads=2,
                  mlp_ratio=4, patch_size=2, depth=2, n_classes=10, classifier_free=True)
    model.set_precision(args.precision)
    model = model.to("cuda")
    d = Diffuser(model, sampling_method="euler", model_type="rectified_flow", n_steps=args.steps[0])
    y = torch.arange(args.batch) % 10
    held_out = {"x": synthetic_images(y).cuda(), "y": y.cuda()}
    shape = (args.batch, CHANNELS, SIZE, SIZE)
    probes = torch.randint(0, 2, (args.probes, *shape)).float() * 2.0 - 1.0  # Rademacher
    u = torch.rand(shape)
    print("before training:")
    report(d, held_out, args.steps, probes, u)
    train(d, model, args.train_steps, 64)
    print("after training:")
    report(d, held_out, args.steps, probes, u)


if __name__ == "__main__":
    main()
