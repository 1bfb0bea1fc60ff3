"""Training a Gaussian-diffusion model for bits per dimension, on synthetic MNIST-shaped images: a tiny learned-variance UNet is
trained on the variational bound itself (loss_type="vlb": the bound's gradient reaches the mean output as well as the variance
output) with the timestep drawn by importance from a running second moment of the per-timestep loss
(timestep_sampler="loss_second_moment"), sec. 3.3 of Nichol & Dhariwal, "Improved Denoising Diffusion Probabilistic Models" (2021):

    python examples/train_vlb.py
    python examples/train_vlb.py --train-steps 1000 --chain 100 --batch 64
    python examples/train_vlb.py --loss-type mse --timestep-sampler uniform      # the hybrid loss with uniform draws, for comparison

Printed: `Diffuser.evaluate_bpd` of held-out images before and after the training, and the sampling distribution the history arrived
at, per quartile of the chain.  Nothing is downloaded or written.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffulab_amd import Diffuser
from diffulab_amd.networks.denoisers import UNetModel
from diffulab_amd.training.optim import FusedAdamW

SIZE = 32


def synthetic_images(labels: torch.Tensor, size: int) -> torch.Tensor:
    """one smooth pattern per class: an oriented sinusoid in [-1, 1], one channel"""
    u = torch.linspace(-1.0, 1.0, size)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    angle = labels.float().view(-1, 1, 1, 1) * (torch.pi / 10)
    return torch.sin(3.0 * (xx * torch.cos(angle) + yy * torch.sin(angle)))


def tiny_unet() -> UNetModel:
    return UNetModel(image_size=[SIZE, SIZE], in_channels=1, model_channels=32, out_channels=2, num_res_blocks=1,
                     attention_resolutions=[2], channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True,
                     n_classes=10, classifier_free=True).to("cuda")


def bits_per_dim(d: Diffuser, held_out) -> float:
    d.eval()
    out = d.evaluate_bpd(held_out)
    assert bool(torch.isfinite(out["total_bpd"]).all())
    return out["total_bpd"].mean().item()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-steps", type=int, default=300, help="training steps on the synthetic images")
    ap.add_argument("--chain", type=int, default=50, help="length of the chain that is trained and evaluated (the 1000-step chain respaced)")
    ap.add_argument("--batch", type=int, default=64, help="training batch size")
    ap.add_argument("--held-out", type=int, default=16, help="held-out images the bound is evaluated on")
    ap.add_argument("--loss-type", default="vlb", choices=["mse", "vlb"])
    ap.add_argument("--timestep-sampler", default="loss_second_moment", choices=["uniform", "loss_second_moment"])
    ap.add_argument("--lr", type=float, default=1e-3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP kernels: it needs a GPU"
    torch.manual_seed(0)
    model = tiny_unet()
    d = Diffuser(model, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000,
                 extra_args={"sampler_parameters": {"var_type": "learned_range"}, "loss_type": args.loss_type,
                             "timestep_sampler": args.timestep_sampler})
    if args.chain != 1000:
        d.set_steps(args.chain)
    y = torch.arange(args.held_out) % 10
    held_out = {"x": synthetic_images(y, SIZE).cuda(), "y": y.cuda()}
    print(f"before training: {bits_per_dim(d, held_out):.4f} bits/dim  ({args.held_out} samples, {args.chain} timesteps)")
    d.train()
    opt = FusedAdamW(model.parameters(), lr=args.lr)
    for step in range(args.train_steps):
        y = torch.randint(0, 10, (args.batch,))
        losses = d.compute_loss({"x": synthetic_images(y, SIZE).cuda(), "y": y.cuda(), "p": 0.1}, timesteps=d.draw_timesteps(args.batch))
        opt.zero_grad()
        sum(losses.values()).backward()
        opt.step()
    if args.train_steps > 0:
        print(f"trained {args.train_steps} steps ({args.loss_type}, {args.timestep_sampler}), last loss "
              + "  ".join(f"{k} {v.item():.4f}" for k, v in losses.items()))
    print(f"after training:  {bits_per_dim(d, held_out):.4f} bits/dim")
    state = d.diffusion.timestep_sampler_state
    if state is not None and state.tensors:
        p, counts = state.tensors["p"].cpu(), state.tensors["counts"].cpu()
        n = p.numel()
        warm = bool((counts == state.history_per_term).all())
        print(f"sampling distribution ({'warmed up' if warm else 'still uniform: not every timestep has its history yet'}):")
        for q in range(4):
            lo, hi = q * n // 4, (q + 1) * n // 4
            if hi > lo:
                print(f"  quartile {q} (t in [{lo}, {hi})):  probability {p[lo:hi].sum().item():.4f}")


if __name__ == "__main__":
    main()
