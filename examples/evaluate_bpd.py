"""Bits per dimension of a Gaussian-diffusion model on held-out data, on synthetic MNIST-shaped images: a tiny UNet with learned
variances is trained for a few steps under the hybrid loss and its variational bound on the negative log-likelihood is evaluated with
`Diffuser.evaluate_bpd` (the `calc_bpd_loop` of Nichol & Dhariwal 2021):

    python examples/evaluate_bpd.py
    python examples/evaluate_bpd.py --train-steps 200 --chain 1000 --batch 64
    python examples/evaluate_bpd.py --timing          # wall time of the loop for the MNIST-DDPM UNet at B = 64, T = 1000

Printed: the total in bits / dim (the sum of every timestep's term and the prior term), the prior term, and the per-timestep bound and
squared errors averaged over the four quartiles of the chain, as the IDDPM evaluation script reports them.  Nothing is downloaded or
written.
"""

import argparse
import os
import sys
import time

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


def mnist_unet() -> UNetModel:
    """configs/model/unet.yaml, the denoiser of configs/train_mnist_ddpm.yaml"""
    return UNetModel(image_size=[32, 32], in_channels=1, model_channels=128, out_channels=1, num_res_blocks=2,
                     attention_resolutions=[4, 8, 16], num_heads=2, resblock_updown=True, n_classes=10, use_scale_shift_norm=True,
                     classifier_free=False).to("cuda")


def train(diffuser: Diffuser, model, steps: int, batch: int) -> None:
    diffuser.train()
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    for _ in range(steps):
        y = torch.randint(0, 10, (batch,))
        losses = diffuser.compute_loss({"x": synthetic_images(y, SIZE).cuda(), "y": y.cuda(), "p": 0.1},
                                       timesteps=diffuser.draw_timesteps(batch))
        opt.zero_grad()
        sum(losses.values()).backward()
        opt.step()
    if steps > 0:
        print(f"trained {steps} steps, last loss " + "  ".join(f"{k} {v.item():.4f}" for k, v in losses.items()))
    diffuser.eval()


def report(out: dict[str, torch.Tensor]) -> None:
    n_t = out["vb"].shape[1]
    print(f"bits/dim {out['total_bpd'].mean().item():.4f}   (prior term {out['prior_bpd'].mean().item():.3e}, t = 0 term "
          f"{out['vb'][:, 0].mean().item():.4f}, {out['vb'].shape[0]} samples, {n_t} timesteps)")
    for q in range(4):
        lo, hi = q * n_t // 4, (q + 1) * n_t // 4
        if hi > lo:
            print(f"  quartile {q} (t in [{lo}, {hi})):  vb {out['vb'][:, lo:hi].mean().item():.6f}  "
                  f"xstart_mse {out['xstart_mse'][:, lo:hi].mean().item():.6f}  mse {out['mse'][:, lo:hi].mean().item():.6f}")


def timing() -> None:
    torch.manual_seed(0)
    model = mnist_unet().eval()
    d = Diffuser(model, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    y = torch.randint(0, 10, (64,))
    inputs = {"x": synthetic_images(y, 32).cuda(), "y": y.cuda()}
    for t_chunk in (1, None):
        d.evaluate_bpd(inputs, t_chunk=t_chunk, timesteps=list(range(0, 1000, 125)))  # warm-up: the pass's batch shape
        torch.cuda.synchronize()
        for run in range(2):
            t0 = time.perf_counter()
            out = d.evaluate_bpd(inputs, t_chunk=t_chunk)
            total = out["total_bpd"].mean().item()  # (the read-back ends the measurement)
            dt = time.perf_counter() - t0
            print(f"calc_bpd_loop  MNIST-DDPM UNet  B 64  T 1000  t_chunk {t_chunk}  run {run}: {dt:.3f} s  (bits/dim {total:.4f})")


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-steps", type=int, default=40, help="training steps on the synthetic images before the evaluation")
    ap.add_argument("--chain", type=int, default=100, help="length of the chain the bound is evaluated on (the 1000-step chain respaced)")
    ap.add_argument("--batch", type=int, default=16, help="held-out images")
    ap.add_argument("--t-chunk", type=int, default=None, help="timesteps per pass (default: as many as fit 256 rows)")
    ap.add_argument("--timing", action="store_true", help="time the loop for the MNIST-DDPM UNet at B = 64, T = 1000 instead")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP kernels: it needs a GPU"
    if args.timing:
        return timing()
    torch.manual_seed(0)
    model = tiny_unet()
    d = Diffuser(model, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000,
                 extra_args={"sampler_parameters": {"var_type": "learned_range"}})
    if args.chain != 1000:
        d.set_steps(args.chain)
    y = (torch.arange(args.batch) % 10)
    held_out = {"x": synthetic_images(y, SIZE).cuda(), "y": y.cuda()}
    print("before training:")
    report(d.evaluate_bpd(held_out, t_chunk=args.t_chunk))
    train(d, model, args.train_steps, 64)
    print("after training:")
    out = d.evaluate_bpd(held_out, t_chunk=args.t_chunk)
    assert bool(torch.isfinite(out["total_bpd"]).all())
    report(out)


if __name__ == "__main__":
    main()
