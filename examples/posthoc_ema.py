"""Post-hoc EMA on synthetic MNIST-shaped images (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion
Models", sec. 3.2): a tiny UNet is trained for a few hundred steps while `PowerEMA` tracks two power-function profiles
(sigma_rel 0.05 and 0.10) and snapshots them; afterwards `posthoc_ema.synthesize` builds the EMA of three OTHER widths from the
snapshots -- one between the tracked two, one below, one above -- without training again:

    python examples/posthoc_ema.py
    python examples/posthoc_ema.py --train-steps 600 --snapshot-every 25 --sigma-rels 0.04 0.075 0.15

Printed per width: the validation loss of the synthesised weights on held-out noise draws and the 1-norm of the coefficient vector
(1 for a stored snapshot; it grows as the target leaves the range the tracked profiles span, and the synthesis loses accuracy with
it).  Snapshots go to a temporary directory that is removed at the end; nothing is downloaded.
"""

import argparse
import copy
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from diffulab_amd import Diffuser
from diffulab_amd.networks.denoisers import UNetModel
from diffulab_amd.training import PowerEMA, posthoc_ema
from diffulab_amd.training.optim import FusedAdamW

SIZE = 32


def synthetic_images(labels: torch.Tensor, size: int) -> torch.Tensor:
    """one smooth pattern per class: an oriented sinusoid in [-1, 1], one channel"""
    u = torch.linspace(-1.0, 1.0, size)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    angle = labels.float().view(-1, 1, 1, 1) * (torch.pi / 10)
    return torch.sin(3.0 * (xx * torch.cos(angle) + yy * torch.sin(angle)))


def tiny_unet() -> UNetModel:
    return UNetModel(image_size=[SIZE, SIZE], in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1,
                     attention_resolutions=[2], channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True,
                     n_classes=10, classifier_free=True).to("cuda")


@torch.no_grad()
def validation_loss(d: Diffuser, model: UNetModel, batches: list) -> float:
    """mean training loss of `model` over fixed held-out (images, labels, timesteps, noise) draws"""
    online, d.denoiser = d.denoiser, model.eval()
    try:
        total = 0.0
        for x, y, t, noise in batches:
            total += sum(v.item() for v in d.compute_loss({"x": x.clone(), "y": y, "p": 0.0}, timesteps=t, noise=noise.clone()).values())
        return total / len(batches)
    finally:
        d.denoiser = online


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-steps", type=int, default=300)
    ap.add_argument("--snapshot-every", type=int, default=20, help="EMA updates between two snapshots")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--sigma-rels", type=float, nargs=3, default=[0.03, 0.075, 0.15], help="widths to synthesise")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP kernels: it needs a GPU"
    torch.manual_seed(0)
    model = tiny_unet()
    d = Diffuser(model, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    opt = FusedAdamW(model.parameters(), lr=args.lr)
    ema = PowerEMA(model, sigma_rels=(0.05, 0.10))
    held_out = []
    for _ in range(4):
        y = torch.randint(0, 10, (args.batch,))
        held_out.append((synthetic_images(y, SIZE).cuda(), y.cuda(), d.draw_timesteps(args.batch),
                         torch.randn(args.batch, 1, SIZE, SIZE).cuda()))
    with tempfile.TemporaryDirectory() as snap_dir:
        d.train()
        for _ in range(args.train_steps):
            y = torch.randint(0, 10, (args.batch,))
            losses = d.compute_loss({"x": synthetic_images(y, SIZE).cuda(), "y": y.cuda(), "p": 0.1}, timesteps=d.draw_timesteps(args.batch))
            opt.zero_grad()
            sum(losses.values()).backward()
            opt.step()
            ema.update()
            if ema.t % args.snapshot_every == 0:
                ema.snapshot(snap_dir)
        if ema.t % args.snapshot_every != 0:
            ema.snapshot(snap_dir)  # the end of the run is always a snapshot time
        n_files = len(posthoc_ema.read_index(snap_dir))
        print(f"trained {args.train_steps} steps, {n_files} snapshots of profiles {ema.sigma_rels}; validation loss: online "
              f"{validation_loss(d, model, held_out):.5f}, tracked " +
              ", ".join(f"{s:.3f}: {validation_loss(d, m, held_out):.5f}" for s, m in zip(ema.sigma_rels, ema.ema_models)))
        scratch = copy.deepcopy(model)
        for s in args.sigma_rels:
            coef = posthoc_ema.synthesize(scratch, snap_dir, s)
            print(f"sigma_rel {s:.3f}: validation loss {validation_loss(d, scratch, held_out):.5f}, coefficient 1-norm {np.abs(coef).sum():.3f}")


if __name__ == "__main__":
    main()
