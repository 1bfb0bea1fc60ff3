"""Fewer denoiser forwards per sample with the second-order multistep samplers, on synthetic data: a tiny class-conditional DiT is
trained for a few steps as a rectified-flow model and a tiny UNet as a DDPM v predictor, and each is sampled from the same seed with
the first-order sampler and with the second-order one at fewer steps:

    python examples/fast_sampling.py
    python examples/fast_sampling.py --euler-steps 50 --ab2-steps 20 --chain 100 --dpmpp-steps 20

`ab2` (rectified flow) is variable-step Adams-Bashforth 2 on the velocity; `dpmpp_2m` (Gaussian diffusion) is DPM-Solver++(2M), Lu et
al. 2022.  Both make one forward per step, as `euler` and `ddim` do, and keep one tensor of the previous step.  For each family the
distance of both results from a long first-order run (the `--ref-steps` Euler run, the full-chain DDIM run) is printed, and the
distance between the two.  `ddim` samples the whole chain (its respacing accepts stride 1 only); `dpmpp_2m` samples the IDDPM-respaced
chain of `--dpmpp-steps` steps.  Nothing is downloaded or written.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffulab_amd import Diffuser, MMDiT
from diffulab_amd.networks.denoisers import UNetModel
from diffulab_amd.training.optim import FusedAdamW

SIZE = 16


def synthetic_images(labels: torch.Tensor, size: int) -> torch.Tensor:
    """one smooth pattern per class: an oriented sinusoid in [-1, 1], one channel"""
    u = torch.linspace(-1.0, 1.0, size)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    angle = labels.float().view(-1, 1, 1, 1) * (torch.pi / 10)
    return torch.sin(3.0 * (xx * torch.cos(angle) + yy * torch.sin(angle)))


def unet() -> UNetModel:
    return UNetModel(image_size=[SIZE, SIZE], in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1,
                     attention_resolutions=[2], channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True,
                     n_classes=10, classifier_free=True).to("cuda")


def dit() -> MMDiT:
    return MMDiT(simple_dit=True, input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4,
                 patch_size=2, depth=2, n_classes=10, classifier_free=True).to("cuda")


def train(diffuser: Diffuser, model, steps: int, channels: int) -> None:
    if steps <= 0:
        return
    diffuser.train()
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    for _ in range(steps):
        y = torch.randint(0, 10, (64,))
        batch = {"x": synthetic_images(y, SIZE).expand(-1, channels, -1, -1).contiguous().cuda(), "y": y.cuda(), "p": 0.1}
        loss = diffuser.compute_loss(batch, timesteps=diffuser.draw_timesteps(64))["loss"]
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"trained {steps} steps, last loss {loss.item():.4f}")
    diffuser.eval()


def sample(diffuser: Diffuser, y: torch.Tensor, guidance: float, channels: int) -> torch.Tensor:
    torch.manual_seed(1)  # the same initial noise for every sampler
    out = diffuser.generate({"y": y}, data_shape=(y.shape[0], channels, SIZE, SIZE), use_tqdm=False, guidance_scale=guidance)["x"]
    assert bool(torch.isfinite(out).all())
    return out


def dist(a: torch.Tensor, b: torch.Tensor) -> str:
    d = (a - b).abs()
    return f"max {d.max().item():.4f} mean {d.mean().item():.4f}"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train-steps", type=int, default=30, help="training steps of each model on the synthetic images")
    ap.add_argument("--euler-steps", type=int, default=50)
    ap.add_argument("--ab2-steps", type=int, default=20)
    ap.add_argument("--ref-steps", type=int, default=200, help="the long Euler run both flow results are compared with")
    ap.add_argument("--chain", type=int, default=100, help="length of the cosine DDPM chain, which DDIM samples in full")
    ap.add_argument("--dpmpp-steps", type=int, default=20, help="steps of the respaced chain dpmpp_2m samples")
    ap.add_argument("--guidance-scale", type=float, default=2.0)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP kernels: it needs a GPU"
    y = (torch.arange(args.batch) % 10).cuda()

    torch.manual_seed(0)
    model = dit()
    flow = {name: Diffuser(model, sampling_method=name, model_type="rectified_flow", n_steps=n)
            for name, n in (("euler", args.euler_steps), ("ab2", args.ab2_steps))}
    ref = Diffuser(model, sampling_method="euler", model_type="rectified_flow", n_steps=args.ref_steps)
    train(flow["euler"], model, args.train_steps, 4)
    model.eval()
    x_ref, x_euler, x_ab2 = (sample(d, y, args.guidance_scale, 4) for d in (ref, flow["euler"], flow["ab2"]))
    print(f"rectified flow, distance from euler {args.ref_steps} steps:  euler {args.euler_steps} steps {dist(x_euler, x_ref)};  "
          f"ab2 {args.ab2_steps} steps {dist(x_ab2, x_ref)}")
    print(f"rectified flow, euler {args.euler_steps} steps against ab2 {args.ab2_steps} steps: {dist(x_euler, x_ab2)}")

    torch.manual_seed(0)
    model = unet()
    extra = {"schedule": "cosine", "sampler_parameters": {"mean_type": "v"}, "loss_target": "mean_type"}
    ddim = Diffuser(model, sampling_method="ddim", model_type="gaussian_diffusion", n_steps=args.chain, extra_args=extra)
    dpmpp = Diffuser(model, sampling_method="dpmpp_2m", model_type="gaussian_diffusion", n_steps=args.chain, extra_args=extra)
    full = Diffuser(model, sampling_method="dpmpp_2m", model_type="gaussian_diffusion", n_steps=args.chain, extra_args=extra)
    if args.dpmpp_steps != args.chain:
        dpmpp.set_steps(args.dpmpp_steps, schedule="cosine")
    train(ddim, model, args.train_steps, 1)
    model.eval()
    x_ddim, x_dpmpp, x_full = (sample(d, y, args.guidance_scale, 1) for d in (ddim, dpmpp, full))
    print(f"gaussian diffusion, distance from ddim {args.chain} steps:  dpmpp_2m {args.dpmpp_steps} steps {dist(x_dpmpp, x_ddim)};  "
          f"dpmpp_2m {args.chain} steps {dist(x_full, x_ddim)}")


if __name__ == "__main__":
    main()
