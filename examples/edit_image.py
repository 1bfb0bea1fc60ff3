"""Image-to-image (SDEdit) and inpainting (RePaint) with `Diffuser.generate`, on synthetic data:

    python examples/edit_image.py                                   # a small DiT, a few training steps, then the three edits
    python examples/edit_image.py --checkpoint denoiser.pt          # a trained state dict of the same architecture instead
    python examples/edit_image.py --model-type gaussian_diffusion --sampler ddpm --steps 20 --resample 2

`init_image` lives in the space the denoiser works in (pixels here; scaled latents behind a vision tower).  `strength` is the fraction
of the sampler's steps that is run, from `init_image` noised to the level where they start; `mask` is 1 where the image is generated and
0 where it is kept; `resample` repeats every step but the last (RePaint's U).  Nothing is downloaded or written.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from diffulab_amd import Diffuser, MMDiT
from diffulab_amd.training.optim import FusedAdamW


def synthetic_images(labels: torch.Tensor, channels: int, size: int) -> torch.Tensor:
    """one smooth pattern per class: oriented sinusoids in [-1, 1]"""
    u = torch.linspace(-1.0, 1.0, size)
    yy, xx = torch.meshgrid(u, u, indexing="ij")
    angle = labels.float().view(-1, 1, 1, 1) * (torch.pi / 10)
    phase = torch.arange(channels).float().view(1, -1, 1, 1) * 0.7
    return torch.sin(3.0 * (xx * torch.cos(angle) + yy * torch.sin(angle)) + phase)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model-type", default="rectified_flow", choices=["rectified_flow", "gaussian_diffusion"])
    ap.add_argument("--sampler", default="euler", help="euler | euler_maruyama (rectified_flow), ddpm | ddim (gaussian_diffusion)")
    ap.add_argument("--steps", type=int, default=10, help="sampler steps")
    ap.add_argument("--train-steps", type=int, default=20, help="training steps on the synthetic images before the edits")
    ap.add_argument("--checkpoint", default=None, help="state dict of the denoiser (skips the training steps)")
    ap.add_argument("--guidance-scale", type=float, default=2.0)
    ap.add_argument("--resample", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this example runs the HIP kernels: it needs a GPU"
    torch.manual_seed(0)
    C, size = 4, 16
    model = MMDiT(simple_dit=True, input_channels=C, output_channels=C, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4,
                  patch_size=2, depth=2, n_classes=10, classifier_free=True)
    if args.checkpoint:
        model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"))
    model = model.to("cuda")
    gaussian = args.model_type == "gaussian_diffusion"
    diffuser = Diffuser(model, sampling_method=args.sampler, model_type=args.model_type, n_steps=1000 if gaussian else args.steps)

    if not args.checkpoint and args.train_steps > 0:
        diffuser.train()
        opt = FusedAdamW(model.parameters(), lr=1e-3)
        for step in range(args.train_steps):
            y = torch.randint(0, 10, (64,))
            batch = {"x": synthetic_images(y, C, size).cuda(), "y": y.cuda(), "p": 0.1}
            loss = diffuser.compute_loss(batch, timesteps=diffuser.draw_timesteps(64))["loss"]
            opt.zero_grad()
            loss.backward()
            opt.step()
        print(f"trained {args.train_steps} steps, last loss {loss.item():.4f}")
    diffuser.eval()
    if gaussian and args.sampler == "ddpm":
        diffuser.set_steps(args.steps)  # respaced chain (the reference's DDIM respacing takes the full chain only)
    steps = diffuser.diffusion.steps

    y = torch.arange(args.batch) % 10
    init = synthetic_images(y, C, size).cuda()
    target = (y + 5) % 10  # edit towards another class
    common = dict(use_tqdm=False, guidance_scale=args.guidance_scale, clamp_x=True)  # (the images live in [-1, 1])

    def rms(a, b):
        return (a - b).pow(2).mean().sqrt().item()

    # 1. image-to-image at two strengths: the lower one stays closer to the image it started from
    for strength in (0.3, 0.7):
        out = diffuser.generate({"y": target.cuda()}, init_image=init, strength=strength, **common)["x"]
        print(f"image-to-image  strength {strength}: rms distance from init_image {rms(out, init):.4f}, "
              f"from the target class's pattern {rms(out, synthetic_images(target, C, size).cuda()):.4f}")

    # 2. inpainting of a centre box: everything outside it is init_image, bit for bit
    mask = torch.zeros(args.batch, 1, size, size, device="cuda")
    mask[:, :, size // 4:3 * size // 4, size // 4:3 * size // 4] = 1.0
    out = diffuser.generate({"y": y.cuda()}, init_image=init, mask=mask, resample=args.resample, return_intermediates=True, **common)
    keep = (mask == 0).expand_as(init)
    assert torch.equal(out["x"][keep], init[keep]) and bool(torch.isfinite(out["x"]).all())
    print(f"inpainting      {steps} steps, resample {args.resample}: kept region identical to init_image, "
          f"filled box rms distance from the original {rms(out['x'][~keep], init[~keep]):.4f}; "
          f"{out['xt'].shape[1]} recorded states of shape {tuple(out['xt'].shape[2:])}")


if __name__ == "__main__":
    main()
