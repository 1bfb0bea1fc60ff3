"""Fixture `dit_input_grad.npz`: the imported reference's gradient of the flow loss with respect to the noised latents z_t, on the
`pb.small` inputs of tests/test_parity_bf16_gpu.py (small DiT, B = 4, 16 x 16 latents), in fp32 and under
``torch.autocast("cpu", bfloat16)``, with the relative L2 error between the two -- the yardstick the input gradient of the HIP engines
is held to (tests/test_input_grad_gpu.py) and the pin of the oracle's own input gradient (tests/test_flow_nll_host.py).

A generator only: it imports the reference through the shims of make_golden.py and calls it; nothing of its text is here.  The
reference's `compute_loss` noises the data itself, so z_t is caught where it enters the denoiser: a forward pre-hook replaces the
`x` keyword by a leaf that requires grad.

    python tests/golden/make_input_grad_golden.py        (where the reference is installed)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (installs the shims and imports the reference)

from oracle import synth  # noqa: E402


def input_grad(m, x0, t, y, noise):
    """(loss, z_t, d loss / d z_t) of the reference's flow loss"""
    caught = {}

    def pre(module, args, kwargs):
        caught["z"] = kwargs["x"].detach().clone().requires_grad_(True)
        return args, {**kwargs, "x": caught["z"]}

    h = m.register_forward_pre_hook(pre, with_kwargs=True)
    try:
        loss = mg.flow_loss_ref(m, x0, t, y, noise)
        loss.backward()
    finally:
        h.remove()
    return loss.detach().float(), caught["z"].detach().float(), caught["z"].grad.detach().float()


def main() -> None:
    tag, cfg, seed, B, H = "pb.small", mg.SMALL, 5, 4, 16
    x0, noise = synth.normal(f"{tag}.x0", (B, cfg.input_channels, H, H)), synth.normal(f"{tag}.noise", (B, cfg.input_channels, H, H))
    t = synth.uniform(f"{tag}.t", (B,), lo=0.05, hi=0.95)
    y = synth.integers(f"{tag}.y", (B,), cfg.n_classes)
    l32, z, g32 = input_grad(mg.build_ref(cfg, seed=seed), x0, t, y, noise)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        lac, _, gac = input_grad(mg.build_ref(cfg, seed=seed), x0, t, y, noise)
    err = ((gac.double() - g32.double()).norm() / g32.double().norm()).item()
    np.savez(os.path.join(HERE, "dit_input_grad.npz"), z=z.numpy(), dz_fp32=g32.numpy(), dz_autocast=gac.numpy(), loss_fp32=l32.numpy(),
             loss_autocast=lac.numpy(), autocast_err=np.float64(err))
    print(f"{tag}: loss fp32 {l32.item():.6f} autocast {lac.item():.6f}; d loss / d z_t: norm {g32.norm().item():.4e}, autocast rel-L2 error {err:.3e}")


if __name__ == "__main__":
    main()
