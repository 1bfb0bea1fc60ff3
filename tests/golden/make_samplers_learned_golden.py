"""Generate tests/golden/samplers_learned.npz by IMPORTING THE REAL REFERENCE: its ``DDPM`` / ``DDIM`` samplers with the learned
variance types (``learned``, ``learned_range``: samplers/gaussian_diffusion/ddpm.py:212-222, 268-282; ddim.py:89) on a
``[B, 2C, H, W]`` prediction, and one respaced ``Diffuser.generate`` loop on the small DiT built with twice the output channels.

Runs only in the build container (the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_samplers_learned_golden.py

Like make_golden.py (whose import shims this script reuses by loading it), only OUTPUTS of the reference are stored.  The step inputs
are the existing sampler fixture's (``smp.xt``, ``t = [0, 7, 999]``, 1000 linear steps) plus a second named draw for the variance half;
the global generator's draws are replayed and stored next to the outputs, as ``gen_samplers`` does.  The loop runs on a 16 x 16 latent
(64 tokens, the grid of ``dit_small16``) so that the GPU engines take it as it is.
"""

from __future__ import annotations

import dataclasses
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)  # installs the import shims and imports the reference

import torch  # noqa: E402

from oracle import synth  # noqa: E402

SHAPE = (3, 4, 8, 8)
TIMESTEPS = (0, 7, 999)
LOOP_B, LOOP_H, LOOP_STEPS, LOOP_SEED = 2, 16, 5, 29
KEYS = ("x_prev", "estimated_x0", "x_prev_mean", "x_prev_std", "logprob")


def prediction() -> torch.Tensor:
    """[3, 8, 8, 8]: the existing fixture's `smp.v` as the mean half, a new draw as the raw variance half"""
    return torch.cat([synth.normal("smp.v", SHAPE), synth.normal("smpl.var", SHAPE)], dim=1)


def main() -> None:
    o = {}
    xt, pred = synth.normal("smp.xt", SHAPE), prediction()
    tt = torch.tensor(TIMESTEPS, dtype=torch.int32)
    betas = mg.GaussianDiffusion(n_steps=1000).betas
    for vt in ("learned", "learned_range"):
        for mt in ("epsilon", "xstart", "xprev"):
            for clamp in (False, True):
                s = mg.DDPM(mean_type=mt, var_type=vt)
                s.set_steps(betas)
                torch.manual_seed(13)
                r = s.step(pred, tt, xt, clamp_x=clamp)
                for k in KEYS:
                    o[f"ddpm_{mt}_{vt}_{int(clamp)}_{k}"] = r[k]
    torch.manual_seed(13)
    o["ddpm_noise"] = torch.randn_like(xt)
    for eta in (0.0, 0.5):
        s = mg.DDIM(var_type="learned_range")
        s.set_steps(betas)
        torch.manual_seed(17)
        r = s.step(pred, tt, xt, eta=eta)
        for k in r:
            o[f"ddim_eta{eta}_{k}"] = r[k]
    torch.manual_seed(17)
    o["ddim_noise"] = torch.randn_like(xt)
    # 5-step respaced DDPM loop with learned_range variances, CFG 1.5, clamp, on the small DiT with 8 output channels
    cfg = dataclasses.replace(mg.SMALL, output_channels=2 * mg.SMALL.input_channels)
    m = mg.build_ref(cfg, seed=5).eval()
    y = synth.integers("smpl.y", (LOOP_B,), cfg.n_classes)
    x_init = synth.normal("smpl.init", (LOOP_B, cfg.input_channels, LOOP_H, LOOP_H))
    g = mg.Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000,
                    extra_args={"sampler_parameters": {"var_type": "learned_range"}})
    g.set_steps(LOOP_STEPS)
    torch.manual_seed(LOOP_SEED)
    with torch.no_grad():
        out = g.generate({"x": x_init.clone(), "y": y}, use_tqdm=False, guidance_scale=1.5, clamp_x=True)
    o["loop_ddpm_x"] = out["x"]
    # the global-generator stream of that loop: per step the p = 1 forward draws rand(B) for the label drop (nn.py:149) BEFORE
    # DDPM.step draws randn_like (ddpm.py:302)
    torch.manual_seed(LOOP_SEED)
    nz = []
    for _ in range(LOOP_STEPS):
        torch.rand(LOOP_B)
        nz.append(torch.randn(LOOP_B, cfg.input_channels, LOOP_H, LOOP_H))
    o["loop_ddpm_noise"] = torch.stack(nz)
    assert all(bool(torch.isfinite(torch.nan_to_num(v, 0, 0, 0)).all()) for v in o.values())
    mg.save("samplers_learned", **o)


if __name__ == "__main__":
    main()
