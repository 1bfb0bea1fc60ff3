"""Generate tests/golden/unet_context.npz by IMPORTING THE REAL REFERENCE: the text-conditioned ``UNetModel`` (a ``TransformerBlock``
at every attention stage, unet.py:358-464) driven by a parameter-free, channel-first context embedder defined below.

Runs only in the build container (the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_unet_context_golden.py

Like make_golden.py (whose import shims this script reuses by loading it), only OUTPUTS of the reference are stored: weights come
from ``oracle.synth.generic_params`` over the reference model's own ``state_dict`` shapes, inputs from named ``oracle.synth`` draws,
and the tests regenerate both.  Per case, two legs: fp32, and ``torch.autocast("cpu", bfloat16)`` (the bf16 yardstick: the relative
error of the reference's own autocast run against its fp32 run, per tensor).
"""

from __future__ import annotations

import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)  # installs the import shims and imports the reference

import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffulab.networks.embedders.common import ContextEmbedder  # noqa: E402

from oracle import synth  # noqa: E402

B, L, C_CTX = 4, 20, 96
MASK_LENGTHS = (20, 7, 1, 0)  # the last sample attends to nothing
TIMESTEPS = (3, 500, 999, 0)
BASE = dict(image_size=[16, 16], in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=[2],
            channel_mult="1, 2", num_heads=2)
CASES = {
    "d1": dict(BASE, use_scale_shift_norm=True, resblock_updown=True, transformer_depth=1),
    "d2": dict(BASE, use_scale_shift_norm=True, resblock_updown=True, transformer_depth=2),
    "dflt": dict(BASE, transformer_depth=1),  # constructor defaults: additive conditioning, Downsample / Upsample modules
}


class ChannelFirstEmbedder(ContextEmbedder):
    """parameter-free: hands precomputed channel-first embeddings [B, C_ctx, L] and a boolean key mask [B, L] through"""

    def __init__(self, channels: int) -> None:
        super().__init__()
        self._n_output = 1
        self._output_size = (channels,)

    def drop_conditions(self, context, p):
        return context

    def forward(self, context, p: float = 0):
        return {"embeddings": context["embeddings"], "attn_mask": context["attn_mask"]}


def inputs() -> dict:
    emb = synth.normal("uc.ctx", (B, C_CTX, L))
    mask = torch.arange(L)[None, :] < torch.tensor(MASK_LENGTHS)[:, None]
    x0 = synth.normal("uc.x0", (B, 3, 16, 16))
    noise = synth.normal("uc.noise", (B, 3, 16, 16))
    return dict(emb=emb, mask=mask, x0=x0, noise=noise, t=torch.tensor(TIMESTEPS, dtype=torch.int32))


def build(kw: dict, seed: int):
    m = mg.UNetModel(context_embedder=ChannelFirstEmbedder(C_CTX), **kw)
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict(synth.generic_params(shapes, seed=seed))
    return m, shapes


def gen() -> None:
    # (the inputs' definition is recorded: tests/test_unet_context_host.py checks tests/unet_context_common.py against it)
    out: dict = {"mask_lengths": np.array(MASK_LENGTHS), "timesteps": np.array(TIMESTEPS), "shape_b_l_cctx": np.array([B, L, C_CTX]),
                 "cases_json": np.array(json.dumps(CASES, sort_keys=True))}
    inp = inputs()
    ctx = {"embeddings": inp["emb"], "attn_mask": inp["mask"]}
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()  # noqa: E731
    for tag, kw in CASES.items():
        legs = {}
        for leg in ("fp32", "autocast"):
            m, shapes = build(kw, seed=61)
            gd = mg.Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
            xt = gd.diffusion.add_noise(inp["x0"], inp["t"], inp["noise"])[0]
            with torch.autocast("cpu", dtype=torch.bfloat16, enabled=leg == "autocast"):
                pred = m(x=xt, timesteps=inp["t"], context=ctx, p=0.0)["x"].detach().float()
                loss = gd.compute_loss({"x": inp["x0"].clone(), "context": ctx, "p": 0.0}, timesteps=inp["t"], noise=inp["noise"])["loss"]
            loss.backward()
            legs[leg] = (pred, loss.detach().float(), {n: p.grad.detach().float().clone() for n, p in m.named_parameters()})
        f32, ac = legs["fp32"], legs["autocast"]
        names = list(f32[2])
        o = {"sd_names": np.array(list(shapes)), "sd_shapes": np.array([",".join(map(str, s)) for s in shapes.values()]),
             "pred": f32[0], "loss": f32[1], "names": np.array(names),
             "grad_norms": np.array([f32[2][n].double().norm().item() for n in names]),
             "ac_pred_err": np.float64(rel(ac[0], f32[0])), "ac_loss": ac[1], "ac_err": np.array([rel(ac[2][n], f32[2][n]) for n in names])}
        for n in names:
            if f32[2][n].numel() <= 2048:
                o["g_" + n] = f32[2][n]
        assert all(bool(torch.isfinite(v).all()) for v in (f32[0], ac[0], *f32[2].values(), *ac[2].values())), tag
        e = o["ac_err"][o["grad_norms"] > 1e-6 * o["grad_norms"].max()]
        print(f"{tag}: loss fp32 {f32[1].item():.6f} autocast {ac[1].item():.6f}; autocast prediction error {o['ac_pred_err']:.3e}; "
              f"per-tensor gradient error median {np.median(e):.3e} max {e.max():.3e}")
        out.update({f"{tag}_{k}": v for k, v in o.items()})
    mg.save("unet_context", **out)


if __name__ == "__main__":
    gen()
