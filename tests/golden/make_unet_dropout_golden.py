"""Generate tests/golden/unet_dropout.npz by IMPORTING THE REAL REFERENCE: the small class-conditional ``UNetModel`` of
``make_golden.gen_unet`` (same parameters, same inputs) built with ``dropout=0.3`` in ``train()`` mode, with every ``nn.Dropout`` its
forward reaches -- ``ResBlock.out_layers.2`` (unet.py:171) and ``AttentionBlock.to_out.1`` (unet.py:272) -- replaced by a module that
multiplies by ``mask * float32(1 / (1 - p))``.  The mask is the numpy definition of tests/dropout_common.py at ``seed=1234, step=0`` and
the block's site, generated as ``[B, pixels, C]`` (the token-row view the HIP kernel indexes) and permuted to the reference's
channel-first layout.

Runs only in the build container (the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_unet_dropout_golden.py

Like make_golden.py (whose import shims this script reuses by loading it), only OUTPUTS of the reference are stored.  The site map
(block prefix -> site) is counted here from the reference's own module tree -- every child of every ``input_blocks[i]``, of
``middle_block`` and of every ``output_blocks[i]``, in that order -- not taken from the package under test.
"""

from __future__ import annotations

import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)  # installs the import shims and imports the reference
sys.path.insert(0, os.path.join(HERE, ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from dropout_common import FIXTURE_P, FIXTURE_SEED, FIXTURE_STEP, keep_mask, scale_of  # noqa: E402

from oracle import synth  # noqa: E402


WIDE_NUMEL = 10000


class MaskedDropout(torch.nn.Module):
    """x [B, C, *spatial] * keep(site) * float32(1 / (1 - p)), keep indexed over the [B * pixels, C] token rows"""

    def __init__(self, site: int, p: float) -> None:
        super().__init__()
        self.site, self.p, self.calls = site, p, 0

    def forward(self, x):
        B, C = x.shape[0], x.shape[1]
        n = x[0, 0].numel()
        keep = keep_mask(B * n, C, FIXTURE_SEED, FIXTURE_STEP, self.site, self.p).reshape(B, n, C).transpose(0, 2, 1)
        self.calls += 1
        return x * (torch.from_numpy(np.ascontiguousarray(keep)).reshape(x.shape).to(x.dtype) * float(scale_of(self.p)))


def install_masks(m, p: float) -> dict[str, int]:
    sites: dict[str, int] = {}
    site = 0
    groups = ([(f"input_blocks.{i}.", g) for i, g in enumerate(m.input_blocks)] + [("middle_block.", m.middle_block)]
              + [(f"output_blocks.{i}.", g) for i, g in enumerate(m.output_blocks)])
    for gp, grp in groups:
        for j, mod in enumerate(grp):
            if isinstance(mod, mg.ResBlock):
                assert isinstance(mod.out_layers[2], torch.nn.Dropout) and mod.out_layers[2].p == p
                mod.out_layers[2] = MaskedDropout(site, p)
                sites[f"{gp}{j}."] = site
            elif isinstance(mod, mg.AttentionBlock):
                assert isinstance(mod.to_out[1], torch.nn.Dropout) and mod.to_out[1].p == p
                mod.to_out[1] = MaskedDropout(site, p)
                sites[f"{gp}{j}."] = site
            site += 1
    return sites


def gen() -> None:
    p = FIXTURE_P
    cfg = mg.UNET_SMALL
    kw = dict(image_size=list(cfg.image_size), in_channels=cfg.in_channels, model_channels=cfg.model_channels,
              out_channels=cfg.out_channels, num_res_blocks=cfg.num_res_blocks, attention_resolutions=list(cfg.attention_resolutions),
              channel_mult=", ".join(map(str, cfg.channel_mult)), num_heads=cfg.num_heads, use_scale_shift_norm=cfg.use_scale_shift_norm,
              resblock_updown=cfg.resblock_updown, conv_resample=cfg.conv_resample, n_classes=cfg.n_classes,
              classifier_free=cfg.classifier_free)
    m = mg.UNetModel(dropout=p, **kw)
    P = synth.generic_params(mg.ounet.param_shapes(cfg), seed=23)
    assert set(m.state_dict()) == set(P)
    m.load_state_dict(P)
    m.train()
    sites = install_masks(m, p)
    masks = [mod for mod in m.modules() if isinstance(mod, MaskedDropout)]
    # (AttentionBlock.dropout, unet.py:267, is never called: whatever nn.Dropout is left in the tree must not be reached)
    left = [mod for mod in m.modules() if isinstance(mod, torch.nn.Dropout)]
    hits = []
    for mod in left:
        mod.register_forward_hook(lambda *_: hits.append(1))

    B = 4
    x0 = synth.normal("un.x0", (B, 1, 16, 16))
    noise = synth.normal("un.noise", (B, 1, 16, 16))
    yl = synth.integers("un.y", (B,), 10)
    ti = torch.tensor([3, 500, 999, 0], dtype=torch.int32)
    gd = mg.Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    xt = gd.diffusion.add_noise(x0, ti, noise)[0]
    o: dict = {"p": np.float64(p), "seed": np.int64(FIXTURE_SEED), "step": np.int64(FIXTURE_STEP),
               "site_prefixes": np.array(list(sites)), "site_ids": np.array(list(sites.values()), dtype=np.int64)}
    o["un_pred"] = m(x=xt, timesteps=ti, y=yl, p=0.0)["x"].detach()
    assert m.training
    loss = gd.compute_loss({"x": x0.clone(), "y": yl, "p": 0.0}, timesteps=ti, noise=noise)["loss"]
    loss.backward()
    assert m.training and not hits and all(mod.calls == 2 for mod in masks), (hits, [mod.calls for mod in masks])
    o["un_loss"] = loss
    names, norms = [], []
    for n, q in m.named_parameters():
        if q.grad is not None:
            names.append(n)
            norms.append(q.grad.double().norm().item())
            if q.grad.numel() <= 20000:
                o["un_g_" + n] = q.grad
    o["un_grad_names"], o["un_grad_norms"] = np.array(names), np.array(norms)
    base = np.load(os.path.join(HERE, "unet.npz"))["un_pred"]
    d = np.linalg.norm(o["un_pred"].double().numpy() - base.astype(np.float64)) / np.linalg.norm(base.astype(np.float64))
    print(f"{len(sites)} sites: {sites}\nloss {loss.item():.6f}; relative L2 distance of the prediction to the p = 0 fixture: {d:.4f}")
    # the same entries as the `un_*` part of unet.npz; they do not compress, and a committed file stays below 1 MiB: the gradient
    # tensors above WIDE_NUMEL elements go into a second file (the tests merge the two)
    wide = {k: o.pop(k) for k in [k for k, v in o.items() if k.startswith("un_g_") and v.numel() > WIDE_NUMEL]}
    mg.save("unet_dropout", **o)
    mg.save("unet_dropout_wide", **wide)


if __name__ == "__main__":
    gen()
