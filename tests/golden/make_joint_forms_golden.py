"""Generate tests/golden/joint_forms.npz by IMPORTING THE REAL REFERENCE: ``MMDiT`` / ``SprintDiT`` / ``DDT`` in their joint text-image
forms behind a two-output context embedder (token embeddings + one pooled vector per sample -> ``mlp_pooled_context``), and the joint
``DDT`` with ``MMDiTSingleStreamBlock`` encoder layers.

Runs only in the build container (the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_joint_forms_golden.py

Like make_golden.py (whose import shims this script reuses by loading it), only OUTPUTS of the reference are stored: weights come
from ``oracle.synth.generic_params`` over the reference model's own ``state_dict`` shapes, inputs from the named ``oracle.synth`` draws
of tests/joint_forms_common.py (the case table and the embedder live there, shared with the tests), and the tests regenerate both.
Per case, two legs: fp32, and ``torch.autocast("cpu", bfloat16)`` (the bf16 yardstick: the relative error of the reference's own
autocast run against its fp32 run, per tensor).  Per parameter: the gradient of sum(pred * g) -- whole up to 768 elements, else a
fixed sample of 384 elements (joint_forms_common.sample_index) -- and the norm of the whole gradient.
"""

from __future__ import annotations

import contextlib
import importlib
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name: str, path: str):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


mg = _load("make_golden", os.path.join(HERE, "make_golden.py"))  # installs the import shims and imports the reference
jc = _load("joint_forms_common", os.path.join(HERE, "..", "joint_forms_common.py"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from diffulab.networks.embedders.common import ContextEmbedder  # noqa: E402

from oracle import synth  # noqa: E402

CLASSES = {"MMDiT": ("diffulab.networks.denoisers.mmdit", "MMDiT"), "SprintDiT": ("diffulab.networks.denoisers.sprint", "SprintDiT"),
           "DDT": ("diffulab.networks.denoisers.ddt", "DDT")}


@contextlib.contextmanager
def injected_scores(scores: torch.Tensor):
    """the token scores of SprintDiT.drop_tokens (sprint.py:343, the only torch.rand of a p = 0 training forward) are the named draw"""
    real = torch.rand

    def rand(*size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        assert shape == tuple(scores.shape), shape
        return scores.clone()

    torch.rand = rand
    try:
        yield
    finally:
        torch.rand = real


def gen() -> None:
    out: dict = {"cases_json": np.array(jc.cases_json()), "mask_lengths": np.array(jc.MASK_LENGTHS),
                 "shape_b_lc_cctx_cpool": np.array([jc.B, jc.LC, jc.C_CTX, jc.C_POOL]),
                 "store_rule": np.array([jc.FULL_BELOW, jc.SAMPLE])}
    inp = jc.inputs(synth)
    rel = lambda a, b: ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()  # noqa: E731
    for tag, (cls, kw, pooled, seed) in jc.CASES.items():
        mod, name = CLASSES[cls]
        Model = getattr(importlib.import_module(mod), name)
        ctx = jc.context_of(inp, pooled)
        legs = {}
        for leg in ("fp32", "autocast"):
            m = Model(context_embedder=jc.make_embedder(ContextEmbedder, inp, pooled), **kw)
            shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
            m.load_state_dict(synth.generic_params(shapes, seed=seed))
            m.train()
            with torch.autocast("cpu", dtype=torch.bfloat16, enabled=leg == "autocast"), \
                    (injected_scores(inp["scores"]) if cls == "SprintDiT" else contextlib.nullcontext()):
                pred = m(x=inp["x"], timesteps=inp["t"], initial_context=ctx, p=0.0)["x"].float()
            (pred * inp["g"]).sum().backward()
            legs[leg] = (pred.detach(), {n: (p.grad.detach().float().clone() if p.grad is not None else torch.zeros_like(p))
                                         for n, p in m.named_parameters()})
        f32, ac = legs["fp32"], legs["autocast"]
        names = list(f32[1])
        o = {"sd_names": np.array(list(shapes)), "sd_shapes": np.array([",".join(map(str, s)) for s in shapes.values()]),
             "pred": f32[0], "ac_pred_err": np.float64(rel(ac[0], f32[0])), "names": np.array(names),
             "grad_norms": np.array([f32[1][n].double().norm().item() for n in names]),
             "ac_err": np.array([rel(jc.stored(ac[1][n]), jc.stored(f32[1][n])) for n in names])}
        for n in names:
            o["g_" + n] = jc.stored(f32[1][n])
        assert all(bool(torch.isfinite(v).all()) for v in (f32[0], ac[0], *f32[1].values(), *ac[1].values())), tag
        nz = o["grad_norms"] > 1e-6 * o["grad_norms"].max()
        print(f"{tag}: {len(names)} parameters ({int((~nz).sum())} with a zero gradient: {[n for n, k in zip(names, nz) if not k]}); "
              f"autocast prediction error {o['ac_pred_err']:.3e}; per-tensor gradient error median {np.median(o['ac_err'][nz]):.3e} "
              f"max {o['ac_err'][nz].max():.3e}")
        out.update({f"{tag}_{k}": v for k, v in o.items()})
    mg.save("joint_forms", **out)


if __name__ == "__main__":
    gen()
