"""GPU tests of the ODE likelihood of a rectified-flow model: the two row kernels (`dl_hutchinson_step`, `dl_normal_nll_rows`) against
fp64 with the bounds of tests/flow_nll_common.py, `Flow.calc_nll_loop` against the restatement of that file (a stub denoiser, then the
closed-form Gaussian model against its exact likelihood), `Diffuser.evaluate_nll` through the DiT in both precision regimes against
the oracle (the three legs of tests/test_parity_bf16_gpu.py), the trainer's val_nll_batches and the example."""

import json
import math
import os
import subprocess
import sys

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

import flow_nll_common as fn  # noqa: E402
import guidance_common as gc  # noqa: E402
import multistep_common as mc  # noqa: E402
from oracle import dit as odit  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
S2 = dict(input_channels=4, output_channels=4, inner_dim=384, embedding_dim=384, num_heads=6, mlp_ratio=4, patch_size=2, depth=12,
          n_classes=1000, classifier_free=True)
SMALL = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2, depth=2,
             n_classes=10, classifier_free=True)
GRAD_BOUND, FACTOR, TOL = 1e-2, 1.5, 1e-5
F32_BAR = 1e-5  # the project's f32-class bar (relative L2)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------------------------ the row kernels
@pytest.mark.parametrize("rows", [1, 3, 256])
@pytest.mark.parametrize("chw", [1, 63, 1024, 4096, 4097, 12293])
def test_row_kernels_against_fp64(rows, chw):
    from diffulab_amd import ops

    tag = f"nll.rows.{rows}.{chw}"
    g, x, v, v0 = (synth.normal(f"{tag}.{k}", (rows, chw)) for k in ("g", "x", "v", "v0"))
    eps = fn.rademacher((rows, chw), 7).float()
    a, b, scale, cols, col = 0.25, -0.125, 1.0 / chw, 5, 2
    dv = {k: t.to(DEV) for k, t in dict(g=g, x=x, v=v, v0=v0, eps=eps).items()}
    for mode in ("sums", "step", "step_v0"):
        xo_ref, xb, s_ref, sb = fn.hutchinson_step(x if mode != "sums" else None, v, v0 if mode == "step_v0" else None, a, b, g, eps, scale)
        runs = []
        for _ in range(2):
            table = torch.full((rows, cols), 7.5, device=DEV)
            x_out = torch.full((rows, chw), 7.5, device=DEV) if mode != "sums" else None
            kw = {} if mode == "sums" else dict(x=dv["x"], v=dv["v"], a=a, x_out=x_out)
            if mode == "step_v0":
                kw.update(v0=dv["v0"], b=b)
            ops.hutchinson_step(dv["g"], dv["eps"], table, col, scale, **kw)
            torch.cuda.synchronize()
            runs.append((table.clone(), None if x_out is None else x_out.clone()))
        table, x_out = runs[0]
        keep = [c for c in range(cols) if c != col]
        assert bool((table[:, keep] == 7.5).all()), "a neighbouring column was written"
        worst = ((table[:, col].double().cpu() - s_ref).abs() / sb).max().item()
        assert worst <= 1.0, (tag, mode, worst)
        if x_out is not None:
            wx = ((x_out.double().cpu() - xo_ref).abs() / xb).max().item()
            assert wx <= 1.0, (tag, mode, wx)
            assert torch.equal(runs[0][1], runs[1][1])
        assert torch.equal(runs[0][0], runs[1][0]), "two runs differ"
    val, nb = fn.normal_nll_rows(x)
    o1, o2 = ops.normal_nll_rows(dv["x"]), ops.normal_nll_rows(dv["x"])
    torch.cuda.synchronize()
    assert ((o1.double().cpu() - val).abs() / nb).max().item() <= 1.0 and torch.equal(o1, o2)
    # in place: x_out may be x
    xi = dv["x"].clone()
    table = torch.zeros(rows, 1, device=DEV)
    ops.hutchinson_step(dv["g"], dv["eps"], table, 0, scale, x=xi, v=dv["v"], a=a, x_out=xi)
    xo_ref, xb, _, _ = fn.hutchinson_step(x, v, None, a, b, g, eps, scale)
    assert ((xi.double().cpu() - xo_ref).abs() / xb).max().item() <= 1.0


# ------------------------------------------------------------------------------------------------------------------ loop vs restatement
@pytest.mark.parametrize("method", ["euler", "heun"])
@pytest.mark.parametrize("K", [1, 2])
def test_loop_against_the_restatement(method, K):
    from diffulab_amd import Diffuser

    B, shape = 3, (3, 2, 8, 8)
    x0 = synth.uniform("nll.loop.x0", shape, lo=-1.0, hi=1.0)
    y = synth.integers("nll.loop.y", (B,), 10)
    probes = fn.rademacher((K, *shape), 21)
    u = synth.uniform("nll.loop.u", shape, lo=0.0, hi=0.999)
    stub = gc.Stub(1.0).to(DEV)
    d = Diffuser(stub, sampling_method="euler", model_type="rectified_flow", n_steps=4)
    inputs = {"x": x0.to(DEV), "y": y.to(DEV)}
    out = d.evaluate_nll(inputs, method=method, probes=probes, dequant_noise=u)
    assert list(inputs) == ["x", "y"] and torch.equal(inputs["x"].cpu(), x0) and not inputs["x"].requires_grad
    assert stub.calls == (8 if method == "heun" else 4)
    ref_stub = gc.Stub(1.0).double()
    field = lambda x, t: ref_stub(x=x, timesteps=torch.full((x.shape[0],), t, dtype=torch.float64), y=y.double().repeat(K))["x"]  # noqa: E731
    ref = fn.nll_loop(field, x0, d.diffusion.timesteps, method, probes, dequant_noise=u)
    assert set(out) == set(ref)
    for k in ref:
        assert out[k].dtype == torch.float32 and out[k].device.type == "cuda" and out[k].shape == ref[k].shape, k
        e = rel(out[k], ref[k])
        print(f"{method} K={K} {k}: rel-L2 {e:.2e}")
        assert e <= F32_BAR, (k, e)
    if K == 2:  # drawn probes: the same shapes, finite, and n_probes is honoured
        for probe in ("rademacher", "gaussian"):
            o = d.evaluate_nll(inputs, method=method, n_probes=2, probe=probe)
            assert o["div_terms"].shape == ref["div_terms"].shape and bool(torch.isfinite(o["nll"]).all())


class _ClosedForm(nn.Module):
    """the exact velocity field of data N(M, S^2) per element (tests/multistep_common.py)"""

    def __init__(self):
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1))

    def forward(self, x, timesteps, p=0, **kw):
        t = timesteps.to(x.dtype).view(-1, *([1] * (x.dim() - 1)))
        V = (1 - t) ** 2 * mc.S * mc.S + t * t
        return {"x": -mc.M + (t - (1 - t) * mc.S * mc.S) / V * (x - (1 - t) * mc.M)}


def test_closed_form_model_on_the_device():
    from diffulab_amd import Diffuser

    g = torch.Generator().manual_seed(11)
    x0 = (mc.M + mc.S * torch.randn(8, 1, 8, 8, generator=g, dtype=torch.float64)).float()
    d = Diffuser(_ClosedForm().to(DEV), sampling_method="euler", model_type="rectified_flow", n_steps=40)
    out = d.evaluate_nll({"x": x0.to(DEV)}, method="heun", dequantize=False)
    exact = fn.gaussian_nll(x0) / fn.LN2 + math.log2(127.5)
    err = (out["total_bpd"].double().cpu() - exact).abs().max().item()
    print(f"closed-form model, Heun 40 steps on the device: worst error {err:.2e} bits/dim")
    assert err <= 1e-3


# ------------------------------------------------------------------------------------------------------------------ through the DiT
def _oracle_field(P, cfg, y, autocast):
    def field(x, t):
        tt = torch.full((x.shape[0],), t, dtype=torch.float32)
        yy = y.repeat(x.shape[0] // y.shape[0])
        if autocast:
            with odit.bf16_autocast():
                return odit.dit_forward(P, x, tt, yy, cfg).float()
        return odit.dit_forward(P, x, tt, yy, cfg)
    return field


CASES = [("small", SMALL, 5, 4, 16, 4), ("s2", S2, 7, 2, 32, 2)]
_legs_cache: dict = {}


def _case(name, cfgk, seed, B, H, steps):
    """inputs and the two oracle legs of a case, computed once and shared by the two precision regimes"""
    if name not in _legs_cache:
        cfg = odit.DiTConfig(**cfgk)
        P = synth.dit_params(odit.param_shapes(cfg), seed=seed)
        shape = (B, cfgk["input_channels"], H, H)
        x0 = synth.uniform(f"nll.{name}.x0", shape, lo=-1.0, hi=1.0)
        y = synth.integers(f"nll.{name}.y", (B,), cfgk["n_classes"])
        probes = fn.rademacher((1, *shape), 31).float()
        u = synth.uniform(f"nll.{name}.u", shape, lo=0.0, hi=0.999)
        grid = torch.linspace(1, 0, steps + 1).tolist()
        legs = {ac: fn.nll_loop(_oracle_field(P, cfg, y, ac), x0, grid, "heun", probes, dequant_noise=u, dtype=torch.float32)
                for ac in (False, True)}
        _legs_cache[name] = (P, x0, y, probes, u, legs[False], legs[True])
    return _legs_cache[name]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name,cfgk,seed,B,H,steps", CASES, ids=[c[0] for c in CASES])
def test_evaluate_nll_through_the_dit(name, cfgk, seed, B, H, steps, precision):
    from diffulab_amd import Diffuser, MMDiT

    P, x0, y, probes, u, r32, rbf = _case(name, cfgk, seed, B, H, steps)
    m = MMDiT(simple_dit=True, **cfgk)
    m.load_state_dict(P)
    m.set_precision(precision)
    m = m.to(DEV)
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=steps)
    m.engine
    m._flat_grad.fill_(-3.25)  # trainable parameters: no p.grad may move
    before = m._flat_grad.clone()
    inputs = {"x": x0.to(DEV), "y": y.to(DEV)}
    out = d.evaluate_nll(inputs, method="heun", probes=probes, dequant_noise=u)
    torch.cuda.synchronize()
    assert torch.equal(m._flat_grad, before), "evaluate_nll wrote parameter gradients"
    assert list(inputs) == ["x", "y"] and torch.equal(inputs["x"].cpu(), x0) and torch.equal(inputs["y"].cpu(), y)
    assert out["div_terms"].shape == (B, 2 * steps)
    for k in ("div_terms", "x1"):
        e_hip, e_bf = rel(out[k], r32[k]), rel(rbf[k], r32[k])
        print(f"{name} {precision} {k}: rel-L2 hip {e_hip:.3e}, bf16-autocast oracle {e_bf:.3e}")
        assert e_hip <= (TOL if precision == "fp32" else max(GRAD_BOUND, FACTOR * e_bf)), (k, e_hip, e_bf)
    nll32 = r32["nll"].double()
    e_hip = (out["nll"].double().cpu() - nll32).abs()
    e_bf = (rbf["nll"].double() - nll32).abs()
    print(f"{name} {precision} nll {nll32.tolist()}: |error| hip {e_hip.tolist()}, bf16-autocast oracle {e_bf.tolist()}; "
          f"divergence part {r32['div'].tolist()}")
    if precision == "fp32":
        assert rel(out["nll"], r32["nll"]) <= TOL
    else:
        # every sample's error against max(1e-3 |nll|, 1.5 x the autocast leg's error); the leg's error is ONE figure per case, its
        # worst sample, like the relative L2 figures above: a sample's own autocast error is a draw that can fall anywhere below that
        # (S/2: 1.1e-4 and 1.5e-3 for the two samples), and the HIP path's rounding is not the oracle's sample by sample
        assert bool((e_hip <= torch.maximum(1e-3 * nll32.abs(), FACTOR * e_bf.max())).all()), (e_hip, e_bf)


# ------------------------------------------------------------------------------------------------------------------ trainer, example
def test_trainer_logs_nll_outside_the_checkpoint_criterion(tmp_path):
    from torch.utils.data import DataLoader

    from diffulab_amd import Diffuser, MMDiT
    from diffulab_amd.datasets import SyntheticDataset
    from diffulab_amd.training import BaseTrainer, FusedAdamW

    def go(name, **kw):
        torch.manual_seed(0)
        m = MMDiT(simple_dit=True, **SMALL)
        d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=2)
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
        mk = lambda n, seed: DataLoader(SyntheticDataset(n, (4, 16, 16), 10, seed), batch_size=16, drop_last=True)  # noqa: E731
        tr = BaseTrainer(n_epoch=1, save_path=tmp_path, project_name=name, use_ema=True, ema_update_after_step=0, ema_update_every=1)
        tr.train(diffuser=d, optimizer=opt, train_dataloader=mk(32, 1), val_dataloader=mk(32, 2), log_validation_images=False,
                 p_classifier_free_guidance=0.1, **kw)
        rows = [json.loads(ln) for ln in (tmp_path / name / "metrics.jsonl").read_text().splitlines()]
        return tr, {k: v for r in rows for k, v in r.items() if k.startswith("val/")}

    tr, val = go("with", val_nll_batches=1, val_nll_args={"method": "euler"})
    print(val)
    assert {"val/loss", "val/nll", "val/bpd"} <= set(val) and all(math.isfinite(val[k]) for k in ("val/nll", "val/bpd"))
    assert abs(val["val/bpd"] - (val["val/nll"] / math.log(2.0) + math.log2(127.5))) <= 1e-4
    crit = sum(v for k, v in val.items() if k not in ("val/nll", "val/bpd"))
    assert abs(tr.val_total - crit) <= 1e-9 * abs(crit)
    tr0, val0 = go("without")
    assert "val/nll" not in val0 and "val/bpd" not in val0
    assert abs(tr0.val_total - sum(val0.values())) <= 1e-9 * abs(sum(val0.values()))


def test_the_example_runs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "evaluate_nll.py"), "--train-steps", "4", "--steps", "2", "4",
                        "--batch", "4", "--probes", "1"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("bits/dim") == 8 and "heun    4 steps (  8 evaluations)" in r.stdout and "trained 4 steps" in r.stdout
