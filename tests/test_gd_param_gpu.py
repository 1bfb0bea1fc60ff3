"""GPU tests of the x0 / x_prev / v training targets: the loss head of every parameterisation (dl_gd_loss_fwd / _bwd, with and without
min-SNR weights, fixed and learned variances), the v-prediction sampler steps (dl_ddpm_step_v, dl_ddim_step_v) and the host layers
over them (gd_head, DDPM / DDIM with mean_type="v", GaussianDiffusion with loss_target / loss_weighting).

Expected values: the f64 evaluation of tests/gd_param_common.py on the same f32 inputs; the reference's own step outputs where it has
the parameterisation (tests/golden/gd_targets.npz); the bits of dl_mse_loss_* / dl_vlb_loss_* where the new head generalises them.

Loss tolerance: the rule of tests/test_learned_variance_gpu.py.  The kernel and the f32 CPU evaluation of the restatement are both f32
evaluations of the same formulas on the same inputs, so the f32 CPU evaluation's own error against f64 is measured per case and the
kernel is allowed twice that plus the 3e-6 this suite grants f32 element-wise kernels: relative for the scalars; for dpred, per half,
every element within 2 * max|f32 - f64| + 3e-6 * max|f64|.  DDPM steps: relative-L2 3e-6 against the f64 evaluation, as every step
test here.  DDIM steps: the same rule as the loss, per output array, against the f64 evaluation -- DDIM's sigma holds
1 - ab / ab_prev, a difference of neighbours that f32 resolves coarsely at small t whatever evaluates it, so the f32 CPU evaluation's
own error is measured (and printed) instead of assumed, and the kernel gets twice that plus 3e-6 of the array's maximum.
Measured figures: DESIGN.md section 2.
"""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as eb  # noqa: E402
import gd_param_common as gp  # noqa: E402
import learned_variance_common as lv  # noqa: E402
from oracle import diffusion as od  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (3, 4, 8, 8)


def rel(a, b):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().double().cpu() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b)).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def clean(t):
    return torch.nan_to_num(t.detach().double().cpu(), 0, 0, 0)  # DDIM's logprob at t == 0: sigma == 0, in the reference too


def within_f32_rule(got, f32, f64, tag):
    """every element of `got` within 2 * max|f32 - f64| + 3e-6 * max|f64| of the f64 evaluation"""
    got, f32, f64 = clean(got), clean(f32), clean(f64)
    e32 = float((f32 - f64).abs().max())
    bound = 2 * e32 + 3e-6 * float(f64.abs().max())
    err = float((got - f64).abs().max())
    print(f"{tag}: max|f64| {float(f64.abs().max()):.3e}  f32-cpu max err {e32:.3e}  kernel max err {err:.3e}  bound {bound:.3e}")
    assert got.shape == f64.shape and err <= bound, (tag, err, bound)


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def T():
    return od.GaussianTables(1000)


def var_mode(ops, var_type):
    return ops.VAR_FIXED if var_type == "fixed" else ops.VAR_MODES[var_type]


_CASES = {}


def device_case(T, name, var_type, case="small"):
    """the f32 inputs of one loss case, on the CPU and on the device, built once per module"""
    key = (name, var_type, case)
    if key not in _CASES:
        c = gp.loss_case(T, name, var_type, case)
        _CASES[key] = (c, {k: c[k].to(DEV) for k in ("pred", "eps", "x0", "xt", "t", "tab")})
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------------ loss vs f64
LOSS_PARAMS = [(case, n, vt, wn) for case in gp.LOSS_CASES for n in gp.TARGETS for vt in gp.VAR_TYPES for wn in ("unweighted", "min_snr")
               if (n, wn) != ("xprev", "min_snr")]


@pytest.mark.parametrize("case,name,var_type,weighting", LOSS_PARAMS)
def test_loss_forward_and_backward(ops, T, case, name, var_type, weighting):
    c, d = device_case(T, name, var_type, case)
    w = gp.weightings(T, name)[weighting]
    args = (c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], name, var_type, w)
    g_mse, g_vb = 0.75, 1.25
    ref = dict(zip(("mse", "vb"), gp.loss(*args)), dpred=gp.loss_backward(*args, g_mse=g_mse, g_vb=g_vb))
    f32 = dict(zip(("mse", "vb"), gp.loss(*args, dtype=torch.float32)),
               dpred=gp.loss_backward(*args, g_mse=g_mse, g_vb=g_vb, dtype=torch.float32))
    assert f32["dpred"].dtype == torch.float32 and f32["mse"].dtype == torch.float32

    tgt, vm = ops.MEAN_TYPES[name], var_mode(ops, var_type)
    wd = None if w is None else w.to(DEV)
    dev = (d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], tgt, wd, vm)
    out = ops.gd_loss_fwd(*dev)
    again = ops.gd_loss_fwd(*dev)
    assert out.shape == (() if var_type == "fixed" else (2,))
    assert torch.equal(bits(out), bits(again))  # fixed-order partials: bit-identical across runs
    gm, gv = torch.tensor(g_mse, device=DEV), torch.tensor(g_vb, device=DEV)
    dpred = ops.gd_loss_bwd(*dev, gm, gv)
    assert dpred.shape == c["pred"].shape

    tag = f"{case} {name}/{var_type}/{weighting}"
    scalars = out.reshape(-1).cpu()
    for i, k in enumerate(("mse", "vb")[:scalars.numel()]):
        e32 = abs(float(f32[k]) - float(ref[k])) / abs(float(ref[k]))
        got = abs(float(scalars[i]) - float(ref[k])) / abs(float(ref[k]))
        print(f"{tag} {k}: ref {float(ref[k]):.9g}  f32-cpu rel err {e32:.3e}  kernel rel err {got:.3e}  bound {2 * e32 + 3e-6:.3e}")
        assert got <= 2 * e32 + 3e-6, (k, got, e32)
    C = c["x0"].shape[1]
    halves = (("mean half", slice(0, C)),) if var_type == "fixed" else (("mean half", slice(0, C)), ("variance half", slice(C, 2 * C)))
    for hname, sl in halves:
        r, a = ref["dpred"][:, sl], f32["dpred"][:, sl].double()
        e32 = float((a - r).abs().max())
        bound = 2 * e32 + 3e-6 * float(r.abs().max())
        err = (dpred[:, sl].double().cpu() - r).abs()
        print(f"{tag} dpred {hname}: max|ref| {float(r.abs().max()):.3e}  f32-cpu max err {e32:.3e}  kernel max err "
              f"{float(err.max()):.3e}  bound {bound:.3e}")
        assert bool(torch.isfinite(dpred[:, sl]).all()) and int((err > bound).sum()) == 0, (hname, float(err.max()), bound)


# ------------------------------------------------------------------------------------------------------------------ bit equality
@pytest.mark.parametrize("case", list(gp.LOSS_CASES))
def test_epsilon_fixed_unweighted_is_the_plain_mse_head_bit_for_bit(ops, T, case):
    c, d = device_case(T, "epsilon", "fixed", case)
    gm = torch.tensor(0.75, device=DEV)
    want = ops.mse_loss_fwd(d["pred"], d["eps"], None, ops.LOSS_EPS)
    want_b = ops.mse_loss_bwd(d["pred"], d["eps"], None, 1.0, ops.LOSS_EPS, gscale_dev=gm)
    for x0, xt in ((d["x0"], d["xt"]), (None, None)):  # the epsilon / fixed form touches neither x0 nor xt
        got = ops.gd_loss_fwd(d["pred"], d["eps"], x0, xt, d["t"], d["tab"], 0, None, ops.VAR_FIXED)
        got_b = ops.gd_loss_bwd(d["pred"], d["eps"], x0, xt, d["t"], d["tab"], 0, None, ops.VAR_FIXED, gm, None)
        assert torch.equal(bits(got), bits(want)) and torch.equal(bits(got_b), bits(want_b))
    # and a weight table of ones is the same loss to rounding, through the weighted kernel
    ones = torch.ones(1000, device=DEV)
    weighted = ops.gd_loss_fwd(d["pred"], d["eps"], None, None, d["t"], d["tab"], 0, ones, ops.VAR_FIXED)
    assert abs(float(weighted) - float(want)) <= 1e-6 * float(want)
    assert torch.equal(bits(ops.gd_loss_bwd(d["pred"], d["eps"], None, None, d["t"], d["tab"], 0, ones, ops.VAR_FIXED, gm, None)), bits(want_b))


@pytest.mark.parametrize("var_type", lv.VAR_TYPES)
@pytest.mark.parametrize("mean_type", lv.MEAN_TYPES)
def test_learned_variance_unweighted_is_the_hybrid_head_bit_for_bit(ops, T, mean_type, var_type):
    """dl_vlb_loss_* regresses its mean half on whatever tensor it is given as `eps` and derives the bound's mean by `mean_type`;
    dl_gd_loss_* forms the regression target of `mean_type` itself.  So the hybrid head is handed the target as a tensor: eps and x0
    as they are, the posterior mean as the fixed-variance step kernel writes it for the prediction x0 (its `mean` output, no clamp)."""
    for case in gp.LOSS_CASES:
        c, d = device_case(T, mean_type, var_type, case)
        mt, vm = ops.MEAN_TYPES[mean_type], ops.VAR_MODES[var_type]
        if mean_type == "xprev":
            tgt = ops.ddpm_step(d["x0"], None, 0.0, d["xt"], torch.zeros_like(d["xt"]), d["t"], gp.fixed_tables(T).to(DEV), 1, False)[2]
        else:
            tgt = d["eps"] if mean_type == "epsilon" else d["x0"]
        gm, gv = torch.tensor(0.75, device=DEV), torch.tensor(1.25, device=DEV)
        want = ops.vlb_loss_fwd(d["pred"], tgt, d["x0"], d["xt"], d["t"], d["tab"], mt, vm)
        want_b = ops.vlb_loss_bwd(d["pred"], tgt, d["x0"], d["xt"], d["t"], d["tab"], mt, vm, gm, gv)
        got = ops.gd_loss_fwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], mt, None, vm)
        got_b = ops.gd_loss_bwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], mt, None, vm, gm, gv)
        assert torch.equal(bits(got), bits(want)), (case, got.tolist(), want.tolist())
        C = c["x0"].shape[1]
        assert torch.equal(bits(got_b[:, :C]), bits(want_b[:, :C])) and torch.equal(bits(got_b[:, C:]), bits(want_b[:, C:])), case


# ------------------------------------------------------------------------------------------------------------------ perfect prediction
def _exact_prediction(T, chain_t, x0, eps, xt, mean_type, learned):
    """the exact target of `mean_type`, built on the CPU in f32 from the tables the kernels read"""
    rows = gp._rows(gp.fixed_tables(T), chain_t, xt, torch.float32)
    tgt = gp.target(rows, eps, x0, xt, mean_type)
    pred = torch.cat([tgt, synth.uniform("gdp.v", tuple(tgt.shape), lo=-1.0, hi=1.0)], dim=1) if learned else tgt
    return tgt, pred.contiguous()


@pytest.mark.parametrize("var_type", ["fixed_small", "learned_range"])
@pytest.mark.parametrize("mean_type", gp.TARGETS)
@pytest.mark.parametrize("chain", list(gp.CHAINS))
def test_perfect_prediction_ties_the_loss_to_the_sampler(golden, monkeypatch, chain, mean_type, var_type):
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion
    from diffulab_amd.diffuse.samplers.gaussian_diffusion import DDIM, DDPM

    g = golden("gd_targets")
    Tc, t = gp.chain(chain)
    x0, eps = gp.fixture_inputs()
    xt = torch.from_numpy(g[f"{chain}_xt"])
    learned = var_type == "learned_range"
    tgt, pred = _exact_prediction(Tc, t, x0, eps, xt, mean_type, learned)
    pred_dev = pred.to(DEV)
    sp = {"mean_type": mean_type, "var_type": var_type}
    gd = GaussianDiffusion(n_steps=1000, sampler_parameters=sp, loss_target="mean_type")
    if chain != "full":
        gd.set_steps(gp.CHAINS[chain][0])
    assert torch.equal(gd.betas, Tc.betas)
    out = gd.compute_loss(lambda **kw: {"x": pred_dev}, {"x": x0.to(DEV)}, t, eps.to(DEV))
    bound = (3e-6) ** 2 * float((tgt.double() ** 2).mean())
    print(f"{chain} {mean_type}/{var_type}: loss {float(out['loss']):.3e}  bound {bound:.3e}")
    assert set(out) == ({"loss", "vb"} if learned else {"loss"}) and float(out["loss"]) <= bound
    # the sampler reads the same tensor back as the posterior mean of (x0, xt)
    rows = gp._rows(gp.fixed_tables(Tc), t, xt, torch.float64)
    want = gp.posterior_mean(rows, x0.double(), xt.double())
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: torch.zeros(ref.shape, device=ref.device, dtype=ref.dtype))
    s = DDPM(**sp)
    s.set_steps(Tc.betas.clone())
    r = s.step(pred_dev, t.to(DEV), xt.to(DEV))
    e = rel(r["x_prev_mean"], want)
    print(f"{chain} {mean_type}/{var_type}: DDPM x_prev_mean rel err {e:.3e}")
    assert e < 3e-6
    if mean_type in gp.REFERENCE_TARGETS:
        assert rel(r["x_prev_mean"], g[f"{chain}_{mean_type}_x_prev_mean"]) < 3e-6
    # DDIM: the mean of its own posterior q_sigma(x_{t-1} | x_t, x0) (ddim.py:68-103) at the true x0
    s = DDIM(**sp)
    s.set_steps(Tc.betas.clone())
    for eta in (0.0, 0.5):
        r = s.step(pred_dev, t.to(DEV), xt.to(DEV), eta=eta)
        want = gp.ddim_step(gp.ddim_tables(Tc), x0, t, xt, torch.zeros_like(xt), eta, dtype=torch.float64)["x_prev_mean"]
        e = rel(r["x_prev_mean"], want)
        print(f"{chain} {mean_type}/{var_type}: DDIM eta {eta} x_prev_mean rel err {e:.3e}")
        assert e < 3e-6


# ------------------------------------------------------------------------------------------------------------------ v steps
def step_inputs(var_type):
    xt = synth.normal("smp.xt", SHAPE)
    o = synth.normal("smp.v", SHAPE)
    pred = o if var_type == "fixed" else torch.cat([o, synth.normal("smpl.var", SHAPE)], dim=1)
    return xt, pred.contiguous(), torch.tensor([0, 7, 999], dtype=torch.int32)


def step_tables(T, var_type):
    return gp.fixed_tables(T) if var_type == "fixed" else lv.tables(T)


@pytest.mark.parametrize("var_type", gp.VAR_TYPES)
def test_v_steps_against_the_restatement(ops, T, monkeypatch, var_type):
    from diffulab_amd.diffuse.samplers.gaussian_diffusion import DDIM, DDPM

    xt, pred, tt = step_inputs(var_type)
    nz = synth.normal("smp.noise", SHAPE)
    tab, tab3 = step_tables(T, var_type), gp.ddim_tables(T)
    d = [v.to(DEV) for v in (pred, xt, nz, tt, tab, tab3)]
    vm = var_mode(ops, var_type)
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: d[2])
    sp = {"mean_type": "v", "var_type": "fixed_small" if var_type == "fixed" else var_type}
    for clamp in (False, True):
        want = gp.ddpm_step_v(tab, pred, tt, xt, nz, var_type, clamp, dtype=torch.float64)
        outs = ops.ddpm_step_v(d[0], None, 0.0, d[1], d[2], d[3], d[4], vm, clamp)
        s = DDPM(**sp)
        s.set_steps(T.betas.clone())
        r = s.step(d[0], d[3], d[1], clamp_x=clamp)
        assert list(r) == list(gp.STEP_KEYS)
        for got, key in zip(outs, gp.STEP_KEYS):
            e = rel(got, want[key])
            print(f"ddpm_step_v {var_type} clamp {int(clamp)} {key}: rel err {e:.3e}")
            assert got.shape == xt.shape and e < 3e-6 and rel(r[key], want[key]) < 3e-6, (clamp, key)
        for eta in (0.0, 0.5):
            want = gp.ddim_step_v(tab3, pred, tt, xt, nz, eta, var_type, clamp, dtype=torch.float64)
            w32 = gp.ddim_step_v(tab3, pred, tt, xt, nz, eta, var_type, clamp, dtype=torch.float32)
            outs = ops.ddim_step_v(d[0], None, 0.0, d[1], d[2], d[3], d[5], vm, clamp, eta)
            s = DDIM(**sp)
            s.set_steps(T.betas.clone())
            r = s.step(d[0], d[3], d[1], clamp_x=clamp, eta=eta)
            assert set(r) == set(want)
            for got, key in zip(outs, gp.STEP_KEYS):
                if got is None:
                    assert eta == 0 and key in ("x_prev_std", "logprob")
                    continue
                tag = f"ddim_step_v {var_type} clamp {int(clamp)} eta {eta} {key}"
                within_f32_rule(got, w32[key], want[key], tag)
                within_f32_rule(r[key], w32[key], want[key], tag + " (DDIM.step)")


@pytest.mark.parametrize("var_type", gp.VAR_TYPES)
def test_cfg_fused_in_the_v_kernels_equals_combine_then_step(ops, T, var_type):
    xt, pred, tt = step_inputs(var_type)
    u = synth.normal("smpl.u", SHAPE)
    pu = u if var_type == "fixed" else torch.cat([u, synth.normal("smpl.uvar", SHAPE)], dim=1).contiguous()
    nz = synth.normal("smp.noise", SHAPE)
    comb = lv.cfg_combine(pred, pu, 1.5)
    tab, tab3 = step_tables(T, var_type), gp.ddim_tables(T)
    d = [v.to(DEV) for v in (pred, pu, xt, nz, tt, tab, comb, tab3)]
    vm = var_mode(ops, var_type)
    fused = ops.ddpm_step_v(d[0], d[1], 1.5, d[2], d[3], d[4], d[5], vm, True)
    plain = ops.ddpm_step_v(d[6], None, 0.0, d[2], d[3], d[4], d[5], vm, True)
    want = gp.ddpm_step_v(tab, comb, tt, xt, nz, var_type, True, dtype=torch.float64)
    for a, b, key in zip(fused, plain, gp.STEP_KEYS):
        assert rel(a, b) < 3e-6 and rel(a, want[key]) < 3e-6, (var_type, key)
    fused = ops.ddim_step_v(d[0], d[1], 1.5, d[2], d[3], d[4], d[7], vm, True, 0.5)
    plain = ops.ddim_step_v(d[6], None, 0.0, d[2], d[3], d[4], d[7], vm, True, 0.5)
    want = gp.ddim_step_v(tab3, comb, tt, xt, nz, 0.5, var_type, True, dtype=torch.float64)
    w32 = gp.ddim_step_v(tab3, comb, tt, xt, nz, 0.5, var_type, True, dtype=torch.float32)
    for a, b, key in zip(fused, plain, gp.STEP_KEYS):
        assert rel(clean(a), clean(b)) < 3e-6, (var_type, key)
        within_f32_rule(a, w32[key], want[key], f"ddim_step_v fused cfg {var_type} {key}")


# ------------------------------------------------------------------------------------------------------------------ write guards
@pytest.mark.parametrize("chw", [1, 63, 257])
def test_outputs_stay_inside_their_windows(ops, T, chw):
    B = 3
    n = B * chw
    tab3 = gp.ddim_tables(T).to(DEV)
    t = torch.tensor([0, 7, 999], dtype=torch.int32, device=DEV)
    xt, nz, eps = (synth.normal(f"gdg.{k}{chw}", (B, chw)).to(DEV) for k in ("xt", "nz", "eps"))
    x0 = synth.uniform(f"gdg.x0{chw}", (B, chw), lo=-1.0, hi=1.0).to(DEV)
    weight = gp.min_snr(T.alphas_bar, "v").float().to(DEV)

    def windows(k, cols=n):
        return [eb.Guarded(1, cols, torch.float32, DEV) for _ in range(k)]

    for var_type in gp.VAR_TYPES:
        vm = var_mode(ops, var_type)
        k = 1 if var_type == "fixed" else 2
        tab = step_tables(T, var_type).to(DEV)
        pred, pu = (synth.normal(f"gdg.{s}{chw}", (B, k * chw)).to(DEV) for s in ("pred", "pu"))
        w = windows(5)
        ops.ddpm_step_v(pred, pu, 1.5, xt, nz, t, tab, vm, True, out=[g.win for g in w])
        for g, key in zip(w, gp.STEP_KEYS):
            g.check(f"dl_ddpm_step_v {var_type} chw {chw}: {key}")
        w = windows(5)
        ops.ddim_step_v(pred, pu, 1.5, xt, nz, t[1:].repeat(2)[:3].contiguous(), tab3, vm, True, 0.5, out=[g.win for g in w])
        for g, key in zip(w, gp.STEP_KEYS):
            g.check(f"dl_ddim_step_v {var_type} chw {chw}: {key}")
        np_ = ops.lib().call("dl_mse_loss_partials", n)
        for target, wt in ((0, None), (1, None), (2, None), (3, weight)):
            w = windows(1, k) + windows(1, k * n) + windows(1, k * np_)  # loss, dpred, the forward's per-block partial sums
            ops.gd_loss_fwd(pred, eps, x0, xt, t, tab, target, wt, vm, out=w[0].win.view(k) if k == 2 else w[0].win[0, 0],
                            partial=w[2].win.view(k * np_))
            ops.gd_loss_bwd(pred, eps, x0, xt, t, tab, target, wt, vm, None, None, out=w[1].win)
            w[0].check(f"dl_gd_loss_fwd {var_type} target {target} chw {chw}")
            w[1].check(f"dl_gd_loss_bwd {var_type} target {target} chw {chw}")
            w[2].check(f"dl_gd_loss_fwd {var_type} target {target} chw {chw}: partial")


# ------------------------------------------------------------------------------------------------------------------ autograd routing
def test_gd_head_autograd_routes_the_upstream_gradients(ops, T):
    from diffulab_amd.diffuse.modelizations.diffusion import gd_head

    c, d = device_case(T, "v", "learned_range")
    w = gp.min_snr(T.alphas_bar, "v").float().to(DEV)
    pred = d["pred"].clone().requires_grad_(True)
    mse, vb = gd_head(pred, d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 3, w, 1)
    (mse + 0.5 * vb).backward()
    want = ops.gd_loss_bwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 3, w, 1, torch.tensor(1.0, device=DEV),
                           torch.tensor(0.5, device=DEV))
    assert torch.equal(bits(pred.grad), bits(want))
    pred.grad = None
    mse, vb = gd_head(pred, d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 3, w, 1)
    vb.backward()  # the bound alone: nothing reaches the mean half
    assert float(pred.grad[:, :3].abs().max()) == 0.0 and float(pred.grad[:, 3:].abs().max()) > 0.0
    # fixed variances: one scalar, one upstream gradient
    c, d = device_case(T, "v", "fixed")
    pred = d["pred"].clone().requires_grad_(True)
    loss = gd_head(pred, d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 3, w)
    assert loss.shape == ()
    (0.5 * loss).backward()
    want = ops.gd_loss_bwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 3, w, ops.VAR_FIXED, torch.tensor(0.5, device=DEV), None)
    assert torch.equal(bits(pred.grad), bits(want)) and float(pred.grad.abs().max()) > 0.0
    with torch.no_grad():
        assert torch.equal(bits(gd_head(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 3, w)), bits(loss.detach()))


# ------------------------------------------------------------------------------------------------------------------ end to end
def _unet(out_channels):
    from diffulab_amd.networks.denoisers import UNetModel

    return UNetModel(image_size=[16, 16], in_channels=1, model_channels=32, out_channels=out_channels, num_res_blocks=1,
                     attention_resolutions=[2], channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True,
                     n_classes=10, classifier_free=True)


def _dit(output_channels):
    from diffulab_amd import MMDiT

    return MMDiT(simple_dit=True, input_channels=4, output_channels=output_channels, inner_dim=128, embedding_dim=64, num_heads=2,
                 mlp_ratio=4, patch_size=2, depth=2, n_classes=10, classifier_free=True)


FAMILIES = {"unet": (_unet, 1, "out.2.weight"), "dit": (_dit, 4, "last_layer.linear.weight")}


@pytest.mark.parametrize("learned", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_v_prediction_train_step_and_sampling_end_to_end(family, learned):
    from diffulab_amd import Diffuser
    from diffulab_amd.training.optim import FusedAdamW

    torch.manual_seed(0)
    make, C, head = FAMILIES[family]
    m = make(2 * C if learned else C)
    with torch.no_grad():  # the output heads start at zero
        dict(m.named_parameters())[head].normal_(std=0.02)
    m = m.to(DEV)
    B = 4
    sp = {"mean_type": "v", "var_type": "learned_range" if learned else "fixed_small"}
    gd = Diffuser(m, model_type="gaussian_diffusion", sampling_method="ddpm", n_steps=1000,
                  extra_args={"sampler_parameters": sp, "loss_target": "mean_type", "loss_weighting": "min_snr"})
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    x0 = synth.uniform(f"gde.{family}", (B, C, 16, 16), lo=-1.0, hi=1.0).to(DEV)
    y = synth.integers("gde.y", (B,), 10).to(DEV)
    ti = torch.tensor([0, 5, 500, 999], dtype=torch.int32)
    inputs = {"x": x0.clone(), "y": y, "p": 0.0}
    losses = gd.compute_loss(inputs, timesteps=ti)
    assert set(losses) == ({"loss", "vb"} if learned else {"loss"})
    assert all(v.shape == () and bool(torch.isfinite(v)) for v in losses.values())
    assert inputs["x"].shape == x0.shape and not torch.equal(inputs["x"], x0)  # overwritten with x_t, as the other paths do
    sum(losses.values()).backward()
    w = dict(m.named_parameters())[head]
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    assert bool((w.grad.flatten(1).abs().sum(1) > 0).all())
    before = w.detach().clone()
    opt.step()
    assert bool(torch.isfinite(w).all()) and not torch.equal(w.detach(), before)
    gd.set_steps(5)
    assert gd.diffusion.loss_weight.shape == (5,)
    img = gd.generate(data_shape=(B, C, 16, 16), model_inputs={"y": y}, guidance_scale=1.5, clamp_x=True, use_tqdm=False)["x"]
    assert img.shape == (B, C, 16, 16) and bool(torch.isfinite(img).all())


def test_the_v_prediction_config_builds_its_diffuser_and_trains(monkeypatch):
    """configs/train_mnist_ddpm_v_prediction.yaml through the Hydra stand-in, the way an entry script reaches it: `@hydra.main`,
    `instantiate(cfg.model)`, `Diffuser(..., extra_args=cfg.diffuser.extra_args)`; then one loss on the device"""
    from diffulab_amd import Diffuser
    from diffulab_amd.compat import hydra_shim
    from diffulab_amd.config import instantiate

    monkeypatch.setattr(sys, "argv", ["train.py", "dataset=mnist_synthetic", "model.model_channels=32"])
    built = {}

    @hydra_shim.main(version_base=None, config_path=os.path.join(ROOT, "configs"), config_name="train_mnist_ddpm_v_prediction")
    def train(cfg):
        den = instantiate(cfg.model)
        built["d"] = Diffuser(denoiser=den, model_type=cfg.diffuser.model_type, n_steps=cfg.diffuser.n_steps,
                              sampling_method=cfg.diffuser.sampling_method, extra_args=cfg.diffuser.get("extra_args", {}))
        built["batch"] = cfg.dataloader.batch_size

    train()
    d = built["d"]
    gd = d.diffusion
    assert type(gd).__name__ == "GaussianDiffusion" and gd.sampler.mean_type == "v" and not gd.sampler.learned_variance
    assert (gd.loss_target, gd.loss_weighting, gd.min_snr_gamma) == ("mean_type", "min_snr", 5.0) and built["batch"] == 128
    assert torch.equal(gd.loss_weight, gp.min_snr(od.GaussianTables(1000).alphas_bar, "v"))
    d.denoiser.to(DEV)
    x0 = synth.uniform("gde.cfg", (2, 1, 32, 32), lo=-1.0, hi=1.0).to(DEV)
    out = d.compute_loss({"x": x0, "y": torch.tensor([1, 2], device=DEV), "p": 0.0}, timesteps=torch.tensor([3, 700], dtype=torch.int32))
    assert set(out) == {"loss"} and bool(torch.isfinite(out["loss"]))
