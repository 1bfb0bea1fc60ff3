"""CPU checks of the x0 / x_prev / v training targets and of min-SNR weighting: the restatement in tests/gd_param_common.py reproduces
what the reference's DDPM says its three parameterisations are (tests/golden/gd_targets.npz, written by
tests/golden/make_gd_targets_golden.py); v, which the reference does not have, satisfies its defining algebra in f64; the min-SNR tables
have the paper's values; the hand-written backward equals torch autograd of the f64 forward; GaussianDiffusion's defaults stay on the
heads they used; the new C entry points refuse bad arguments before any device work.

Bound of an inverse compared in f32 (estimated_x0 from an xprev or epsilon prediction, epsilon from x0): these divide by coef1, sqrt_ab
or sqrt(1 / ab - 1), which amplifies f32 rounding at the ends of the chain, so the rule is the one tests/test_learned_variance_gpu.py
states: every element within twice the f32 restatement's own measured error against f64, plus 3e-6 of the reference's maximum.
"""

import ctypes

import numpy as np
import pytest
import torch

import gd_param_common as gp
import learned_variance_common as lv
from oracle import diffusion as od


def rel(a, b):
    a = (a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).double()
    b = (b.detach() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b))).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def within_inverse_bound(f32: torch.Tensor, f64: torch.Tensor, ref, what) -> None:
    ref = torch.as_tensor(np.asarray(ref)).double()
    e32 = float((f32.double() - f64).abs().max())
    bound = 2 * e32 + 3e-6 * float(ref.abs().max())
    err = float((f32.double() - ref).abs().max())
    assert err <= bound, (what, err, bound)


# ------------------------------------------------------------------------------------------------------------------ fixture
def test_fixture_holds_every_case(golden):
    g = golden("gd_targets")
    want = {f"{c}_{k}" for c in gp.CHAINS for k in ("xt", "xprev_target", "eps_from_xstart")}
    want |= {f"{c}_{mt}_{k}" for c in gp.CHAINS for mt in gp.REFERENCE_TARGETS for k in ("estimated_x0", "x_prev_mean")}
    assert set(g) == want
    assert all(v.dtype == np.float32 and v.shape == gp.FIXTURE_SHAPE for v in g.values())


@pytest.mark.parametrize("chain", list(gp.CHAINS))
def test_restatement_reproduces_the_reference_targets_and_steps(golden, chain):
    g = golden("gd_targets")
    T, t = gp.chain(chain)
    assert T.betas.shape == (gp.CHAINS[chain][0],)
    tab = lv.tables(T)
    x0, eps = gp.fixture_inputs()
    xt = od.ddpm_add_noise(T, x0, t, eps)
    assert rel(xt, g[f"{chain}_xt"]) < 3e-6
    xt = torch.from_numpy(g[f"{chain}_xt"])  # from here on the reference's own x_t
    r32, r64 = gp._rows(tab, t, xt, torch.float32), gp._rows(tab, t, xt, torch.float64)
    xprev = gp.target(r32, eps, x0, xt, "xprev")
    assert xprev.dtype == torch.float32 and rel(xprev, g[f"{chain}_xprev_target"]) < 3e-6
    # epsilon from x0 (ddpm.py:324-326): an inverse
    def eps_of(rows, x0, xt):
        return ((1 / rows[0]) * xt - x0) / (1 / rows[1] - 1).sqrt()
    within_inverse_bound(eps_of(r32, x0, xt), eps_of(r64, x0.double(), xt.double()), g[f"{chain}_eps_from_xstart"], (chain, "eps"))
    for mt in gp.REFERENCE_TARGETS:
        tgt = gp.target(r32, eps, x0, xt, mt)
        x0e = gp.x_start(tgt, xt, r32, mt)
        x0e64 = gp.x_start(tgt.double(), xt.double(), r64, mt)
        mean = gp.posterior_mean(r32, x0e, xt)
        assert mean.dtype == torch.float32 and rel(mean, g[f"{chain}_{mt}_x_prev_mean"]) < 3e-6, (chain, mt)
        within_inverse_bound(x0e, x0e64, g[f"{chain}_{mt}_estimated_x0"], (chain, mt, "estimated_x0"))
        # a step fed the exact target of its parameterisation lands on the posterior mean of (x0, xt)
        assert rel(g[f"{chain}_{mt}_x_prev_mean"], g[f"{chain}_xprev_target"]) < 3e-6, (chain, mt)


# ------------------------------------------------------------------------------------------------------------------ v
@pytest.mark.parametrize("chain", list(gp.CHAINS))
def test_v_satisfies_its_defining_algebra_in_f64(chain):
    T, t = gp.chain(chain)
    tab64 = torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.posterior_mean_coef1, T.posterior_mean_coef2,
                         T.posterior_log_variance_clipped, T.betas])  # the fp64 schedule itself: sqrt_ab^2 == ab to an ulp
    x0, eps = (v.double() for v in gp.fixture_inputs())
    rows = gp._rows(tab64, t, x0, torch.float64)
    sab, s1 = rows[0], (1 - rows[1]).sqrt()
    xt = sab * x0 + s1 * eps
    v = gp.target(rows, eps, x0, xt, "v")
    assert float((gp.x_start(v, xt, rows, "v") - x0).abs().max()) <= 1e-12
    assert float((s1 * xt + sab * v - eps).abs().max()) <= 1e-12
    mean_from_v = gp.posterior_mean(rows, gp.x_start(v, xt, rows, "v"), xt)
    assert float((mean_from_v - gp.target(rows, eps, x0, xt, "xprev")).abs().max()) <= 1e-12


def test_v_step_restatement_on_the_exact_target_is_the_posterior_mean():
    """f32, on the tables the kernels read: the v inverse multiplies (no division), so the posterior mean of the recovered x0 meets
    the one of the true x0 to the relative-L2 3e-6 of the reference mean types"""
    for chain in gp.CHAINS:
        T, t = gp.chain(chain)
        tab = gp.fixed_tables(T)
        x0, eps = gp.fixture_inputs()
        xt = od.ddpm_add_noise(T, x0, t, eps)
        rows = gp._rows(tab, t, xt, torch.float32)
        r = gp.ddpm_step_v(tab, gp.target(rows, eps, x0, xt, "v"), t, xt, torch.zeros_like(xt), "fixed")
        assert rel(r["x_prev_mean"], gp.posterior_mean(rows, x0, xt)) < 3e-6 and rel(r["estimated_x0"], x0) < 3e-6
        d = gp.ddim_step_v(gp.ddim_tables(T), gp.target(rows, eps, x0, xt, "v"), t, xt, torch.zeros_like(xt), 0.0, "fixed")
        assert rel(d["estimated_x0"], x0) < 3e-6


# ------------------------------------------------------------------------------------------------------------------ min-SNR
def test_min_snr_tables():
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion, min_snr_weights

    gamma = 5.0
    for chain in gp.CHAINS:
        T, _ = gp.chain(chain)
        w = {n: gp.min_snr(T.alphas_bar, n, gamma) for n in ("epsilon", "xstart", "v")}
        assert all(v.dtype == torch.float64 and v.shape == T.alphas_bar.shape and bool((v > 0).all()) for v in w.values())
        assert float(w["epsilon"].max()) <= 1.0 and float(w["v"].max()) <= 1.0 and float(w["xstart"].max()) <= gamma
        assert float(w["epsilon"].max()) == 1.0 and float(w["xstart"].max()) == gamma  # both regimes of the min occur
        for n, v in w.items():
            assert torch.equal(min_snr_weights(T.alphas_bar, n, gamma), v), (chain, n)
    # the two rows of the 1000-step linear chain either side of snr == gamma: snr[129] = 5.0647138..., snr[130] = 4.9832105...
    T, _ = gp.chain("full")
    snr = T.alphas_bar / (1 - T.alphas_bar)
    assert int((snr - gamma).abs().argmin()) == 130 and abs(float(snr[129]) - 5.064713815153268) < 1e-9
    assert abs(float(snr[130]) - 4.983210512272224) < 1e-9
    literal = {"epsilon": (5.0 / 5.064713815153268, 1.0), "xstart": (5.0, 4.983210512272224),
               "v": (5.0 / 6.064713815153268, 4.983210512272224 / 5.983210512272224)}
    for n, (above, below) in literal.items():
        got = min_snr_weights(T.alphas_bar, n, gamma)
        assert abs(float(got[129]) - above) < 1e-9 and abs(float(got[130]) - below) < 1e-9, (n, float(got[129]), float(got[130]))
    with pytest.raises(ValueError, match="xprev"):
        min_snr_weights(T.alphas_bar, "xprev", gamma)
    with pytest.raises(ValueError, match="xprev"):
        gp.min_snr(T.alphas_bar, "xprev", gamma)
    with pytest.raises(ValueError, match="xprev"):
        GaussianDiffusion(sampler_parameters={"mean_type": "xprev"}, loss_target="mean_type", loss_weighting="min_snr")


# ------------------------------------------------------------------------------------------------------------------ backward
BACKWARD_CASES = [(n, vt, wn) for n in gp.TARGETS for vt in gp.VAR_TYPES for wn in ("unweighted", "min_snr") if (n, wn) != ("xprev", "min_snr")]


@pytest.mark.parametrize("name,var_type,weighting", BACKWARD_CASES)
def test_hand_written_backward_equals_autograd_in_f64(name, var_type, weighting):
    T = od.GaussianTables(1000)
    c = gp.loss_case(T, name, var_type)
    w = gp.weightings(T, name)[weighting]
    args = (c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], name, var_type, w)
    pred = c["pred"].double().requires_grad_(True)
    mse, vb = gp.loss(c["tab"], pred, *args[2:])
    assert mse.dtype == torch.float64 and bool(torch.isfinite(mse)) and (vb is None) == (var_type == "fixed")
    C = c["x0"].shape[1]
    for g_mse, g_vb in ((1.0, 1.0), (0.0, 1.0), (0.7, 0.0), (1.3, 0.25)):
        total = g_mse * mse + (0.0 if vb is None else g_vb * vb)
        (grad,) = torch.autograd.grad(total, pred, retain_graph=True)
        hand = gp.loss_backward(*args, g_mse=g_mse, g_vb=g_vb)
        assert hand.shape == grad.shape
        assert float((grad - hand).abs().max()) <= 1e-12 * max(float(grad.abs().max()), 1e-300), (g_mse, g_vb)
    if vb is not None:  # the bound sends nothing into the mean half
        (gvb,) = torch.autograd.grad(vb, pred)
        assert float(gvb[:, :C].abs().max()) == 0.0 and float(gvb[:, C:].abs().max()) > 0.0
    if w is not None:  # the weight is on the mse alone: the bound of the weighted case is the unweighted bound
        assert vb is None or float(vb.detach()) == float(gp.loss(c["tab"], c["pred"], *args[2:8])[1])
        assert float(mse.detach()) != float(gp.loss(c["tab"], c["pred"], *args[2:8])[0])


def test_loss_inputs_stay_clear_of_the_clamp_and_of_the_bin_thresholds():
    T = od.GaussianTables(1000)
    for case in gp.LOSS_CASES:
        for name in gp.TARGETS:
            for vt in ("learned", "learned_range"):
                c = gp.loss_case(T, name, vt, case)
                x0, t = c["x0"], c["t"]
                edge = x0.abs() == 1.0
                assert bool(((x0.abs() - 0.999).abs() > 1e-3)[~edge].all()) and float(x0.abs().max()) == 1.0
                first = t == 0
                assert bool((x0[first] == 1.0).any()) and bool((x0[first] == -1.0).any())
                rows = gp._rows(c["tab"], t, c["xt"], torch.float64)
                p = lv.hybrid_parts(c["tab"], gp._bound_pred(c["pred"].double(), c["xt"].double(), rows, name), c["eps"], x0, c["xt"], t,
                                    "xstart", vt)
                assert float(p["prob"][p["first"]].min()) > 1e-11, (case, name, vt)


# ------------------------------------------------------------------------------------------------------------------ constructor
class _Stub(torch.nn.Module):
    def forward(self, x, timesteps, **kw):
        return {"x": torch.cat([x, x], dim=1) if self.double else x}


def _host_diffusion(monkeypatch, **kw):
    """a GaussianDiffusion whose heads are recorders and whose noising runs on the CPU oracle: compute_loss's routing without a GPU"""
    from diffulab_amd.diffuse.modelizations import gaussian_diffusion as gdm

    calls = []
    monkeypatch.setattr(gdm, "mse_head", lambda *a: calls.append(("mse_head", a)) or torch.zeros(()))
    monkeypatch.setattr(gdm, "hybrid_head", lambda *a: calls.append(("hybrid_head", a)) or (torch.zeros(()), torch.zeros(())))
    gd = gdm.GaussianDiffusion(**kw)
    T = od.GaussianTables(1000)
    monkeypatch.setattr(gd, "add_noise", lambda x, t, noise=None: (od.ddpm_add_noise(T, x, t, noise), noise))
    return gdm, gd, calls


@pytest.mark.parametrize("var_type", ["fixed_small", "learned_range"])
@pytest.mark.parametrize("mean_type", gp.REFERENCE_TARGETS)
def test_defaults_leave_compute_loss_on_the_heads_it_used(monkeypatch, mean_type, var_type):
    gdm, gd, calls = _host_diffusion(monkeypatch, sampler_parameters={"mean_type": mean_type, "var_type": var_type})

    def boom(*a, **k):
        raise AssertionError("gd_head reached with default arguments")

    monkeypatch.setattr(gdm, "gd_head", boom)
    assert (gd.loss_target, gd.loss_weighting, gd.min_snr_gamma, gd.loss_weight) == ("epsilon", None, 5.0, None)
    m = _Stub()
    m.double = var_type == "learned_range"
    x0, eps = gp.fixture_inputs()
    t = torch.tensor(gp.CHAINS["full"][1], dtype=torch.int32)
    out = gd.compute_loss(m, {"x": x0.clone()}, t, eps)
    assert [c[0] for c in calls] == ["hybrid_head" if m.double else "mse_head"]
    a = calls[0][1]
    if m.double:  # the parent's call: (prediction, noise, x0, xt, t, tables, mean_type, var_mode)
        assert set(out) == {"loss", "vb"} and len(a) == 8 and a[1] is eps and torch.equal(a[2], x0) and a[6:] == (gp.TARGETS.index(mean_type), 1)
    else:  # the parent's call: mse_head(prediction, noise, None, LOSS_EPS)
        assert set(out) == {"loss"} and len(a) == 4 and a[1] is eps and a[2] is None and a[3] == 1


@pytest.mark.parametrize("kw,target,weighted", [
    (dict(sampler_parameters={"mean_type": "xstart"}, loss_target="mean_type"), 1, False),
    (dict(sampler_parameters={"mean_type": "v", "var_type": "learned_range"}, loss_target="mean_type", loss_weighting="min_snr"), 3, True),
    (dict(loss_weighting="min_snr", min_snr_gamma=3.0), 0, True),
    (dict(sampler_parameters={"mean_type": "xprev"}, loss_target="mean_type"), 2, False),
])
def test_new_arguments_route_compute_loss_through_gd_head(monkeypatch, kw, target, weighted):
    gdm, gd, calls = _host_diffusion(monkeypatch, **kw)
    seen = []

    def head(pred, eps, x0, xt, t, tables, tgt, weight=None, var_mode=-1):
        seen.append((tgt, weight, var_mode, eps, x0, xt))
        return torch.zeros(()) if var_mode == -1 else (torch.zeros(()), torch.ones(()))

    monkeypatch.setattr(gdm, "gd_head", head)
    m = _Stub()
    m.double = gd.sampler.learned_variance
    x0, eps = gp.fixture_inputs()
    t = torch.tensor(gp.CHAINS["full"][1], dtype=torch.int32)
    inputs = {"x": x0.clone()}
    out = gd.compute_loss(m, inputs, t, eps)
    assert calls == [] and len(seen) == 1
    tgt, weight, var_mode, e, x, xt = seen[0]
    assert tgt == target and var_mode == (1 if m.double else -1) and e is eps and torch.equal(x, x0) and xt is inputs["x"]
    assert set(out) == ({"loss", "vb"} if m.double else {"loss"})  # the keys of the returned dict do not change
    if m.double:
        assert float(out["vb"]) == gd.vlb_weight
    if weighted:
        want = gp.min_snr(od.GaussianTables(1000).alphas_bar, gp.TARGETS[target], gd.min_snr_gamma).float()
        assert weight.dtype == torch.float32 and torch.equal(weight, want)
    else:
        assert weight is None


def test_constructor_refusals_and_the_rebuilt_weight_table():
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion
    from diffulab_amd.diffuse.samplers.gaussian_diffusion import DDIM, DDPM

    with pytest.raises(ValueError, match='loss_target="mean_type"'):
        GaussianDiffusion(sampler_parameters={"mean_type": "v"})
    with pytest.raises(ValueError, match='loss_target="mean_type"'):
        GaussianDiffusion(sampling_method="ddim", sampler_parameters={"mean_type": "v"}, loss_target="epsilon")
    with pytest.raises(ValueError, match="min_snr"):
        GaussianDiffusion(loss_weighting="p2")
    with pytest.raises(ValueError, match="mean_type"):
        GaussianDiffusion(loss_target="x0")
    # a weight touches "loss" alone: where it would also change how the bound reads the output, the combination is refused
    for mt in ("xstart", "xprev"):
        for vt in lv.VAR_TYPES:
            with pytest.raises(ValueError, match='loss_target="mean_type"'):
                GaussianDiffusion(sampler_parameters={"mean_type": mt, "var_type": vt}, loss_weighting="min_snr")
        assert GaussianDiffusion(sampler_parameters={"mean_type": mt}, loss_weighting="min_snr")._target == "epsilon"  # fixed variances
    assert GaussianDiffusion(sampler_parameters={"var_type": "learned"}, loss_weighting="min_snr")._target == "epsilon"
    assert GaussianDiffusion(sampler_parameters={"mean_type": "xstart", "var_type": "learned"}, loss_target="mean_type",
                             loss_weighting="min_snr")._target == "xstart"
    for cls in (DDPM, DDIM):
        assert cls(mean_type="v").mean_type == "v"
        with pytest.raises(ValueError):
            cls(mean_type="velocity")
    gd = GaussianDiffusion(sampler_parameters={"mean_type": "v"}, loss_target="mean_type", loss_weighting="min_snr")
    assert gd.loss_weight.dtype == torch.float64 and gd.loss_weight.shape == (1000,)
    assert torch.equal(gd.loss_weight, gp.min_snr(od.GaussianTables(1000).alphas_bar, "v"))
    assert torch.equal(gd._weight(torch.device("cpu")), gd.loss_weight.float()) and len(gd._dev_weight) == 1
    gd.set_steps(50)  # a respaced chain has its own alphas_bar
    T50 = od.GaussianTables(1000, n_steps=50)
    assert gd.loss_weight.shape == (50,) and torch.equal(gd.loss_weight, gp.min_snr(T50.alphas_bar, "v")) and gd._dev_weight == {}
    assert torch.equal(gd._weight(torch.device("cpu")), gp.min_snr(T50.alphas_bar, "v").float())
    # through the Diffuser, the way the YAML reaches it
    from diffulab_amd import Diffuser

    d = Diffuser(torch.nn.Linear(1, 1), sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000,
                 extra_args={"sampler_parameters": {"mean_type": "v"}, "loss_target": "mean_type", "loss_weighting": "min_snr",
                             "min_snr_gamma": 4.0})
    assert d.diffusion.min_snr_gamma == 4.0 and float(d.diffusion.loss_weight.max()) <= 1.0


def test_the_v_prediction_config_composes():
    import os

    from diffulab_amd.config import load_config

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = load_config(os.path.join(root, "configs"), "train_mnist_ddpm_v_prediction")
    e = c.diffuser.extra_args
    assert e.sampler_parameters.mean_type == "v" and e.loss_target == "mean_type" and e.loss_weighting == "min_snr"
    assert c.diffuser.model_type == "gaussian_diffusion" and c.dataloader.batch_size == 128


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_entry_points_refuse_bad_arguments_before_any_launch():
    from diffulab_amd import _lib

    L = _lib.lib()
    c = L.cdll
    buf = ctypes.create_string_buffer(1024)
    P = ctypes.c_void_p(ctypes.addressof(buf))  # a non-null dummy, never dereferenced: the calls below are refused on the host
    i64, F = ctypes.c_int64, ctypes.c_float

    def refused(name, *args):
        assert getattr(c, name)(*args) == -1 and name in c.dl_last_error().decode(), (name, c.dl_last_error().decode())

    # dl_gd_loss_fwd(pred, eps, x0, xt, t, tables, T, target, weight, var_mode, partial, loss, batch, chw, stream)
    def fwd(pred=P, eps=P, x0=P, xt=P, t=P, tab=P, T=1000, target=0, w=None, vm=-1, partial=P, loss=P, B=2, chw=64):
        refused("dl_gd_loss_fwd", pred, eps, x0, xt, t, tab, T, target, w, vm, partial, loss, i64(B), i64(chw), None)

    # dl_gd_loss_bwd(pred, eps, x0, xt, t, tables, T, target, weight, var_mode, g_mse, g_vb, dpred, batch, chw, stream)
    def bwd(pred=P, eps=P, x0=P, xt=P, t=P, tab=P, T=1000, target=0, w=None, vm=-1, dpred=P, B=2, chw=64):
        refused("dl_gd_loss_bwd", pred, eps, x0, xt, t, tab, T, target, w, vm, None, None, dpred, i64(B), i64(chw), None)

    for f in (fwd, bwd):
        f(pred=None)
        f(t=None)
        f(tab=None)
        f(target=4)
        f(target=-1)
        f(vm=2)
        f(vm=-2)
        f(B=0)
        f(chw=0)
        f(T=0)
        f(eps=None)  # the epsilon target reads eps
        f(eps=None, target=3)
        f(x0=None, target=1)
        f(x0=None, target=3)
        f(x0=None, vm=0)  # learned variances read x0 and xt whatever the target
        f(xt=None, vm=1)
        f(xt=None, target=2)
    fwd(partial=None)
    fwd(loss=None)
    bwd(dpred=None)

    # dl_ddpm_step_v(pred, pu, g, xt, noise, t, tables, T, var_mode, clamp, x_prev, x0, mean, std, logprob, batch, chw, stream)
    def ddpm(pred=P, xt=P, noise=P, t=P, tab=P, T=1000, vm=-1, xp=P, B=2, chw=64):
        refused("dl_ddpm_step_v", pred, None, F(0), xt, noise, t, tab, T, vm, 0, xp, P, P, P, P, i64(B), i64(chw), None)

    # dl_ddim_step_v(pred, pu, g, xt, noise, t, tables, T, var_mode, clamp, eta, x_prev, x0, mean, std, logprob, batch, chw, stream)
    def ddim(pred=P, xt=P, noise=P, t=P, tab=P, T=1000, vm=-1, xp=P, B=2, chw=64):
        refused("dl_ddim_step_v", pred, None, F(0), xt, noise, t, tab, T, vm, 0, F(0), xp, P, P, None, None, i64(B), i64(chw), None)

    for f in (ddpm, ddim):
        f(pred=None)
        f(xt=None)
        f(noise=None)
        f(t=None)
        f(tab=None)
        f(xp=None)
        f(vm=2)
        f(vm=-2)
        f(B=0)
        f(chw=-1)
        f(T=0)
    # the entry points of the reference's three mean types keep refusing v
    refused("dl_ddpm_step", P, None, F(0), P, P, P, P, 1000, 3, 0, P, P, P, P, P, i64(2), i64(64), None)
    refused("dl_ddpm_step_lv", P, None, F(0), P, P, P, P, 1000, 3, 1, 0, P, P, P, P, P, i64(2), i64(64), None)
    refused("dl_ddim_step", P, None, F(0), P, P, P, P, 1000, 3, None, 0, F(0), P, P, P, None, None, i64(2), i64(64), None)
    refused("dl_ddim_step_lv", P, None, F(0), P, P, P, P, 1000, 3, None, 0, F(0), P, P, P, None, None, i64(2), i64(64), None)
    refused("dl_vlb_loss_fwd", P, P, P, P, P, P, 1000, 3, 1, P, P, i64(2), i64(64), None)
    assert {"dl_gd_loss_fwd", "dl_gd_loss_bwd", "dl_ddpm_step_v", "dl_ddim_step_v"} <= set(L.protos)
