"""GPU tests of the learned-variance DDPM: the step kernels that read a [B, 2C, H, W] prediction in place (dl_ddpm_step_lv,
dl_ddim_step_lv), the fused hybrid loss (dl_vlb_loss_fwd / _bwd) and the host layers over them (DDPM / DDIM, GaussianDiffusion).

Expected values: (1) the reference's own outputs (tests/golden/samplers_learned.npz), to the relative-L2 3e-6 that
tests/test_kernels_gpu.py holds the fixed-variance steps to; (2) for the loss, which the reference does not have, the f64 evaluation of
tests/learned_variance_common.py on the same f32 inputs.

Loss tolerance.  The kernel and the f32 CPU evaluation of the restatement are both f32 evaluations of the same formulas on the same
inputs; they differ in the transcendental implementations (expf, logf, tanhf) and in the order of the reductions.  So the f32 CPU
evaluation's own error against f64 is measured here, per case, and the kernel is allowed twice that plus the 3e-6 this suite grants
f32 element-wise kernels: relative for the two scalars; for dpred, per half, every element within
2 * max|f32 - f64| + 3e-6 * max|f64| (the maximum over the half, not the element's own f32 error, which can be zero by chance).
Measured figures: DESIGN.md section 2.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as eb  # noqa: E402
import learned_variance_common as lv  # noqa: E402
from oracle import diffusion as od  # noqa: E402
from oracle import dit as odit  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
SHAPE = (3, 4, 8, 8)


def rel(a, b):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().double().cpu() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b)).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def T():
    return od.GaussianTables(1000)


def step_inputs():
    xt = synth.normal("smp.xt", SHAPE)
    pred = torch.cat([synth.normal("smp.v", SHAPE), synth.normal("smpl.var", SHAPE)], dim=1)
    return xt, pred, torch.tensor([0, 7, 999], dtype=torch.int32)


def sampler(cls, T, **kw):
    s = cls(**kw)
    s.set_steps(T.betas.clone())
    return s


# ------------------------------------------------------------------------------------------------------------------ step parity
def test_steps_against_reference_fixture(ops, T, golden, monkeypatch):
    """every array of the fixture, through ops and through DDPM.step / DDIM.step"""
    from diffulab_amd.diffuse.samplers.gaussian_diffusion import DDIM, DDPM

    g = golden("samplers_learned")
    xt, pred, tt = (v.to(DEV) for v in step_inputs())
    tab = lv.tables(T).to(DEV)
    dn = torch.from_numpy(g["ddpm_noise"]).to(DEV)
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: dn)
    for vt in lv.VAR_TYPES:
        for mt in lv.MEAN_TYPES:
            for clamp in (False, True):
                outs = ops.ddpm_step_lv(pred, None, 0.0, xt, dn, tt, tab, ops.MEAN_TYPES[mt], ops.VAR_MODES[vt], clamp)
                r = sampler(DDPM, T, mean_type=mt, var_type=vt).step(pred, tt, xt, clamp_x=clamp)
                assert list(r) == ["x_prev", "estimated_x0", "x_prev_mean", "x_prev_std", "logprob"]
                for got, key in zip(outs, lv.STEP_KEYS):
                    want = torch.from_numpy(g[f"ddpm_{mt}_{vt}_{int(clamp)}_{key}"])
                    assert got.shape == xt.shape and rel(got, want) < 3e-6, (mt, vt, clamp, key)
                    assert rel(r[key], want) < 3e-6, (mt, vt, clamp, key)
    di = torch.from_numpy(g["ddim_noise"]).to(DEV)
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: di)
    tab3 = torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.alphas_bar_prev]).float().to(DEV)
    for eta in (0.0, 0.5):
        outs = ops.ddim_step(pred, None, 0.0, xt, di, tt, tab3, None, ops.MEAN_TYPES["epsilon"], False, eta, halves=True)
        r = sampler(DDIM, T, var_type="learned_range").step(pred, tt, xt, eta=eta)
        assert {f"ddim_eta{eta}_{k}" for k in r} == {k for k in g if k.startswith(f"ddim_eta{eta}_")}
        for got, key in zip(outs, lv.STEP_KEYS):
            if got is None:
                assert eta == 0 and key in ("x_prev_std", "logprob")
                continue
            want = torch.from_numpy(np.nan_to_num(g[f"ddim_eta{eta}_{key}"], nan=0, posinf=0, neginf=0))  # logprob at t == 0: sigma == 0
            assert rel(torch.nan_to_num(got, 0, 0, 0), want) < 3e-6, (eta, key)
            assert rel(torch.nan_to_num(r[key], 0, 0, 0), want) < 3e-6, (eta, key)


def test_cfg_fused_in_the_kernel_equals_combine_then_step(ops, T):
    xt, pred, tt = step_inputs()
    pu = torch.cat([synth.normal("smpl.u", SHAPE), synth.normal("smpl.uvar", SHAPE)], dim=1)
    nz = synth.normal("smp.noise", SHAPE)
    comb = lv.cfg_combine(pred, pu, 1.5)
    tab = lv.tables(T)
    d = [v.to(DEV) for v in (pred, pu, xt, nz, tt, tab, comb)]
    for vt in lv.VAR_TYPES:
        fused = ops.ddpm_step_lv(d[0], d[1], 1.5, d[2], d[3], d[4], d[5], 0, ops.VAR_MODES[vt], True)
        plain = ops.ddpm_step_lv(d[6], None, 0.0, d[2], d[3], d[4], d[5], 0, ops.VAR_MODES[vt], True)
        want = lv.ddpm_step(tab, comb, tt, xt, nz, "epsilon", vt, True, dtype=torch.float64)
        for a, b, key in zip(fused, plain, lv.STEP_KEYS):
            assert rel(a, b) < 3e-6 and rel(a, want[key]) < 3e-6, (vt, key)
    tab3 = torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.alphas_bar_prev]).float().to(DEV)
    fused = ops.ddim_step(d[0], d[1], 1.5, d[2], d[3], d[4], tab3, None, 0, True, 0.5, halves=True)
    plain = ops.ddim_step(d[6][:, :4].contiguous(), None, 0.0, d[2], d[3], d[4], tab3, None, 0, True, 0.5)
    for a, b, key in zip(fused, plain, lv.STEP_KEYS):
        assert rel(torch.nan_to_num(a, 0, 0, 0), torch.nan_to_num(b, 0, 0, 0)) < 3e-6, key


def test_sampler_loop_against_reference_fixture(golden, monkeypatch):
    """5-step respaced DDPM, learned_range, CFG 1.5, clamp, on this project's DiT with the fixture's weights; the bound is the one
    tests/test_dit_gpu.py holds `loop_ddpm_x` to (bf16 denoiser)"""
    from diffulab_amd import Diffuser, MMDiT

    g = golden("samplers_learned")
    kw = dict(input_channels=4, output_channels=8, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2, depth=2,
              n_classes=10, classifier_free=True)
    m = MMDiT(simple_dit=True, **kw)
    m.load_state_dict(synth.dit_params(odit.param_shapes(odit.DiTConfig(**kw)), seed=5))
    m = m.to(DEV).eval()
    y = synth.integers("smpl.y", (2,), 10).to(DEV)
    x_init = synth.normal("smpl.init", (2, 4, 16, 16))
    it = iter(torch.from_numpy(g["loop_ddpm_noise"]))
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: next(it).to(ref.device))
    gd = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000,
                  extra_args={"sampler_parameters": {"var_type": "learned_range"}})
    gd.set_steps(5)
    out = gd.diffusion.denoise(m, {"x": x_init.to(DEV), "y": y}, use_tqdm=False, guidance_scale=1.5, clamp_x=True)
    assert out["x"].shape == (2, 4, 16, 16)
    assert rel(out["x"], g["loop_ddpm_x"]) < 3e-2


# ------------------------------------------------------------------------------------------------------------------ hybrid loss
@pytest.mark.parametrize("var_type", lv.VAR_TYPES)
@pytest.mark.parametrize("mean_type", lv.MEAN_TYPES)
def test_hybrid_loss_forward_and_backward(ops, T, mean_type, var_type):
    c = lv.loss_case(T, mean_type, var_type)
    args = (c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], mean_type, var_type)
    # the inputs keep clear of the clamp and of the bin thresholds (checked on the f64 restatement, on the CPU)
    p = lv.hybrid_parts(*args)
    x0 = c["x0"]
    assert float(p["prob"][p["first"]].min()) > 10 * 1e-12
    assert bool(((x0.abs() - 0.999).abs() > 1e-3)[x0.abs() != 1.0].all()) and int((x0.abs() == 1.0).sum()) > 6
    g_mse, g_vb = 0.75, 1.25
    ref = {"mse": p["mse"], "vb": p["vb"], "dpred": lv.hybrid_backward(*args, g_mse=g_mse, g_vb=g_vb)}
    m32, v32 = lv.hybrid_loss(*args, dtype=torch.float32)
    f32 = {"mse": m32, "vb": v32, "dpred": lv.hybrid_backward(*args, g_mse=g_mse, g_vb=g_vb, dtype=torch.float32)}
    assert f32["dpred"].dtype == torch.float32

    d = {k: c[k].to(DEV) for k in ("pred", "eps", "x0", "xt", "t", "tab")}
    mt, vm = ops.MEAN_TYPES[mean_type], ops.VAR_MODES[var_type]
    both = ops.vlb_loss_fwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], mt, vm)
    again = ops.vlb_loss_fwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], mt, vm)
    assert torch.equal(both.view(torch.int32), again.view(torch.int32))  # fixed-order partials: bit-identical across runs
    gm, gv = torch.tensor(g_mse, device=DEV), torch.tensor(g_vb, device=DEV)
    dpred = ops.vlb_loss_bwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], mt, vm, gm, gv)
    assert dpred.shape == c["pred"].shape

    for i, k in enumerate(("mse", "vb")):
        e32 = abs(float(f32[k]) - float(ref[k])) / abs(float(ref[k]))
        got = abs(float(both[i]) - float(ref[k])) / abs(float(ref[k]))
        print(f"{mean_type}/{var_type} {k}: ref {float(ref[k]):.9g}  f32-cpu rel err {e32:.3e}  kernel rel err {got:.3e}  bound {2 * e32 + 3e-6:.3e}")
        assert got <= 2 * e32 + 3e-6, (k, got, e32)
    C = x0.shape[1]
    for name, sl in (("mean half", slice(0, C)), ("variance half", slice(C, 2 * C))):
        r, a = ref["dpred"][:, sl], f32["dpred"][:, sl].double()
        e32 = float((a - r).abs().max())
        bound = 2 * e32 + 3e-6 * float(r.abs().max())
        err = (dpred[:, sl].double().cpu() - r).abs()
        print(f"{mean_type}/{var_type} dpred {name}: max|ref| {float(r.abs().max()):.3e}  f32-cpu max err {e32:.3e}  kernel max err "
              f"{float(err.max()):.3e}  bound {bound:.3e}")
        assert bool(torch.isfinite(dpred[:, sl]).all()) and int((err > bound).sum()) == 0, (name, float(err.max()), bound)
    # the mean half is the plain DL_LOSS_EPS backward on that half, bit for bit; so is the mse scalar
    o = d["pred"][:, :C].contiguous()
    plain = ops.mse_loss_bwd(o, d["eps"], None, 1.0, ops.LOSS_EPS, gscale_dev=gm)
    assert torch.equal(dpred[:, :C].contiguous().view(torch.int32), plain.view(torch.int32))
    assert torch.equal(both[0].view(torch.int32), ops.mse_loss_fwd(o, d["eps"], None, ops.LOSS_EPS).view(torch.int32))


def test_hybrid_head_autograd_routes_both_upstream_gradients(ops, T):
    from diffulab_amd.diffuse.modelizations.diffusion import hybrid_head

    c = lv.loss_case(T, "epsilon", "learned_range")
    d = {k: c[k].to(DEV) for k in ("pred", "eps", "x0", "xt", "t", "tab")}
    pred = d["pred"].clone().requires_grad_(True)
    mse, vb = hybrid_head(pred, d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 0, 1)
    (mse + 0.5 * vb).backward()
    want = ops.vlb_loss_bwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 0, 1, torch.tensor(1.0, device=DEV),
                            torch.tensor(0.5, device=DEV))
    assert torch.equal(pred.grad.view(torch.int32), want.view(torch.int32))
    pred.grad = None
    mse, vb = hybrid_head(pred, d["eps"], d["x0"], d["xt"], d["t"], d["tab"], 0, 1)
    vb.backward()  # the bound alone: nothing reaches the mean half
    assert float(pred.grad[:, :3].abs().max()) == 0.0 and float(pred.grad[:, 3:].abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------------------------ write guards
@pytest.mark.parametrize("chw", [1, 63, 257])
def test_outputs_stay_inside_their_windows(ops, T, chw):
    B = 3
    n = B * chw
    tab = lv.tables(T).to(DEV)
    tab3 = torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.alphas_bar_prev]).float().to(DEV)
    t = torch.tensor([0, 7, 999], dtype=torch.int32, device=DEV)
    xt, nz, eps = (synth.normal(f"lvg.{k}{chw}", (B, chw)).to(DEV) for k in ("xt", "nz", "eps"))
    x0 = synth.uniform(f"lvg.x0{chw}", (B, chw), lo=-1.0, hi=1.0).to(DEV)
    pred, pu = (synth.normal(f"lvg.{k}{chw}", (B, 2 * chw)).to(DEV) for k in ("pred", "pu"))

    def windows(k, cols=n):
        return [eb.Guarded(1, cols, torch.float32, DEV) for _ in range(k)]

    for vm in (0, 1):
        w = windows(5)
        ops.ddpm_step_lv(pred, pu, 1.5, xt, nz, t, tab, 0, vm, True, out=[g.win for g in w])
        for g, key in zip(w, lv.STEP_KEYS):
            g.check(f"dl_ddpm_step_lv var_mode {vm} chw {chw}: {key}")
        w = windows(1, 2) + windows(1, 2 * n)
        ops.vlb_loss_fwd(pred, eps, x0, xt, t, tab, 0, vm, out=w[0].win.view(2))
        ops.vlb_loss_bwd(pred, eps, x0, xt, t, tab, 0, vm, None, None, out=w[1].win)
        w[0].check(f"dl_vlb_loss_fwd var_mode {vm} chw {chw}")
        w[1].check(f"dl_vlb_loss_bwd var_mode {vm} chw {chw}")
    w = windows(5)
    ops.ddim_step(pred, pu, 1.5, xt, nz, t[1:].repeat(2)[:3].contiguous(), tab3, None, 0, True, 0.5, halves=True, out=[g.win for g in w])
    for g, key in zip(w, lv.STEP_KEYS):
        g.check(f"dl_ddim_step_lv chw {chw}: {key}")


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


@pytest.mark.parametrize("family", list(FAMILIES))
def test_train_step_and_sampling_end_to_end(family):
    from diffulab_amd import Diffuser
    from diffulab_amd.training.optim import FusedAdamW

    torch.manual_seed(0)
    make, C, head = FAMILIES[family]
    m = make(2 * C)
    with torch.no_grad():  # the output heads start at zero: give the variance channels something to predict from
        dict(m.named_parameters())[head].normal_(std=0.02)
    m = m.to(DEV)
    B = 4
    gd = Diffuser(m, model_type="gaussian_diffusion", sampling_method="ddpm", n_steps=1000,
                  extra_args={"sampler_parameters": {"var_type": "learned_range"}})
    assert gd.diffusion.vlb_weight == 1.0
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    x0 = synth.uniform(f"lve.{family}", (B, C, 16, 16), lo=-1.0, hi=1.0).to(DEV)
    y = synth.integers("lve.y", (B,), 10).to(DEV)
    ti = torch.tensor([0, 5, 500, 999], dtype=torch.int32)
    inputs = {"x": x0.clone(), "y": y, "p": 0.0}
    losses = gd.compute_loss(inputs, timesteps=ti)
    assert set(losses) == {"loss", "vb"} and all(v.shape == () and bool(torch.isfinite(v)) for v in losses.values())
    assert inputs["x"].shape == x0.shape and not torch.equal(inputs["x"], x0)  # overwritten with x_t, as the fixed path does
    losses["vb"].backward()  # the bound alone reaches the head through the variance channels only
    w = dict(m.named_parameters())[head]
    rows = w.grad.flatten(1).abs().sum(1) > 0
    assert int(rows.sum()) == w.shape[0] // 2, (int(rows.sum()), w.shape[0])
    opt.zero_grad()
    losses = gd.compute_loss({"x": x0.clone(), "y": y, "p": 0.0}, timesteps=ti)
    sum(losses.values()).backward()
    assert bool((dict(m.named_parameters())[head].grad.flatten(1).abs().sum(1) > 0).all())
    before = w.detach().clone()
    opt.step()
    assert bool(torch.isfinite(w).all()) and not torch.equal(w.detach(), before)
    gd.set_steps(3)
    img = gd.generate(data_shape=(B, C, 16, 16), model_inputs={"y": y}, guidance_scale=1.5, clamp_x=True, use_tqdm=False)["x"]
    assert img.shape == (B, C, 16, 16) and bool(torch.isfinite(img).all())
    ddim = Diffuser(m, model_type="gaussian_diffusion", sampling_method="ddim", n_steps=1000,
                    extra_args={"sampler_parameters": {"var_type": "learned_range"}})
    # (the reference's DDIM respacing takes stride 1 only -- modelizations/utils.py:26-31 --, so three steps of the full chain)
    x = torch.randn(B, C, 16, 16, device=DEV)
    with torch.no_grad():
        for t in (999, 500, 1):
            x = ddim.diffusion.one_step_denoise(m, {"x": x, "y": y}, t=t, guidance_scale=1.5)["x_prev"]
            assert x.shape == (B, C, 16, 16) and bool(torch.isfinite(x).all())


@pytest.mark.parametrize("family", list(FAMILIES))
def test_fixed_variance_loss_is_the_plain_mse_head(family, ops):
    """with a fixed var_type compute_loss is what it was: one entry, the bits of mse_head on the model's prediction"""
    from diffulab_amd import Diffuser
    from diffulab_amd.diffuse.modelizations.diffusion import mse_head

    torch.manual_seed(0)
    make, C, head = FAMILIES[family]
    m = make(C)
    with torch.no_grad():
        dict(m.named_parameters())[head].normal_(std=0.02)
    m = m.to(DEV)
    seen = {}

    def tapped(**kw):
        out = m(**kw)
        seen["pred"] = out["x"]
        return out

    gd = Diffuser(m, model_type="gaussian_diffusion", sampling_method="ddpm", n_steps=1000,
                  extra_args={"sampler_parameters": {"var_type": "fixed_small"}})
    B = 4
    x0 = synth.uniform(f"lve.{family}", (B, C, 16, 16), lo=-1.0, hi=1.0).to(DEV)
    noise = synth.normal(f"lve.n.{family}", (B, C, 16, 16)).to(DEV)
    y = synth.integers("lve.y", (B,), 10).to(DEV)
    ti = torch.tensor([0, 5, 500, 999], dtype=torch.int32)
    losses = gd.diffusion.compute_loss(tapped, {"x": x0.clone(), "y": y, "p": 0.0}, ti, noise)
    assert set(losses) == {"loss"} and seen["pred"].shape == x0.shape
    direct = mse_head(seen["pred"].detach(), noise, None, ops.LOSS_EPS)
    assert torch.equal(losses["loss"].detach().view(torch.int32), direct.view(torch.int32))
