"""CPU checks of the learned-variance work: the plain-torch restatement in tests/learned_variance_common.py reproduces the reference's
own DDPM / DDIM outputs (tests/golden/samplers_learned.npz, written by tests/golden/make_samplers_learned_golden.py) to the bounds
tests/test_oracle_golden.py holds the fixed-variance oracle to (1e-6 per step array, 1e-5 for the sampler loop); the hand-written
backward of the hybrid loss equals torch autograd of its forward in f64; the new C entry points refuse bad arguments before any device
work; the samplers and the modelization accept the learned types."""

import ctypes

import numpy as np
import pytest
import torch

import learned_variance_common as lv
from oracle import diffusion as od
from oracle import dit as odit
from oracle import synth

SHAPE = (3, 4, 8, 8)


def rel(a, b):
    a = (a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).double()
    b = (b.detach() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b))).double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def step_inputs():
    xt = synth.normal("smp.xt", SHAPE)
    pred = torch.cat([synth.normal("smp.v", SHAPE), synth.normal("smpl.var", SHAPE)], dim=1)
    return xt, pred, torch.tensor([0, 7, 999], dtype=torch.int32)


def test_fixture_holds_every_case(golden):
    g = golden("samplers_learned")
    want = {f"ddpm_{mt}_{vt}_{c}_{k}" for mt in lv.MEAN_TYPES for vt in lv.VAR_TYPES for c in (0, 1) for k in lv.STEP_KEYS}
    want |= {f"ddim_eta0.0_{k}" for k in ("x_prev", "estimated_x0", "x_prev_mean")}
    want |= {f"ddim_eta0.5_{k}" for k in lv.STEP_KEYS}
    want |= {"ddpm_noise", "ddim_noise", "loop_ddpm_x", "loop_ddpm_noise"}
    assert set(g) == want
    assert all(v.dtype != object for v in g.values())


def test_f32_restatement_reproduces_the_reference_steps(golden):
    g = golden("samplers_learned")
    T = od.GaussianTables(1000)
    tab = lv.tables(T)
    xt, pred, tt = step_inputs()
    dn = torch.from_numpy(g["ddpm_noise"])
    for vt in lv.VAR_TYPES:
        for mt in lv.MEAN_TYPES:
            for clamp in (False, True):
                r = lv.ddpm_step(tab, pred, tt, xt, dn, mt, vt, clamp)
                for k in lv.STEP_KEYS:
                    tag = f"ddpm_{mt}_{vt}_{int(clamp)}_{k}"
                    assert r[k].dtype == torch.float32 and rel(r[k], g[tag]) < 1e-6, tag
    for eta in (0.0, 0.5):
        r = lv.ddim_step(T, pred, tt, xt, torch.from_numpy(g["ddim_noise"]), eta)
        assert {f"ddim_eta{eta}_{k}" for k in r} == {k for k in g if k.startswith(f"ddim_eta{eta}_")}
        for k in r:
            a, b = r[k], g[f"ddim_eta{eta}_{k}"]
            if k == "logprob":  # -inf / nan at t == 0 where sigma == 0, in the reference too
                a, b = torch.nan_to_num(a, 0, 0, 0), np.nan_to_num(b, nan=0, posinf=0, neginf=0)
            assert rel(a, b) < 1e-6, (eta, k)


def test_f64_restatement_agrees_with_f32():
    """the f64 evaluation the GPU tests compare with is the same function: it differs from the f32 one by rounding only"""
    tab = lv.tables(od.GaussianTables(1000))
    xt, pred, tt = step_inputs()
    nz = synth.normal("smp.noise", SHAPE)
    for vt in lv.VAR_TYPES:
        a, b = lv.ddpm_step(tab, pred, tt, xt, nz, "epsilon", vt), lv.ddpm_step(tab, pred, tt, xt, nz, "epsilon", vt, dtype=torch.float64)
        for k in lv.STEP_KEYS:
            assert b[k].dtype == torch.float64 and rel(a[k], b[k]) < 1e-6, (vt, k)


def test_f32_restatement_reproduces_the_reference_loop(golden):
    g = golden("samplers_learned")
    cfg = odit.DiTConfig(input_channels=4, output_channels=8, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2,
                         depth=2, n_classes=10, classifier_free=True)
    P = synth.dit_params(odit.param_shapes(cfg), seed=5)
    y = synth.integers("smpl.y", (2,), cfg.n_classes)
    xc = synth.normal("smpl.init", (2, 4, 16, 16))
    y_un = torch.full_like(y, cfg.n_classes)
    T = od.GaussianTables(1000, n_steps=5)
    tab, tmap = lv.tables(T), torch.tensor(T.timestep_map, dtype=torch.int32)
    nz = torch.from_numpy(g["loop_ddpm_noise"])
    with torch.no_grad():
        for i, t in enumerate(reversed(range(5))):
            ti = torch.full((2,), t, dtype=torch.int32)
            tm = tmap[ti.long()]
            e = lv.cfg_combine(odit.dit_forward(P, xc, tm, y, cfg), odit.dit_forward(P, xc, tm, y_un, cfg), 1.5)
            assert e.shape == (2, 8, 16, 16)
            xc = lv.ddpm_step(tab, e, ti, xc, nz[i], "epsilon", "learned_range", clamp_x=True)["x_prev"]
    assert rel(xc, g["loop_ddpm_x"]) < 1e-5


@pytest.mark.parametrize("var_type", lv.VAR_TYPES)
@pytest.mark.parametrize("mean_type", lv.MEAN_TYPES)
def test_hand_written_backward_equals_autograd_in_f64(mean_type, var_type):
    T = od.GaussianTables(1000)
    c = lv.loss_case(T, mean_type, var_type)
    args = (c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], mean_type, var_type)
    pred = c["pred"].double().requires_grad_(True)
    mse, vb = lv.hybrid_loss(c["tab"], pred, *args[2:])
    assert mse.dtype == torch.float64 and bool(torch.isfinite(mse)) and bool(torch.isfinite(vb))
    for g_mse, g_vb in ((1.0, 1.0), (0.0, 1.0), (0.7, 0.0), (1.3, 0.25)):
        (grad,) = torch.autograd.grad(g_mse * mse + g_vb * vb, pred, retain_graph=True)
        hand = lv.hybrid_backward(*args, g_mse=g_mse, g_vb=g_vb)
        assert float((grad - hand).abs().max()) <= 1e-12 * float(grad.abs().max()), (g_mse, g_vb)
    # the bound sends nothing into the mean half
    (gvb,) = torch.autograd.grad(vb, pred)
    assert float(gvb[:, :3].abs().max()) == 0.0 and float(gvb[:, 3:].abs().max()) > 0.0


def test_loss_inputs_stay_clear_of_the_clamp_and_of_the_bin_thresholds():
    T = od.GaussianTables(1000)
    for mt in lv.MEAN_TYPES:
        for vt in lv.VAR_TYPES:
            c = lv.loss_case(T, mt, vt)
            x0 = c["x0"]
            edge = x0.abs() == 1.0
            assert int((x0 == 1.0).sum()) > 3 and int((x0 == -1.0).sum()) > 3
            assert bool(((x0.abs() - 0.999).abs() > 1e-3)[~edge].all()) and float(x0.abs().max()) == 1.0
            assert bool(edge[:2].any()) and bool((x0[:2] == 1.0).any()) and bool((x0[:2] == -1.0).any())  # among the t == 0 samples
            p = lv.hybrid_parts(c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], mt, vt)
            assert float(p["prob"][p["first"]].min()) > 1e-11


def test_samplers_and_modelization_accept_the_learned_types():
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion
    from diffulab_amd.diffuse.samplers.gaussian_diffusion import DDIM, DDPM

    for cls in (DDPM, DDIM):
        for vt in lv.VAR_TYPES:
            s = cls(var_type=vt)
            s.set_steps(torch.from_numpy(od.beta_schedule(1000)))
            a, b = s._variance_tables()
            assert s.learned_variance and torch.equal(a, s.posterior_log_variance_clipped) and torch.equal(b, s.betas)
            with pytest.raises(AssertionError):
                s._check_halves(torch.zeros(2, 4, 8, 8), torch.zeros(2, 4, 8, 8))
            with pytest.raises(AssertionError):
                s._check_halves(torch.zeros(2, 7, 8, 8), torch.zeros(2, 4, 8, 8))
            s._check_halves(torch.zeros(2, 8, 8, 8), torch.zeros(2, 4, 8, 8))
        assert not cls().learned_variance
    assert GaussianDiffusion(n_steps=1000, sampler_parameters={"var_type": "learned_range"}).vlb_weight == 1.0
    assert GaussianDiffusion(n_steps=4000, sampler_parameters={"var_type": "learned"}).vlb_weight == 4.0
    assert GaussianDiffusion(n_steps=1000, vlb_weight=0.001).vlb_weight == 0.001


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from diffulab_amd import _lib

    L = _lib.lib()
    c = L.cdll
    buf = ctypes.create_string_buffer(1024)
    P = ctypes.c_void_p(ctypes.addressof(buf))  # a non-null dummy, never dereferenced: the calls below are refused on the host
    i64, F = ctypes.c_int64, ctypes.c_float

    def refused(name, *args):
        assert getattr(c, name)(*args) == -1 and name in c.dl_last_error().decode(), (name, c.dl_last_error().decode())

    refused("dl_ddpm_step_lv", P, None, F(0), P, P, P, P, 1000, 0, 2, 0, P, P, P, P, P, i64(2), i64(64), None)  # var_mode
    refused("dl_ddpm_step_lv", P, None, F(0), P, P, P, P, 1000, 3, 1, 0, P, P, P, P, P, i64(2), i64(64), None)  # mean_type
    refused("dl_ddpm_step_lv", P, None, F(0), P, P, P, P, 1000, 0, 1, 0, P, P, P, P, P, i64(0), i64(64), None)  # batch
    refused("dl_ddim_step_lv", P, None, F(0), P, P, P, P, 1000, 2, None, 0, F(0), P, P, P, None, None, i64(2), i64(64), None)  # coefs
    refused("dl_vlb_loss_fwd", P, P, P, P, P, P, 1000, 0, 5, P, P, i64(2), i64(64), None)
    refused("dl_vlb_loss_fwd", P, P, None, P, P, P, 1000, 0, 1, P, P, i64(2), i64(64), None)
    refused("dl_vlb_loss_bwd", P, P, P, P, P, P, 1000, 0, 1, None, None, None, i64(2), i64(64), None)
