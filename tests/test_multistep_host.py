"""CPU checks of the second-order multistep samplers "ab2" (rectified flow) and "dpmpp_2m" (Gaussian diffusion): the step coefficients,
the order of both solvers on a closed-form model, the history rule of the product samplers (driven on the CPU with `ops` replaced by
the f32 restatement of tests/multistep_common.py), the refusals, the C declarations, and the per-element bound functions the GPU tests
use."""

import ctypes
import math

import pytest
import torch

import guidance_common as gc
import image_cond_common as ic
import multistep_common as mc
from oracle import diffusion as od
from oracle import synth

SHAPE = (2, 3, 5, 7)
MEAN_NAMES = ("epsilon", "xstart", "xprev", "v")
CHAINS = [(sched, n) for sched in ("linear", "cosine") for n in (1000, 5, 20, 250)]


def chain(sched, n):
    return od.GaussianTables(1000, n_steps=n, schedule=sched)


def product_sampler(sched, n, **kw):
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion

    g = GaussianDiffusion(n_steps=1000, sampling_method="dpmpp_2m", schedule=sched, sampler_parameters=kw)
    if n != 1000:
        g.set_steps(n, schedule=sched)
    return g


# ------------------------------------------------------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("sched,n", CHAINS)
def test_dpmpp_coefficients(sched, n):
    T = chain(sched, n)
    g = product_sampler(sched, n)
    assert torch.equal(g.sampler.alphas_bar, T.alphas_bar)  # the sampler's table is the (respaced) chain's
    ab = [float(v) for v in T.alphas_bar]
    for t in range(n):
        for second in (False, True):
            second = second and 2 <= t < n - 1
            a, b, c = mc.dpmpp_coefs(ab, t, second)
            assert all(math.isfinite(v) for v in (a, b, c)), (t, second, a, b, c)
            got = g.sampler.coefficients(t, second)
            assert all(abs(p - q) <= 1e-12 * max(1.0, abs(q)) for p, q in zip(got, (a, b, c))), (t, second, got, (a, b, c))
            if t == 0:
                assert (a, b, c) == (0.0, 1.0, 0.0) == got
                continue
            # a constant x0 is reproduced: x_t = alpha_t x0 gives x_prev = alpha_{t-1} x0
            assert abs(a * math.sqrt(ab[t]) + b + c - math.sqrt(ab[t - 1])) <= 1e-12
            if not second:  # the DDIM eta = 0 step alpha_{t-1} x0 + sigma_{t-1} eps with eps = (x_t - alpha_t x0) / sigma_t
                s_t, s_p = math.sqrt(1 - ab[t]), math.sqrt(1 - ab[t - 1])
                assert c == 0.0 and abs(a - s_p / s_t) <= 1e-14 and abs(b - (math.sqrt(ab[t - 1]) - s_p * math.sqrt(ab[t]) / s_t)) <= 1e-12
    # the steps at t == 1 and t == 0 stay first order whatever is asked
    assert g.sampler.coefficients(1, True) == g.sampler.coefficients(1, False) and g.sampler.coefficients(0, True) == (0.0, 1.0, 0.0)
    assert mc.dpmpp_coefs(ab, 1, True) == mc.dpmpp_coefs(ab, 1, False)


def test_ab2_weight_is_finite_on_the_grids_and_one_half_on_a_uniform_one():
    from diffulab_amd.diffuse.modelizations.flow import Flow

    assert mc.ab2_weight(0.25, 0.25) == 0.5
    uniform = [1.0, 0.75, 0.5, 0.25, 0.0]
    assert all(mc.ab2_weight(b - c, a - b) == 0.5 for a, b, c in zip(uniform, uniform[1:], uniform[2:]))
    for n in (5, 10, 20, 40, 250):
        for shift in (None, 3.0):
            f = Flow(n_steps=n, sampling_method="ab2")
            f.set_steps(n, shift=shift)
            ts = f.timesteps
            assert ts == od.flow_timesteps(n, shift)
            ws = [mc.ab2_weight(b - c, a - b) for a, b, c in zip(ts, ts[1:], ts[2:])]
            assert all(math.isfinite(w) and w > 0 for w in ws)
            if shift is None:
                assert all(abs(w - 0.5) < 1e-5 for w in ws)


# ------------------------------------------------------------------------------------------------------------------ order
def _err(x, exact):
    return float((x - exact).abs().max())


def test_ab2_order_on_the_closed_form_model():
    x1 = synth.normal("ms.x1", (4096,)).double()
    exact = mc.flow_exact(x1)
    for shift in (None, 3.0):
        for N in (10, 20, 40):
            ts = od.flow_timesteps(N, shift)
            e1, e2 = _err(mc.flow_solve(x1, ts, "euler"), exact), _err(mc.flow_solve(x1, ts, "ab2"), exact)
            print(f"\nflow shift {shift} N {N}: euler {e1:.4g}  ab2 {e2:.4g}")
            assert e2 <= 0.5 * e1, (shift, N, e1, e2)
    for N in (10, 20, 40):
        e, e2n = (_err(mc.flow_solve(x1, od.flow_timesteps(k), "ab2"), exact) for k in (N, 2 * N))
        print(f"\nflow N {N}: err(N) / err(2N) = {e / e2n:.3g}")
        assert e / e2n >= 3, (N, e, e2n)


def test_dpmpp_2m_order_on_the_closed_form_model():
    xT = synth.normal("ms.x1", (4096,)).double()
    for sched in ("linear", "cosine"):
        for n in (20, 40, 80):
            ab = chain(sched, n).alphas_bar
            exact = mc.gauss_exact(xT, float(ab[-1]))
            e1, e2 = _err(mc.gauss_solve(xT, ab, "ddim"), exact), _err(mc.gauss_solve(xT, ab, "dpmpp_2m"), exact)
            print(f"\n{sched} n {n}: ddim {e1:.4g}  dpmpp_2m {e2:.4g}")
            assert e2 <= 0.5 * e1, (sched, n, e1, e2)
    # the reason for the rule: with the step at t == 1 left second order the solver misses the same bound
    ab = chain("linear", 20).alphas_bar
    exact = mc.gauss_exact(xT, float(ab[-1]))
    e1, bad = _err(mc.gauss_solve(xT, ab, "ddim"), exact), _err(mc.gauss_solve(xT, ab, "dpmpp_2m", last_two_first_order=False), exact)
    print(f"\nlinear n 20, only t == 0 first order: ddim {e1:.4g}  dpmpp_2m {bad:.4g}")
    assert not bad <= 0.5 * e1, (e1, bad)


# ------------------------------------------------------------------------------------------------------------------ history rule
class Recorder:
    """`ops` on the CPU: the f32 restatement stands in for the kernels and every step launch is recorded as 1 (no history) or 2"""

    def __init__(self, monkeypatch):
        from diffulab_amd import ops

        self.orders: list[int] = []
        self.batches: list[int] = []
        for name in ("ab2_step", "dpmpp_2m_step", "cfg_rescale_coef", "inpaint_blend", "flow_add_noise", "ddpm_add_noise"):
            monkeypatch.setattr(ops, name, getattr(self, name))

    def ab2_step(self, x, v, vu, g, mul, v_last, t_curr, t_prev, w=0.0, out=None):
        self.orders.append(1 if v_last is None else 2)
        self.batches.append(x.shape[0])
        o = mc.ab2_step(x, v, vu, g, mul, v_last, mc.f32r(t_curr), mc.f32r(t_curr - t_prev), mc.f32r(w), torch.float32)
        return o["x_prev"], o["estimated_x0"], o["v_out"]

    def dpmpp_2m_step(self, pred, pu, g, mul, thr, xt, x0_last, t, tables, mean_type, var_mode, clamp_x, a, b, c, out=None):
        assert x0_last is not None or c == 0.0
        self.orders.append(1 if x0_last is None else 2)
        self.batches.append(xt.shape[0])
        o = mc.dpmpp_step(tables, pred, pu, g, mul, thr, xt, x0_last, t, MEAN_NAMES[mean_type], "fixed", clamp_x, mc.f32r(a), mc.f32r(b),
                          mc.f32r(c), torch.float32)
        return o["x_prev"], o["estimated_x0"]

    @staticmethod
    def cfg_rescale_coef(pred, pu, g, phi, halves=False, out=None):
        return gc.rescale_coef(pred, pu, g, phi, torch.float32)

    @staticmethod
    def inpaint_blend(x, ref, noise, mask, a, b, out=None):
        r = ic.blend_ref(x, ref, noise, mask, mc.f32r(a), mc.f32r(b), torch.float32)
        return r if out is None else out.copy_(r)

    @staticmethod
    def flow_add_noise(x, noise, t, out=None):
        tt = t.float().view(-1, *([1] * (x.dim() - 1)))
        return (1 - tt) * x + tt * noise

    @staticmethod
    def ddpm_add_noise(x, noise, t, sab, ab, out=None):
        shape = (-1,) + (1,) * (x.dim() - 1)
        return sab[t.long()].view(shape) * x + (1 - ab[t.long()]).sqrt().view(shape) * noise


def hand_out(monkeypatch, noises):
    it = iter(noises)
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: next(it).to(device=ref.device, dtype=ref.dtype))
    monkeypatch.setattr(torch, "randn", lambda *size, device=None, dtype=None, **kw: next(it).to(device=device, dtype=dtype or torch.float32))


def make(flow, steps=6):
    from diffulab_amd import Diffuser

    if flow:
        model = gc.Stub(1.0)
        return Diffuser(model, sampling_method="ab2", model_type="rectified_flow", n_steps=steps), model
    model = gc.Stub(1.0 / 1000)
    d = Diffuser(model, sampling_method="dpmpp_2m", model_type="gaussian_diffusion", n_steps=1000, extra_args={"schedule": "cosine"})
    d.set_steps(steps, schedule="cosine")
    return d, model


def inputs():
    y = synth.integers("msh.y", (SHAPE[0],), 10).float()
    return y, [synth.normal(f"msh.nz.{i}", SHAPE) for i in range(40)]


@pytest.mark.parametrize("flow", [True, False])
def test_a_plain_run_is_first_order_once_and_where_the_rule_says(flow, monkeypatch):
    rec = Recorder(monkeypatch)
    y, noises = inputs()
    k = 6
    d, model = make(flow, k)
    want_orders = [1] + [2] * (k - 1) if flow else [1] + [2] * (k - 3) + [1, 1]
    for run in range(2):  # two calls in a row both start first order
        rec.orders.clear()
        hand_out(monkeypatch, noises)
        out = d.generate({"y": y}, data_shape=SHAPE, use_tqdm=False, return_intermediates=True)
        assert rec.orders == want_orders, (run, rec.orders)
        orders: list[int] = []
        if flow:
            ref = mc.flow_loop(gc.Stub(1.0), od.flow_timesteps(k), y, noises, dtype=torch.float32, orders=orders)
        else:
            ref = mc.gaussian_loop(gc.Stub(1.0 / 1000), od.GaussianTables(1000, n_steps=k, schedule="cosine"), 1000, y, noises,
                                   dtype=torch.float32, orders=orders)
        assert orders == want_orders and model.calls == k * (run + 1)
        assert torch.allclose(out["x"], ref["x"], rtol=0, atol=1e-5) and torch.allclose(out["xt"], torch.stack(ref["xt"], dim=1), rtol=0, atol=1e-5)
        assert torch.allclose(out["estimated_x0"], torch.stack(ref["x0"], dim=1), rtol=0, atol=1e-5)
        assert set(out) == ({"x", "xt", "estimated_x0"} if flow else {"x", "xt", "estimated_x0", "xt_mean"})
        assert d.diffusion.sampler._last is None  # the image-sized history tensor is let go when the loop ends
        if not flow:
            assert torch.equal(out["xt_mean"], out["xt"][:, 1:])  # nothing rewrites x_prev in a plain run


@pytest.mark.parametrize("flow", [True, False])
def test_the_rule_needs_no_reset(flow, monkeypatch):
    """with `reset` disabled the conditions alone make a new run, a repeated step and a new batch first order"""
    rec = Recorder(monkeypatch)
    y, noises = inputs()
    d, _ = make(flow, 6)
    monkeypatch.setattr(d.diffusion.sampler, "reset", lambda: None)
    first = None
    for _ in range(2):
        rec.orders.clear()
        hand_out(monkeypatch, noises)
        d.generate({"y": y}, data_shape=SHAPE, use_tqdm=False)
        first = first or list(rec.orders)
        assert rec.orders[0] == 1 and rec.orders == first
    # a change of batch size drops the history: the same next step, one sample fewer
    rec.orders.clear()
    s = d.diffusion.sampler
    x2, x1 = torch.zeros(SHAPE), torch.zeros(1, *SHAPE[1:])
    if flow:
        s.step(x2, x2, 1.0, 0.75), s.step(x2, x2, 0.75, 0.5), s.step(x1, x1, 0.5, 0.25), s.step(x1, x1, 0.25, 0.0)
        s.step(x1, x1, 0.25, 0.0)  # ... and a step whose t_curr is not the last t_prev
    else:
        t = lambda i, x: dict(timesteps=torch.full((x.shape[0],), i, dtype=torch.int32), xt=x, step_index=i)  # noqa: E731
        s.step(x2, **t(5, x2)), s.step(x2, **t(4, x2)), s.step(x1, **t(3, x1)), s.step(x1, **t(2, x1)), s.step(x1, **t(2, x1))
    assert rec.orders == [1, 2, 1, 2, 1] and rec.batches[-5:] == [2, 2, 1, 1, 1]


@pytest.mark.parametrize("flow", [True, False])
def test_every_repeated_step_of_resample_is_first_order(flow, monkeypatch):
    rec = Recorder(monkeypatch)
    y, noises = inputs()
    k, U_ = 6, 3
    d, model = make(flow, k)
    init = synth.uniform("msh.init", SHAPE, lo=-1.0, hi=1.0)
    mask = torch.zeros(SHAPE[0], 1, *SHAPE[2:])
    mask[..., 4:] = 1.0
    hand_out(monkeypatch, noises)
    out = d.generate({"y": y}, data_shape=SHAPE, use_tqdm=False, init_image=init, mask=mask, resample=U_, return_intermediates=True)
    # per step: the first run may use the previous step's last repeat, every repeat after it is first order
    if flow:
        want = [1, 1, 1] + [2, 1, 1] * (k - 2) + [2]
    else:
        want = [1, 1, 1] + [2, 1, 1] * (k - 3) + [1, 1, 1] + [1]  # ... and t == 1, t == 0 are first order anyway
    assert rec.orders == want and model.calls == U_ * (k - 1) + 1
    orders: list[int] = []
    kw = dict(init=init, mask=mask, resample=U_, dtype=torch.float32, orders=orders)
    if flow:
        ref = mc.flow_loop(gc.Stub(1.0), od.flow_timesteps(k), y, noises, **kw)
    else:
        ref = mc.gaussian_loop(gc.Stub(1.0 / 1000), od.GaussianTables(1000, n_steps=k, schedule="cosine"), 1000, y, noises, **kw)
    assert orders == want
    assert torch.allclose(out["x"], ref["x"], rtol=0, atol=1e-5) and torch.allclose(out["xt"], torch.stack(ref["xt"], dim=1), rtol=0, atol=1e-5)
    keep = (mask <= 0).expand(SHAPE)
    assert torch.equal(out["x"][keep], init[keep])
    if not flow:  # xt_mean is x_prev as the step made it: the in-place blend of the known region must not reach it
        want_mean = torch.stack(ref["mean"], dim=1)
        assert torch.allclose(out["xt_mean"], want_mean, rtol=0, atol=1e-5)
        assert torch.equal(out["xt_mean"][:, -1], out["estimated_x0"][:, -1])  # t == 0: the step's x0, not init_image
        assert not torch.equal(out["xt_mean"][:, -1][keep], init[keep]) and not torch.allclose(out["xt_mean"], out["xt"][:, 1:], rtol=0, atol=1e-3)


def test_existing_samplers_have_a_reset_that_does_nothing_and_get_no_step_index(monkeypatch):
    from diffulab_amd.diffuse.modelizations.flow import Flow
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion
    from diffulab_amd.diffuse.samplers.common import Sampler

    for d in (Flow(n_steps=4, sampling_method="euler"), Flow(n_steps=4, sampling_method="euler_maruyama"),
              GaussianDiffusion(sampling_method="ddpm"), GaussianDiffusion(sampling_method="ddim")):
        assert d.sampler.multistep is False and d.sampler.reset() is None and type(d.sampler).reset is Sampler.reset
    assert Flow(sampling_method="ab2").sampler.multistep and GaussianDiffusion(sampling_method="dpmpp_2m").sampler.multistep
    seen = {}
    for name in ("ddim", "dpmpp_2m"):
        g = GaussianDiffusion(n_steps=1000, sampling_method=name)
        monkeypatch.setattr(g.sampler, "step", lambda **kw: seen.update({name: kw}) or {"x_prev": kw["xt"], "estimated_x0": kw["xt"]})
        g.one_step_denoise(gc.Stub(1e-3), {"x": torch.zeros(SHAPE)}, t=7)
    assert "step_index" not in seen["ddim"] and seen["dpmpp_2m"]["step_index"] == 7


def test_the_names_reach_the_yaml_and_set_steps():
    import os

    from diffulab_amd import Diffuser
    from diffulab_amd.config import load_config

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs")
    for top, name in (("train_cifar10_flow_matching", "ab2"), ("train_mnist_ddpm", "dpmpp_2m")):
        cfg = load_config(root, top, [f"diffuser.sampling_method={name}"])
        extra = cfg.diffuser.get("extra_args", {})
        d = Diffuser(gc.Stub(), sampling_method=cfg.diffuser.sampling_method, model_type=cfg.diffuser.model_type,
                     n_steps=cfg.diffuser.n_steps, extra_args={k: extra[k] for k in extra})
        assert d.diffusion.sampler.name == name and d.diffusion.sampler.multistep
        d.set_steps(20)
        assert d.diffusion.steps == 20
        if name == "dpmpp_2m":  # the IDDPM-respaced chain, not the reference's stride-1-only ddim spacing
            T = od.GaussianTables(1000, n_steps=20)
            assert d.diffusion.timestep_map == T.timestep_map and torch.equal(d.diffusion.sampler.alphas_bar, T.alphas_bar)
            assert len(d.diffusion.sampler._ab) == 20
        else:
            assert d.diffusion.timesteps == od.flow_timesteps(20)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_device_work(monkeypatch):
    from diffulab_amd import Diffuser, ops
    from diffulab_amd.diffuse.modelizations.flow import Flow
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion
    from diffulab_amd.diffuse.samplers.gaussian_diffusion import DPMSolverPP2M

    def barred():
        raise RuntimeError("the device library was reached")

    monkeypatch.setattr(ops, "lib", barred)
    monkeypatch.setattr(ops, "_LIB", None)
    with pytest.raises(ValueError, match="xprev"):
        DPMSolverPP2M(mean_type="xprev")
    with pytest.raises(ValueError, match="xprev"):
        Diffuser(gc.Stub(), sampling_method="dpmpp_2m", model_type="gaussian_diffusion", extra_args={"sampler_parameters": {"mean_type": "xprev"}})
    model = gc.Stub()
    d = Diffuser(model, sampling_method="ab2", model_type="rectified_flow", n_steps=4)
    with pytest.raises(ValueError, match="dynamic_threshold.*flow"):
        d.generate({}, data_shape=SHAPE, use_tqdm=False, dynamic_threshold=0.9)
    with pytest.raises(ValueError, match="dynamic_threshold"):
        d.diffusion.sampler.step(torch.zeros(2, 4), torch.zeros(2, 4), 1.0, 0.5, dynamic_threshold=0.9)
    assert model.calls == 0
    with pytest.raises(ValueError, match="eta must be 0"):  # DDIM's keyword is refused by name, not by a TypeError
        GaussianDiffusion(sampling_method="dpmpp_2m").sampler.step(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4),
                                                                   step_index=3, eta=0.5)
    with pytest.raises(ValueError, match="step_index"):
        GaussianDiffusion(sampling_method="dpmpp_2m").sampler.step(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32), torch.zeros(2, 4))
    # an unknown name raises as it did
    with pytest.raises(ValueError, match="sampling method must be one of"):
        GaussianDiffusion(sampling_method="dpmpp_3m")
    with pytest.raises(AssertionError, match="Unknown sampling method"):
        Flow(sampling_method="ab3")
    # ... and the new names do not cross families
    with pytest.raises(ValueError, match="sampling method must be one of"):
        GaussianDiffusion(sampling_method="ab2")
    with pytest.raises(AssertionError, match="Unknown sampling method"):
        Flow(sampling_method="dpmpp_2m")


def test_entry_points_are_declared_exported_and_refuse_bad_arguments_before_any_launch():
    from diffulab_amd import _lib

    protos = _lib.parse_header()
    assert protos["dl_ab2_step"][2] == ["x", "v", "v_uncond", "guidance", "cfg_mul", "v_last", "t_curr", "dt", "w", "x_prev", "x0_est",
                                        "v_out", "batch", "chw", "stream"]
    assert protos["dl_dpmpp_2m_step"][2] == ["pred", "pred_uncond", "guidance", "cfg_mul", "x0_thr", "xt", "x0_last", "t", "tables", "T",
                                             "mean_type", "var_mode", "clamp_x", "a", "b", "c", "x_prev", "x0_est", "batch", "chw", "stream"]
    c = _lib.lib().cdll
    bufs = [ctypes.create_string_buffer(64) for _ in range(4)]
    P, Q, R, S_ = (ctypes.c_void_p(ctypes.addressof(b)) for b in bufs)  # non-null dummies, never dereferenced
    i64, F = ctypes.c_int64, ctypes.c_float

    def refused(name, *args):
        assert getattr(c, name)(*args) == -1 and name in c.dl_last_error().decode(), (name, c.dl_last_error().decode())

    def ab2(x=P, v=P, vl=None, w=0.0, xp=Q, vo=R, B=2, chw=64):
        refused("dl_ab2_step", x, v, None, F(0), None, vl, F(1), F(0.1), F(w), xp, None, vo, i64(B), i64(chw), None)

    ab2(x=None), ab2(v=None), ab2(xp=None), ab2(vo=None), ab2(B=0), ab2(chw=0), ab2(vo=P), ab2(vl=R)
    ab2(vl=S_, w=float("inf")), ab2(vl=S_, w=float("nan"))

    def dpm(pred=P, xt=P, xl=None, t=P, tab=P, T=1000, mt=0, vm=-1, a=0.5, b=0.5, cc=0.0, xp=Q, x0=R, B=2, chw=64):
        refused("dl_dpmpp_2m_step", pred, None, F(0), None, None, xt, xl, t, tab, T, mt, vm, 0, F(a), F(b), F(cc), xp, x0, i64(B),
                i64(chw), None)

    dpm(pred=None), dpm(xt=None), dpm(t=None), dpm(tab=None), dpm(xp=None), dpm(x0=None), dpm(T=0), dpm(B=0), dpm(chw=0)
    dpm(mt=2), dpm(mt=4), dpm(mt=-1), dpm(vm=2), dpm(vm=-2), dpm(a=float("nan")), dpm(b=float("inf")), dpm(cc=0.25)
    dpm(xl=R, cc=0.25), dpm(xl=Q, cc=0.25), dpm(x0=Q)
    refused("dl_dpmpp_2m_step", P, None, F(0), None, None, P, None, P, P, 1000, 2, -1, 0, F(0.5), F(0.5), F(0.0), Q, R, i64(2), i64(64), None)
    assert "mean_type 2" in c.dl_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------ bound functions
def _flow_case(B, chw, cfg, mul, hist):
    x, v, vu, vl = (synth.normal(f"msb.{k}.{B}.{chw}", (B, chw)) for k in ("x", "v", "vu", "vl"))
    m = synth.uniform(f"msb.mul.{B}", (B,), lo=0.6, hi=1.0) if mul else None
    return x, v, vu if cfg else None, m, vl if hist else None


@pytest.mark.parametrize("cfg,mul,hist", [(False, False, False), (True, False, True), (True, True, True), (True, True, False)])
def test_ab2_bounds_admit_the_f32_restatement_and_reject_a_perturbed_coefficient(cfg, mul, hist):
    x, v, vu, m, vl = _flow_case(3, 257, cfg, mul, hist)
    t_curr, dt, w = mc.f32r(0.7), mc.f32r(0.7 - 0.55), mc.f32r(mc.ab2_weight(0.15, 0.1))
    args = (x, v, vu, 3.0, m, vl, t_curr, dt, w)
    ref, r32, bound = mc.ab2_step(*args, torch.float64), mc.ab2_step(*args, torch.float32), mc.ab2_bounds(*args)
    for k in ref:
        assert r32[k].dtype == torch.float32 and bool(((r32[k].double() - ref[k]).abs() <= bound[k]).all()), k
    e = 1 + 2.0**-10
    off = mc.ab2_step(x, v, vu, 3.0, m, vl, t_curr, dt * e, w, torch.float64)
    assert bool(((off["x_prev"] - ref["x_prev"]).abs() > bound["x_prev"]).any())
    off = mc.ab2_step(x, v, vu, 3.0, m, vl, t_curr * e, dt, w, torch.float64)
    assert bool(((off["estimated_x0"] - ref["estimated_x0"]).abs() > bound["estimated_x0"]).any())
    if hist:
        off = mc.ab2_step(x, v, vu, 3.0, m, vl, t_curr, dt, w * e, torch.float64)
        assert bool(((off["x_prev"] - ref["x_prev"]).abs() > bound["x_prev"]).any())
    if cfg:
        off = mc.ab2_step(x, v, vu, 3.0 * e, m, vl, t_curr, dt, w, torch.float64)
        assert bool(((off["v_out"] - ref["v_out"]).abs() > bound["v_out"]).any())


@pytest.mark.parametrize("mean_type", ["epsilon", "xstart", "v"])
@pytest.mark.parametrize("t_idx,second", [(999, False), (500, True), (2, True), (1, False)])
def test_dpmpp_bounds_admit_the_f32_restatement_and_reject_a_perturbed_coefficient(mean_type, t_idx, second):
    T = chain("linear", 1000)
    tab = torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.alphas_bar_prev]).float()
    B, chw = 3, 257
    pred, pu, xt, xl = (synth.normal(f"msb.g.{k}", (B, chw)) for k in ("pred", "pu", "xt", "xl"))
    m, thr = synth.uniform("msb.g.mul", (B,), lo=0.6, hi=1.0), synth.uniform("msb.g.thr", (B,), lo=1.0, hi=2.0)
    t = torch.full((B,), t_idx, dtype=torch.int32)
    a, b, c = (mc.f32r(v) for v in mc.dpmpp_coefs(T.alphas_bar, t_idx, second))
    for with_thr in (False, True):
        th = thr if with_thr else None
        last = xl if second else None
        args = (tab, pred, pu, 3.0, m, th, xt, last, t, mean_type, "fixed")
        ref, r32 = mc.dpmpp_step(*args, with_thr, a, b, c, torch.float64), mc.dpmpp_step(*args, with_thr, a, b, c, torch.float32)
        bound = mc.dpmpp_bounds(*args, a, b, c)
        for k in ref:
            assert r32[k].dtype == torch.float32 and bool(((r32[k].double() - ref[k]).abs() <= bound[k]).all()), (k, with_thr)
        e = 1 + 2.0**-10
        for pa, pb, pc in ((a * e, b, c), (a, b * e, c)) + (((a, b, c * e),) if second else ()):
            off = mc.dpmpp_step(*args, with_thr, pa, pb, pc, torch.float64)
            assert bool(((off["x_prev"] - ref["x_prev"]).abs() > bound["x_prev"]).any()), (pa, pb, pc)
