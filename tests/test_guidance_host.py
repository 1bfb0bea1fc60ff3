"""CPU checks of guided sampling (CFG rescale, guidance interval, dynamic thresholding): the argument validation of
`Diffuser.generate` / `Diffusion.denoise`, the restatement of tests/guidance_common.py against torch.quantile and against the
definitions, the interval arithmetic of both families, and the new C entry points, which refuse bad arguments before any device work.
"""

import ctypes

import pytest
import torch

import guidance_common as gc
from oracle import diffusion as od
from oracle import synth


def _diffuser(flow: bool, **kw):
    from diffulab_amd import Diffuser

    model = gc.Stub()
    if flow:
        return Diffuser(model, sampling_method="euler", model_type="rectified_flow", n_steps=6, **kw), model
    return Diffuser(model, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000, **kw), model


# ------------------------------------------------------------------------------------------------------------------ validation
BAD = [
    (dict(guidance_scale=5, guidance_rescale=-0.1), "guidance_rescale"),
    (dict(guidance_scale=5, guidance_rescale=1.5), "guidance_rescale"),
    (dict(guidance_scale=5, guidance_rescale="0.5"), "guidance_rescale"),
    (dict(guidance_scale=5, guidance_rescale=float("nan")), "guidance_rescale"),
    (dict(guidance_scale=5, guidance_interval=(0.7, 0.3)), "guidance_interval"),
    (dict(guidance_scale=5, guidance_interval=(-0.1, 0.3)), "guidance_interval"),
    (dict(guidance_scale=5, guidance_interval=(0.1, 1.3)), "guidance_interval"),
    (dict(guidance_scale=5, guidance_interval=0.5), "guidance_interval"),
    (dict(guidance_scale=5, guidance_interval=(0.1, 0.2, 0.3)), "guidance_interval"),
    (dict(dynamic_threshold=0.0), "dynamic_threshold"),
    (dict(dynamic_threshold=1.01), "dynamic_threshold"),
    (dict(dynamic_threshold=True), "dynamic_threshold"),
    (dict(dynamic_threshold=0.9, threshold_max=0.5), "threshold_max"),
    (dict(threshold_max=2.0), "threshold_max"),
    (dict(guidance_scale=0, guidance_rescale=0.5), "guidance_rescale"),
    (dict(guidance_scale=0, guidance_interval=(0.2, 0.8)), "guidance_interval"),
]


@pytest.mark.parametrize("kw,name", BAD)
def test_every_validation_rule_names_its_argument(kw, name):
    from diffulab_amd.diffuse.utils import check_guidance

    with pytest.raises(ValueError, match=name):
        check_guidance(**{"guidance_scale": 0, **kw})
    d, model = _diffuser(flow=False)
    with pytest.raises(ValueError, match=name):  # before any device work: the stub lives on the CPU and is never called
        d.generate({}, data_shape=(2, 1, 4, 4), use_tqdm=False, **kw)
    assert model.calls == 0
    if "dynamic_threshold" not in kw and "threshold_max" not in kw:
        d, model = _diffuser(flow=True)
        with pytest.raises(ValueError, match=name):
            d.generate({}, data_shape=(2, 1, 4, 4), use_tqdm=False, **kw)
        assert model.calls == 0


def test_flow_refuses_the_dynamic_threshold_and_says_why():
    d, model = _diffuser(flow=True)
    with pytest.raises(ValueError, match="dynamic_threshold.*flow.*x0 clamp"):
        d.generate({}, data_shape=(2, 1, 4, 4), use_tqdm=False, dynamic_threshold=0.995)
    with pytest.raises(ValueError, match="dynamic_threshold"):
        d.diffusion.one_step_denoise(model, {"x": torch.zeros(2, 1, 4, 4)}, t_prev=0.5, t_curr=1.0, guidance_scale=0, dynamic_threshold=0.9)
    with pytest.raises(ValueError, match="dynamic_threshold"):
        d.diffusion.sampler.step(torch.zeros(2, 4), torch.zeros(2, 4), 1.0, 0.5, dynamic_threshold=0.9)
    assert model.calls == 0


def test_good_arguments_pass_validation():
    from diffulab_amd.diffuse.utils import check_guidance

    assert check_guidance(0) is False and check_guidance(5) is False
    assert check_guidance(5, 0.7) and check_guidance(5, 1.0, (0.0, 1.0), 1.0, 1.0) and check_guidance(0, dynamic_threshold=0.995)
    assert check_guidance(5, guidance_interval=[0.3, 0.3])


@pytest.mark.parametrize("flow", [True, False])
def test_defaults_do_not_reach_denoise_as_keywords(flow, monkeypatch):
    d, _ = _diffuser(flow)
    seen = []
    monkeypatch.setattr(d.diffusion, "denoise", lambda model, **kw: seen.append(kw) or {"x": torch.zeros(1)})
    new = ("guidance_rescale", "guidance_interval", "dynamic_threshold", "threshold_max")
    d.generate({}, data_shape=(1, 1, 2, 2), use_tqdm=False, guidance_scale=3)
    d.generate({}, data_shape=(1, 1, 2, 2), use_tqdm=False, guidance_scale=3, guidance_rescale=0.0, guidance_interval=None,
               dynamic_threshold=None, threshold_max=None)
    assert len(seen) == 2 and seen[0] == seen[1] and not set(new) & set(seen[0])
    d.generate({}, data_shape=(1, 1, 2, 2), use_tqdm=False, guidance_scale=3, guidance_rescale=0.7, guidance_interval=(0.2, 0.8))
    assert seen[2]["guidance_rescale"] == 0.7 and seen[2]["guidance_interval"] == (0.2, 0.8) and "dynamic_threshold" not in seen[2]


# ------------------------------------------------------------------------------------------------------------------ the quantile
def _rows(n, kind):
    if kind == "normal":
        return synth.normal(f"gh.q.{n}", (3, n))
    base = torch.tensor([0.25, -0.25, 1.5, -3.0, 0.0])  # ties, also between a value and its negative
    return base[(torch.arange(3 * n) * 7) % 5].view(3, n).contiguous()


@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("p", [1e-3, 0.5, 0.995, 1.0])
@pytest.mark.parametrize("n", [1, 2, 7, 257])
def test_restated_quantile_is_torch_quantile_in_f64(n, p, kind):
    x = _rows(n, kind)
    want = torch.quantile(x.abs().double(), p, dim=1)
    got = gc.abs_quantile(x, p, torch.float64)
    k, f = gc.quantile_position(p, n)
    assert 0 <= k < n and 0.0 <= f < 1.0
    # the only difference to torch's own evaluation is the f32 rounding of the fraction f
    assert float((got - want).abs().max()) <= 2.0**-24 * float(x.abs().max()) + 1e-300, (got, want)
    if kind == "ties" or p == 1.0 or n == 1:
        lo, hi = gc.order_stats(x, k)
        if bool((lo == hi).all()):
            assert torch.equal(got, want)


def test_quantile_position_matches_the_product():
    from diffulab_amd.diffuse.utils import quantile_position

    for n in (1, 2, 7, 257, 1024, 3072, 196608):
        for p in (1e-3, 0.5, 0.995, 1.0, 1.0 - 2.0**-40):
            k, f = quantile_position(p, n)
            assert (k, f) == gc.quantile_position(p, n) and 0 <= k < n and 0.0 <= f < 1.0
    assert quantile_position(1.0, 7) == (6, 0.0) and quantile_position(0.5, 2) == (0, 0.5) and quantile_position(0.3, 1) == (0, 0.0)


# ------------------------------------------------------------------------------------------------------------------ the rescale
def test_restated_rescale():
    c, u = synth.normal("gh.c", (3, 4, 5, 7)), synth.normal("gh.u", (3, 4, 5, 7))
    for g in (1.5, 7.0):
        assert torch.equal(gc.rescale_coef(c, u, g, 0.0), torch.ones(3, dtype=torch.float64))
        r = gc.rescale_coef(c, u, g, 1.0)
        o = (u.double() + g * (c.double() - u.double())).flatten(1)
        assert torch.allclose((r[:, None] * o).std(dim=1), c.double().flatten(1).std(dim=1), rtol=1e-13, atol=0)
        half = gc.rescale_coef(c, u, g, 0.5)
        assert torch.allclose(half, 0.5 + 0.5 * r, rtol=1e-15, atol=0)
    # S_o == 0: a constant combined prediction, and n == 1
    flat = torch.full((2, 3, 4), 0.75)
    assert torch.equal(gc.rescale_coef(flat, flat, 3.0, 1.0), torch.ones(2, dtype=torch.float64))
    assert torch.equal(gc.rescale_coef(c[:, :1, :1, :1], u[:, :1, :1, :1], 3.0, 1.0), torch.ones(3, dtype=torch.float64))
    # the variance half of a 2C prediction keeps the plain combine
    pred, pu = synth.normal("gh.p2", (2, 6, 5)), synth.normal("gh.u2", (2, 6, 5))
    o = gc.guided(pred, pu, 3.0, 1.0, True)
    plain = pu.double() + 3.0 * (pred.double() - pu.double())
    assert torch.equal(o[:, 3:], plain[:, 3:]) and not torch.equal(o[:, :3], plain[:, :3])
    assert torch.allclose(o[:, :3].flatten(1).std(dim=1), pred[:, :3].double().flatten(1).std(dim=1), rtol=1e-13, atol=0)


def test_restated_threshold():
    x0 = synth.normal("gh.x0", (3, 2, 5, 7), std=2.0)
    s = gc.threshold_of(x0, 0.9, None)
    assert bool((s >= 1).all()) and torch.equal(s, gc.abs_quantile(x0.flatten(1), 0.9).clamp_min(1.0))
    assert torch.equal(gc.threshold_of(x0, 0.9, 1.25), s.clamp_max(1.25))
    y = gc.apply_threshold(x0.double(), s)
    assert float(y.abs().max()) <= 1.0 and torch.equal(y, x0.double().clamp(-s.view(3, 1, 1, 1), s.view(3, 1, 1, 1)) / s.view(3, 1, 1, 1))
    small = 0.5 * torch.tanh(x0)
    assert torch.equal(gc.apply_threshold(small.double(), gc.threshold_of(small, 0.995, None)), small.double())


# ------------------------------------------------------------------------------------------------------------------ the interval
def test_interval_arithmetic_of_both_families():
    from diffulab_amd.diffuse.modelizations.flow import Flow
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion
    from diffulab_amd.diffuse.utils import in_guidance_interval

    assert in_guidance_interval(None, 0.5) and in_guidance_interval((0.3, 0.7), 0.3) and in_guidance_interval((0.3, 0.7), 0.7)
    assert not in_guidance_interval((0.3, 0.7), 0.7000001) and not in_guidance_interval((0.3, 0.7), 0.2999999)
    # flow: level = t_curr on the grid 1, 0.9, ..., 0.1
    f = Flow(n_steps=10)
    levels = f.timesteps[:-1]
    assert sum(in_guidance_interval((0.3, 0.7), t) for t in levels) == gc.guided_steps_flow(od.flow_timesteps(10), (0.3, 0.7))
    assert gc.guided_steps_flow(od.flow_timesteps(10), (0.0, 1.0)) == 10 and gc.guided_steps_flow(od.flow_timesteps(10), (0.0, 0.05)) == 0
    # Gaussian diffusion, the full chain: level = (t + 1) / T, both ends inclusive
    g = GaussianDiffusion(n_steps=1000)
    assert g.guidance_level(0) == 1 / 1000 and g.guidance_level(999) == 1.0 and g.guidance_level(299) == 0.3
    assert [t for t in range(1000) if in_guidance_interval((0.3, 0.7), g.guidance_level(t))] == list(range(299, 700))
    # a respaced chain reads the training index the denoiser is given
    g.set_steps(6, schedule="cosine")
    T = od.GaussianTables(1000, n_steps=6, schedule="cosine")
    assert g.timestep_map == T.timestep_map and len(T.timestep_map) == 6
    for t in range(6):
        assert g.guidance_level(t) == (T.timestep_map[t] + 1) / 1000 == gc.gaussian_level(T.timestep_map, 1000, t)
    want = [t for t in range(6) if 0.3 <= (T.timestep_map[t] + 1) / 1000 <= 0.7]
    assert [t for t in range(6) if in_guidance_interval((0.3, 0.7), g.guidance_level(t))] == want and 0 < len(want) < 6
    assert gc.guided_steps_gaussian(T, 1000, (0.3, 0.7)) == len(want)
    edge = (T.timestep_map[2] + 1) / 1000  # an interval that ends exactly on a step includes it
    assert in_guidance_interval((edge, edge), g.guidance_level(2)) and not in_guidance_interval((edge, edge), g.guidance_level(3))


def test_unguided_steps_make_one_forward_on_the_host_path(monkeypatch):
    """the loop's bookkeeping without a device: the sampler step is replaced, the forwards are counted"""
    for flow in (True, False):
        d, model = _diffuser(flow)
        seen = []

        def step(*a, **kw):
            seen.append(kw)
            x = kw.get("xt", a[0] if a else None)
            return {"x_prev": x, "estimated_x0": x}

        monkeypatch.setattr(d.diffusion.sampler, "step", step)
        if not flow:
            d.set_steps(6, schedule="cosine")
        x = torch.zeros(2, 1, 4, 4)
        d.generate({"x": x, "y": torch.zeros(2)}, use_tqdm=False, guidance_scale=5, guidance_rescale=0.7, guidance_interval=(0.3, 0.7))
        if flow:
            n_guided = gc.guided_steps_flow(od.flow_timesteps(6), (0.3, 0.7))
        else:
            n_guided = gc.guided_steps_gaussian(od.GaussianTables(1000, n_steps=6, schedule="cosine"), 1000, (0.3, 0.7))
        assert 0 < n_guided < 6 and model.calls == 6 + n_guided and len(seen) == 6
        assert all(kw["guidance_rescale"] == 0.7 for kw in seen)
        assert sum("guidance_scale" in kw and kw["guidance_scale"] > 0 for kw in seen) == n_guided


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_new_entry_points_are_exported_and_none_is_named_dl_f32():
    from diffulab_amd import _lib

    protos = _lib.parse_header()
    for name in gc.NEW_ENTRY_POINTS:
        assert name in protos and not name.startswith("dl_f32_")
    L = _lib.lib()
    for name in gc.NEW_ENTRY_POINTS:
        assert hasattr(L.cdll, name)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from diffulab_amd import _lib

    c = _lib.lib().cdll
    buf = ctypes.create_string_buffer(1024)
    P = ctypes.c_void_p(ctypes.addressof(buf))  # a non-null dummy, never dereferenced: the calls below are refused on the host
    i64, F = ctypes.c_int64, ctypes.c_float
    INF = float("inf")

    def refused(name, *args):
        assert getattr(c, name)(*args) == -1 and name in c.dl_last_error().decode(), (name, c.dl_last_error().decode())

    # dl_cfg_rescale_coef(pred, pred_uncond, guidance, phi, r, batch, chw, sample_stride, stream)
    def coef(pred=P, pu=P, phi=0.5, r=P, B=2, chw=64, stride=64):
        refused("dl_cfg_rescale_coef", pred, pu, F(3), F(phi), r, i64(B), i64(chw), i64(stride), None)

    coef(pred=None), coef(pu=None), coef(r=None), coef(B=0), coef(chw=0), coef(chw=-3), coef(stride=65), coef(stride=192)
    coef(phi=-0.1), coef(phi=1.1), coef(phi=float("nan"))

    # dl_abs_quantile_rows(x, k, f, q, lohi, batch, n, stream)
    def quant(x=P, k=0, f=0.0, q=P, B=2, n=64):
        refused("dl_abs_quantile_rows", x, i64(k), F(f), q, None, i64(B), i64(n), None)

    quant(x=None), quant(q=None), quant(B=0), quant(n=0), quant(k=-1), quant(k=64), quant(k=65), quant(f=-0.1), quant(f=1.0)
    quant(f=float("nan")), quant(n=1 << 31)

    # dl_x0_threshold(pred, pred_uncond, guidance, cfg_mul, xt, t, tables, T, mean_type, coefs, k, f, threshold_max, s, lohi, batch, chw,
    #                 sample_stride, stream)
    def thr(pred=P, xt=P, t=P, tab=P, T=1000, mt=0, coefs=None, k=0, f=0.0, cap=INF, s=P, B=2, chw=64, stride=64):
        refused("dl_x0_threshold", pred, None, F(0), None, xt, t, tab, T, mt, coefs, i64(k), F(f), F(cap), s, None, i64(B), i64(chw),
                i64(stride), None)

    thr(pred=None), thr(xt=None), thr(t=None), thr(tab=None), thr(s=None), thr(T=0), thr(B=0), thr(chw=0), thr(stride=100)
    thr(k=64), thr(k=-1), thr(f=1.0), thr(f=-0.5), thr(mt=4), thr(mt=-1), thr(mt=2), thr(cap=0.5), thr(cap=float("nan"))

    # dl_euler_step_g(x, v, v_uncond, guidance, cfg_mul, t_curr, dt, x_prev, x0_est, batch, chw, stream)
    def eu(x=P, v=P, xp=P, B=2, chw=64):
        refused("dl_euler_step_g", x, v, None, F(0), P, F(1), F(0.1), xp, P, i64(B), i64(chw), None)

    eu(x=None), eu(v=None), eu(xp=None), eu(B=0), eu(chw=0)

    # dl_euler_maruyama_step_g(x, v, v_uncond, guidance, cfg_mul, noise, x_prev_in, t_curr, dt, sigma, std, x_prev, mean, x0_est, logprob,
    #                          batch, chw, stream)
    def em(x=P, v=P, noise=P, xpin=None, xp=P, B=2, chw=64):
        refused("dl_euler_maruyama_step_g", x, v, None, F(0), P, noise, xpin, F(1), F(0.1), F(0.5), F(0.2), xp, P, P, P, i64(B), i64(chw),
                None)

    em(x=None), em(v=None), em(xp=None), em(B=0), em(chw=0), em(noise=None), em(xpin=P)

    # dl_ddpm_step_g(pred, pred_uncond, guidance, cfg_mul, x0_thr, xt, noise, t, tables, T, mean_type, var_mode, clamp_x, x_prev, x0_est,
    #                mean, std, logprob, batch, chw, stream)
    def ddpm(pred=P, xt=P, noise=P, t=P, tab=P, T=1000, mt=0, vm=-1, xp=P, B=2, chw=64):
        refused("dl_ddpm_step_g", pred, None, F(0), P, P, xt, noise, t, tab, T, mt, vm, 0, xp, P, P, P, P, i64(B), i64(chw), None)

    ddpm(pred=None), ddpm(xt=None), ddpm(noise=None), ddpm(t=None), ddpm(tab=None), ddpm(xp=None), ddpm(T=0), ddpm(B=0), ddpm(chw=0)
    ddpm(mt=4), ddpm(mt=-1), ddpm(vm=2), ddpm(vm=-2)

    # dl_ddim_step_g(pred, pred_uncond, guidance, cfg_mul, x0_thr, xt, noise, t, tables, T, mean_type, var_mode, ddpm_coefs, clamp_x, eta,
    #                x_prev, x0_est, mean, std, logprob, batch, chw, stream)
    def ddim(pred=P, xt=P, noise=P, t=P, tab=P, T=1000, mt=0, vm=-1, coefs=None, xp=P, B=2, chw=64):
        refused("dl_ddim_step_g", pred, None, F(0), P, P, xt, noise, t, tab, T, mt, vm, coefs, 0, F(0), xp, P, P, None, None, i64(B),
                i64(chw), None)

    ddim(pred=None), ddim(xt=None), ddim(noise=None), ddim(t=None), ddim(tab=None), ddim(xp=None), ddim(T=0), ddim(B=0), ddim(chw=0)
    ddim(mt=4), ddim(mt=-1), ddim(vm=2), ddim(vm=-2), ddim(mt=2)
