"""GPU tests of the second-order multistep samplers: the two step kernels (dl_ab2_step, dl_dpmpp_2m_step) element by element against
fp64, their bit identities and write guards, the loops of `Diffuser.generate` with sampling_method "ab2" / "dpmpp_2m" against the
restatement of tests/multistep_common.py, two end-to-end runs on the real engines, and the example.

Kernel bounds, per element and per output (derived in tests/multistep_common.py from the kernels' operation counts; every one is
k * 2^-24 * (the sum of the absolute terms) + 2^-149, k = the longest chain of roundings a term passes through + 1).  With
A = |u| + |g| (|c| + |u|) (|c| without a combine), m = |cfg_mul| (1 without):
    dl_ab2_step       v_out 5 m A;  x0_est 7 (|x| + |t_curr| m A);  x_prev 10 (|x| + |dt| (|1 + w| m A + |w v_last|))
    dl_dpmpp_2m_step  x0_est 11 X / s;  x_prev 15 |b| X / s + 4 (|a xt| + |c x0_last|), where X = |xt| / sab + sigma / sab m A (epsilon),
                      sab |xt| + sigma m A (v), m A (xstart), and s the sample's threshold (1 without)
Inputs are the same f32 values on both sides, the coefficients rounded to f32 as the host passes them.

Loop tolerance, as in tests/test_image_cond_gpu.py: the product may be 4 x as far from the f64 restatement as the f32 restatement is
(both figures come from the restatement and are printed)."""

import itertools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as eb  # noqa: E402
import guidance_common as gc  # noqa: E402
import image_cond_common as ic  # noqa: E402
import multistep_common as mc  # noqa: E402
from oracle import diffusion as od  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(B, chw) for B in (1, 3) for chw in (1, 63, 257)]
G = 3.0
WORST: dict[str, float] = {}


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def T():
    return od.GaussianTables(1000)


def bits(t):
    return t.contiguous().view(torch.int32)


def dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def within(tag, got, ref, bound):
    for k in ref:
        err = (got[k].double().cpu() - ref[k]).abs()
        ratio = float((err / bound[k]).max())
        WORST[f"{tag} {k}"] = max(WORST.get(f"{tag} {k}", 0.0), ratio)
        assert bool(torch.isfinite(got[k]).all()) and int((err > bound[k]).sum()) == 0, (tag, k, ratio)


# ------------------------------------------------------------------------------------------------------------------ dl_ab2_step
def flow_case(B, chw, cfg, mul, hist):
    x, v, vu, vl = (synth.normal(f"msg.{k}.{B}.{chw}", (B, 1, chw)) for k in ("x", "v", "vu", "vl"))
    m = synth.uniform(f"msg.mul.{B}", (B,), lo=0.6, hi=1.0) if mul else None
    return x, v, (vu if cfg else None), m, (vl if hist else None)


FLOW_SCALARS = (0.7, 0.55, 0.1)  # t_curr, t_prev, the previous step's dt: a non-uniform pair of steps


@pytest.mark.parametrize("B,chw", SIZES)
def test_ab2_kernel_against_fp64_element_by_element(ops, B, chw):
    t_curr, t_prev, dt_last = FLOW_SCALARS
    w = mc.ab2_weight(t_curr - t_prev, dt_last)
    for cfg, mul, hist in itertools.product((False, True), repeat=3):
        x, v, vu, m, vl = flow_case(B, chw, cfg, mul, hist)
        args = (x, v, vu, G, m, vl, mc.f32r(t_curr), mc.f32r(t_curr - t_prev), mc.f32r(w))
        ref, bound = mc.ab2_step(*args, torch.float64), mc.ab2_bounds(*args)
        xp, x0, vo = ops.ab2_step(*dev(x, v, vu), G, *dev(m, vl), t_curr, t_prev, w)
        assert xp.shape == x.shape and xp.dtype == torch.float32
        within("dl_ab2_step", {"x_prev": xp, "estimated_x0": x0, "v_out": vo}, ref, bound)


def test_ab2_without_history_is_the_euler_step_bit_for_bit(ops):
    t_curr, t_prev, _ = FLOW_SCALARS
    for (B, chw), cfg, mul in itertools.product(SIZES, (False, True), (False, True)):
        x, v, vu, m, _ = dev(*flow_case(B, chw, cfg, mul, False))
        want_xp, want_x0 = ops.euler_step_g(x, v, vu, G, m, t_curr, t_prev)
        xp, x0, vo = ops.ab2_step(x, v, vu, G, m, None, t_curr, t_prev, float("nan"))  # w is not read
        assert torch.equal(bits(xp), bits(want_xp)) and torch.equal(bits(x0), bits(want_x0)), (B, chw, cfg, mul)
        # the combined v euler_step_g implies: x0_est = 0 - v (-1) returns it exactly
        _, implied = ops.euler_step_g(torch.zeros_like(x), v, vu, G, m, -1.0, 0.0)
        assert torch.equal(bits(vo), bits(implied)), (B, chw, cfg, mul)
        # ... and a second-order step writes the same x0_est and v_out
        vl = synth.normal(f"msg.vl.{B}.{chw}", (B, 1, chw)).to(DEV)
        xp2, x02, vo2 = ops.ab2_step(x, v, vu, G, m, vl, t_curr, t_prev, 0.75)
        assert torch.equal(bits(x02), bits(x0)) and torch.equal(bits(vo2), bits(vo)) and not torch.equal(xp2, xp)


# ------------------------------------------------------------------------------------------------------------------ dl_dpmpp_2m_step
def gauss_case(B, chw, var_type, cfg, hist):
    C = 2 if var_type != "fixed" else 1
    pred, pu = (synth.normal(f"msg.g.{k}.{B}.{chw}.{C}", (B, C, chw)) for k in ("pred", "pu"))
    xt, xl = (synth.normal(f"msg.g.{k}.{B}.{chw}", (B, 1, chw)) for k in ("xt", "xl"))
    return pred, (pu if cfg else None), xt, (xl if hist else None)


def tables(T):
    return torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.alphas_bar_prev]).float()


def var_mode(ops, var_type):
    return ops.VAR_FIXED if var_type == "fixed" else ops.VAR_MODES[var_type]


@pytest.mark.parametrize("var_type", ["fixed", "learned_range"])
@pytest.mark.parametrize("mean_type", ["epsilon", "xstart", "v"])
def test_dpmpp_kernel_against_fp64_element_by_element(ops, T, mean_type, var_type):
    tab = tables(T)
    dtab = tab.to(DEV)
    n = 0
    for (B, chw), cfg, mul, thr, clamp, hist in itertools.product(SIZES, *[(False, True)] * 5):
        t_idx = ((500, 2) if hist else (999, 1, 0))[n % (2 if hist else 3)]
        n += 1
        a, b, c = mc.dpmpp_coefs(T.alphas_bar, t_idx, hist)
        pred, pu, xt, xl = gauss_case(B, chw, var_type, cfg, hist)
        m = synth.uniform(f"msg.g.mul.{B}", (B,), lo=0.6, hi=1.0) if mul else None
        s = synth.uniform(f"msg.g.thr.{B}", (B,), lo=1.0, hi=2.0) if thr else None
        t = torch.full((B,), t_idx, dtype=torch.int32)
        args = (tab, pred, pu, G, m, s, xt, xl, t, mean_type, var_type)
        fa, fb, fc = (mc.f32r(v) for v in (a, b, c))
        ref, bound = mc.dpmpp_step(*args, clamp, fa, fb, fc, torch.float64), mc.dpmpp_bounds(*args, fa, fb, fc)
        xp, x0 = ops.dpmpp_2m_step(*dev(pred, pu), G, *dev(m, s, xt, xl, t), dtab, ops.MEAN_TYPES[mean_type], var_mode(ops, var_type),
                                   clamp, a, b, c)
        assert xp.shape == xt.shape and x0.shape == xt.shape
        within(f"dl_dpmpp_2m_step {mean_type} {var_type}", {"x_prev": xp, "estimated_x0": x0}, ref, bound)
        if t_idx == 0:
            assert (a, b, c) == (0.0, 1.0, 0.0) and torch.equal(bits(xp), bits(x0))


def test_dpmpp_bit_identities(ops, T):
    dtab = tables(T).to(DEV)
    for (B, chw), var_type, mean_type in itertools.product(SIZES, ("fixed", "learned_range"), ("epsilon", "xstart", "v")):
        pred, pu, xt, xl = dev(*gauss_case(B, chw, var_type, True, True))
        t = torch.full((B,), 0, dtype=torch.int32, device=DEV)
        mt, vm = ops.MEAN_TYPES[mean_type], var_mode(ops, var_type)
        # (0, 1, 0): x_prev is x0_est bit for bit, which is the x0 dl_ddim_step_g forms from the same arguments
        xp, x0 = ops.dpmpp_2m_step(pred, pu, G, None, None, xt, None, t, dtab, mt, vm, False, 0.0, 1.0, 0.0)
        assert torch.equal(bits(xp), bits(x0))
        want = ops.ddim_step_g(pred, pu, G, None, None, xt, torch.zeros_like(xt), t, dtab, None, mt, vm, False, 0.0)[1]
        assert torch.equal(bits(x0), bits(want)), (B, chw, var_type, mean_type)
        if mean_type == "xstart":  # ... whatever x_t holds: a zero `a` drops its term
            xp_nan, _ = ops.dpmpp_2m_step(pred, pu, G, None, None, torch.full_like(xt, float("nan")), None, t, dtab, mt, vm, False, 0.0, 1.0, 0.0)
            assert torch.equal(bits(xp_nan), bits(xp))
        # c == 0 reads no history
        t5 = torch.full((B,), 500, dtype=torch.int32, device=DEV)
        first = ops.dpmpp_2m_step(pred, pu, G, None, None, xt, None, t5, dtab, mt, vm, False, 0.9, 0.2, 0.0)
        again = ops.dpmpp_2m_step(pred, pu, G, None, None, xt, torch.full_like(xt, float("nan")), t5, dtab, mt, vm, False, 0.9, 0.2, 0.0)
        assert all(torch.equal(bits(p), bits(q)) for p, q in zip(first, again))


def test_the_threshold_kernel_thresholds_the_x0_the_step_uses(ops, T):
    dtab = tables(T).to(DEV)
    B, chw = 3, 257
    for mean_type, var_type in (("epsilon", "fixed"), ("v", "learned_range")):
        pred, pu, xt, xl = dev(*gauss_case(B, chw, var_type, True, True))
        t = torch.full((B,), 500, dtype=torch.int32, device=DEV)
        mt, vm = ops.MEAN_TYPES[mean_type], var_mode(ops, var_type)
        k, f = gc.quantile_position(0.9, chw)
        s = ops.x0_threshold(pred, pu, G, None, xt, t, dtab, None, mt, k, f, None, var_type != "fixed")
        _, plain = ops.dpmpp_2m_step(pred, pu, G, None, None, xt, None, t, dtab, mt, vm, False, 0.9, 0.2, 0.0)
        _, x0 = ops.dpmpp_2m_step(pred, pu, G, None, s, xt, None, t, dtab, mt, vm, False, 0.9, 0.2, 0.0)
        assert float(plain.abs().max()) > 1.0 and float(x0.abs().max()) <= 1.0
        want = gc.threshold_of(plain.cpu(), 0.9, None, torch.float64)
        assert bool(((s.double().cpu() - want).abs() <= 8 * mc.U * want).all())  # lo + f (hi - lo) in f32: 3 U (|lo| + |hi|)


# ------------------------------------------------------------------------------------------------------------------ write guards
@pytest.mark.parametrize("chw", [1, 63, 257])
def test_outputs_stay_inside_their_windows(ops, T, chw):
    B = 2
    n = B * chw
    t_curr, t_prev, _ = FLOW_SCALARS
    for cfg, mul, hist in itertools.product((False, True), repeat=3):
        x, v, vu, m, vl = dev(*flow_case(B, chw, cfg, mul, hist))
        keep = [None if q is None else q.clone() for q in (x, v, vu, vl)]
        gs = [eb.Guarded(1, n, torch.float32, DEV) for _ in range(3)]
        ops.ab2_step(x, v, vu, G, m, vl, t_curr, t_prev, 0.75, out=tuple(g.win.view(B, 1, chw) for g in gs))
        for g, name in zip(gs, ("x_prev", "x0_est", "v_out")):
            g.check(f"dl_ab2_step chw {chw} {name} cfg {cfg} mul {mul} hist {hist}")
        assert all(q is None or torch.equal(bits(q), bits(k_)) for q, k_ in zip((x, v, vu, vl), keep))
    dtab = tables(T).to(DEV)
    t = torch.full((B,), 500, dtype=torch.int32, device=DEV)
    for var_type, gd, hist in itertools.product(("fixed", "learned_range"), (False, True), (False, True)):
        pred, pu, xt, xl = dev(*gauss_case(B, chw, var_type, True, hist))
        m = synth.uniform("msg.w.mul", (B,), lo=0.6, hi=1.0).to(DEV) if gd else None
        s = synth.uniform("msg.w.thr", (B,), lo=1.0, hi=2.0).to(DEV) if gd else None
        keep = [None if q is None else q.clone() for q in (pred, pu, xt, xl)]
        gs = [eb.Guarded(1, n, torch.float32, DEV) for _ in range(2)]
        ops.dpmpp_2m_step(pred, pu, G, m, s, xt, xl, t, dtab, ops.MEAN_TYPES["epsilon"], var_mode(ops, var_type), True, 0.9, 0.3,
                          -0.1 if hist else 0.0, out=tuple(g.win.view(B, 1, chw) for g in gs))
        for g, name in zip(gs, ("x_prev", "x0_est")):
            g.check(f"dl_dpmpp_2m_step chw {chw} {name} {var_type} guided {gd} hist {hist}")
        assert all(q is None or torch.equal(bits(q), bits(k_)) for q, k_ in zip((pred, pu, xt, xl), keep))  # pred, x0_last untouched


# ------------------------------------------------------------------------------------------------------------------ the loops
STEPS = 6
SHAPE = (2, 3, 5, 7)
TRAINING = 1000
GUIDED = dict(guidance=3.0, phi=0.7)
INTERVALS = {"flow": (0.2, 0.9), "gaussian": (0.1, 0.9)}  # each excludes two of the six steps (asserted below)


def loop_inputs():
    y = synth.integers("msg.y", (SHAPE[0],), 10).float()
    return y, [synth.normal(f"msg.nz.{i}", SHAPE) for i in range(40)]


def chain():
    return od.GaussianTables(TRAINING, n_steps=STEPS, schedule="cosine")


def make(sampler, mean_type):
    from diffulab_amd import Diffuser

    if sampler == "ab2":
        model = gc.Stub(1.0).to(DEV)
        return Diffuser(model, sampling_method="ab2", model_type="rectified_flow", n_steps=STEPS), model
    model = gc.Stub(1.0 / TRAINING).to(DEV)
    extra = {"schedule": "cosine", "sampler_parameters": {"mean_type": mean_type}}
    if mean_type == "v":
        extra["loss_target"] = "mean_type"
    d = Diffuser(model, sampling_method="dpmpp_2m", model_type="gaussian_diffusion", n_steps=TRAINING, extra_args=extra)
    d.set_steps(STEPS, schedule="cosine")
    return d, model


def restate(sampler, mean_type, y, noises, dtype, orders=None, **kw):
    if sampler == "ab2":
        return mc.flow_loop(gc.Stub(1.0), od.flow_timesteps(STEPS), y, noises, dtype=dtype, orders=orders, **kw)
    return mc.gaussian_loop(gc.Stub(1.0 / TRAINING), chain(), TRAINING, y, noises, mean_type, dtype=dtype, orders=orders, **kw)


def hand_out(monkeypatch, noises):
    it = iter(noises)
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: next(it).to(device=ref.device, dtype=ref.dtype))
    monkeypatch.setattr(torch, "randn", lambda *size, device=None, dtype=None, **kw: next(it).to(device=device, dtype=dtype or torch.float32))


@pytest.mark.parametrize("opt", ["plain", "guided", "image", "image_full"])
@pytest.mark.parametrize("sampler,mean_type", [("ab2", "v"), ("dpmpp_2m", "epsilon"), ("dpmpp_2m", "v")])
def test_loops_against_the_restatement(sampler, mean_type, opt, ops, monkeypatch):
    y, noises = loop_inputs()
    kw, gen = {}, {}
    n_guided, k, n_calls = 0, STEPS, STEPS
    if opt == "guided":
        interval = INTERVALS["flow" if sampler == "ab2" else "gaussian"]
        kw = dict(GUIDED, interval=interval)
        gen = dict(guidance_scale=GUIDED["guidance"], guidance_rescale=GUIDED["phi"], guidance_interval=interval)
        n_guided = (gc.guided_steps_flow(od.flow_timesteps(STEPS), interval) if sampler == "ab2"
                    else gc.guided_steps_gaussian(chain(), TRAINING, interval))
        assert n_guided == STEPS - 2
        n_calls = STEPS + n_guided
    if opt.startswith("image"):  # "image": the issue's case; "image_full": every step, so second-order steps meet mask and resample
        strength = 0.5 if opt == "image" else 1.0
        init = synth.uniform("msg.init", SHAPE, lo=-1.0, hi=1.0)
        mask = torch.zeros(SHAPE[0], 1, *SHAPE[2:])
        mask[..., 4:] = 1.0
        kw = dict(init=init, mask=mask, strength=strength, resample=2)
        gen = dict(init_image=init.to(DEV), mask=mask.to(DEV), strength=strength, resample=2)
        k = ic.strength_steps(STEPS, strength)
        n_calls = ic.n_model_calls(STEPS, strength, 2, False)
    want_orders: list[int] = []
    r64 = restate(sampler, mean_type, y, noises, torch.float64, want_orders, **kw)
    r32 = restate(sampler, mean_type, y, noises, torch.float32, **kw)
    # (the three steps that strength 0.5 leaves of a six-step chain start at t == 2, a first step, and go on to t == 1 and t == 0:
    # every launch of that case is first order by the rule)
    assert r32["x"].dtype == torch.float32 and want_orders[0] == 1 and (2 in want_orders) == ((sampler, opt) != ("dpmpp_2m", "image"))
    want_xt, want_x0 = torch.stack(r64["xt"], dim=1), torch.stack(r64["x0"], dim=1)
    dist = max(float((torch.stack(r32["xt"], dim=1).double() - want_xt).abs().max()),
               float((torch.stack(r32["x0"], dim=1).double() - want_x0).abs().max()), float((r32["x"].double() - r64["x"]).abs().max()))
    assert dist > 0.0

    orders: list[int] = []
    real = ops._call

    def spy(name, *args):
        if name == "dl_ab2_step":
            orders.append(1 if args[5] is None else 2)
        elif name == "dl_dpmpp_2m_step":
            orders.append(1 if args[6] is None else 2)
        else:
            assert name not in ("dl_euler_step", "dl_euler_step_g", "dl_ddim_step", "dl_ddim_step_g", "dl_ddim_step_v"), name
        return real(name, *args)

    monkeypatch.setattr(ops, "_call", spy)
    d, model = make(sampler, mean_type)
    hand_out(monkeypatch, noises)
    out = d.generate({"y": y.to(DEV)}, data_shape=SHAPE, use_tqdm=False, return_intermediates=True, **gen)
    assert orders == want_orders and model.calls == n_calls
    assert out["xt"].shape == (SHAPE[0], k + 1) + SHAPE[1:] and out["estimated_x0"].shape == (SHAPE[0], k) + SHAPE[1:]
    got = max(float((out["xt"].double().cpu() - want_xt).abs().max()), float((out["estimated_x0"].double().cpu() - want_x0).abs().max()),
              float((out["x"].double().cpu() - r64["x"]).abs().max()))
    print(f"\n{sampler} {mean_type} {opt}: orders {orders}  max|x| {float(want_xt.abs().max()):.3e}  f32 restatement vs f64 {dist:.3e}  "
          f"product vs f64 {got:.3e}  tolerance {4 * dist:.3e}")
    assert got <= 4 * dist, (got, dist)
    assert "xt_std" not in out and "logprob" not in out and ("xt_mean" in out) == (sampler == "dpmpp_2m")
    if sampler == "dpmpp_2m":  # xt_mean is x_prev as the step made it, before the in-place blend of the known region
        want_mean = torch.stack(r64["mean"], dim=1)
        got_mean = float((out["xt_mean"].double().cpu() - want_mean).abs().max())
        assert got_mean <= 4 * dist, (got_mean, dist)
        assert torch.equal(bits(out["xt_mean"][:, -1]), bits(out["estimated_x0"][:, -1]))  # t == 0 returns its x0
    if opt.startswith("image"):
        keep = (kw["mask"] <= 0).expand(SHAPE)
        assert torch.equal(bits(out["x"].cpu()[keep]), bits(kw["init"][keep]))
        if sampler == "dpmpp_2m":
            assert not torch.equal(out["xt_mean"][:, -1].cpu()[keep], kw["init"][keep])
    elif sampler == "dpmpp_2m":
        assert torch.equal(bits(out["xt_mean"]), bits(out["xt"][:, 1:]))


def test_worst_ratios_of_the_kernel_tests():
    """runs after the kernel tests (module order): the worst |diff| / bound of every output"""
    print("\nworst |diff| / bound: " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------------------------ end to end
def _unet():  # the smallest shapes the engines accept, as tests/test_guidance_gpu.py sizes them
    from diffulab_amd.networks.denoisers import UNetModel

    return UNetModel(image_size=[16, 16], in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=[2],
                     channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True, n_classes=10,
                     classifier_free=True)


def _dit():
    from diffulab_amd import MMDiT

    return MMDiT(simple_dit=True, input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4,
                 patch_size=2, depth=2, n_classes=10, classifier_free=True)


def test_end_to_end_dit_ab2_with_cfg():
    from diffulab_amd import Diffuser

    torch.manual_seed(0)
    m = _dit()
    with torch.no_grad():  # the output head starts at zero
        dict(m.named_parameters())["last_layer.linear.weight"].normal_(std=0.02)
    m = m.to(DEV).eval()
    assert m.precision == "bf16"
    d = Diffuser(m, sampling_method="ab2", model_type="rectified_flow", n_steps=4)
    y = synth.integers("mse.y", (4,), 10).to(DEV)
    noise = synth.normal("mse.dit", (4, 4, 16, 16)).to(DEV)
    outs = [d.generate({"x": noise.clone(), "y": y}, use_tqdm=False, guidance_scale=5)["x"] for _ in range(2)]
    assert outs[0].shape == (4, 4, 16, 16) and bool(torch.isfinite(outs[0]).all()) and torch.equal(bits(outs[0]), bits(outs[1]))
    euler = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=4)
    assert not torch.equal(euler.generate({"x": noise.clone(), "y": y}, use_tqdm=False, guidance_scale=5)["x"], outs[0])


def test_end_to_end_unet_dpmpp_2m_v_with_dynamic_threshold():
    from diffulab_amd import Diffuser

    torch.manual_seed(0)
    m = _unet()
    with torch.no_grad():
        dict(m.named_parameters())["out.2.weight"].normal_(std=0.2)
    m = m.to(DEV).eval()
    assert m.precision == "bf16"
    d = Diffuser(m, sampling_method="dpmpp_2m", model_type="gaussian_diffusion", n_steps=4,
                 extra_args={"schedule": "cosine", "sampler_parameters": {"mean_type": "v"}, "loss_target": "mean_type"})
    y = synth.integers("mse.y", (4,), 10).to(DEV)
    noise = synth.normal("mse.unet", (4, 1, 16, 16)).to(DEV)
    outs = [d.generate({"x": noise.clone(), "y": y}, use_tqdm=False, dynamic_threshold=0.995, threshold_max=4.0, return_intermediates=True)
            for _ in range(2)]
    x = outs[0]["x"]
    assert x.shape == (4, 1, 16, 16) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(outs[0]["xt"]).all())
    assert outs[0]["estimated_x0"].shape == (4, 4, 1, 16, 16) and float(outs[0]["estimated_x0"].abs().max()) <= 1.0
    assert all(torch.equal(bits(outs[0][k_]), bits(outs[1][k_])) for k_ in outs[0])
    assert torch.equal(bits(x), bits(outs[0]["estimated_x0"][:, -1]))  # the step at t == 0 returns its x0


def test_the_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "fast_sampling.py"), "--train-steps", "4", "--euler-steps", "8",
                        "--ab2-steps", "4", "--ref-steps", "16", "--chain", "8", "--dpmpp-steps", "4"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ab2 4 steps" in r.stdout and "dpmpp_2m 4 steps" in r.stdout
