"""CPU checks of the bits-per-dimension evaluation: the fp64 restatement of tests/bpd_common.py against closed forms that do not go
through it, the equality of the four parameterisations, the chunk planner of `calc_bpd_loop`, every argument error (raised before any
device work, so with no device present) and the two new C entry points' declarations and bindings."""

import ast
import ctypes
import math
import os

import pytest
import torch

import bpd_common as bc
import gd_param_common as gp
import learned_variance_common as lv
from oracle import diffusion as od
from oracle import synth

LN2 = math.log(2.0)
F64 = torch.float64


def exact_case(T, shape=(8, 2, 4, 4)):
    """fp64 inputs on the fp64 schedule: one row per index of the chain, x_t formed without rounding to f32"""
    n = T.betas.numel()
    t = torch.arange(n, dtype=torch.int32)
    x0 = synth.uniform("bpdh.x0", shape, lo=-1.0, hi=1.0).double()
    eps = synth.normal("bpdh.eps", shape).double()
    sab = T.sqrt_alphas_bar.view(-1, 1, 1, 1)
    xt = sab * x0 + (1.0 - T.alphas_bar).sqrt().view(-1, 1, 1, 1) * eps
    return t, x0, eps, xt


# ------------------------------------------------------------------------------------------------------------------ closed forms
def test_true_eps_with_fixed_small_has_no_kl_and_no_error():
    T = bc.chain("t8")[0]
    t, x0, eps, xt = exact_case(T)
    tab, lv_q = bc.tables(T, "fixed_small", F64)
    for clip in (False, True):  # the exact x0 lies inside [-1, 1] up to round-off: the clamp moves it by no more than that
        r = bc.terms(tab, lv_q, eps, eps, x0, xt, t, "epsilon", "fixed_small", clip, F64)
        assert r["vb"].shape == (8,) and float(r["vb"][1:].abs().max()) < 1e-14, r["vb"]  # (fp64 round-off of -1 + lv_p - lv_q + 1)
        assert float(r["mse"].abs().max()) < 1e-18 and float(r["xstart_mse"].abs().max()) < 1e-18
        assert float(r["vb"][0]) > 0  # the t == 0 term is a negative log-probability of a bin


def test_true_eps_with_fixed_large_is_the_variance_mismatch_alone():
    T = bc.chain("t8")[0]
    t, x0, eps, xt = exact_case(T)
    tab, lv_q = bc.tables(T, "fixed_large", F64)
    r = bc.terms(tab, lv_q, eps, eps, x0, xt, t, "epsilon", "fixed_large", False, F64)
    v = torch.cat([T.posterior_variance[1:2], T.betas[1:]])  # the model's variance
    pv = torch.cat([T.posterior_variance[1:2], T.posterior_variance[1:]])  # the posterior's, clipped at its first entry
    want = 0.5 * (-1.0 + torch.log(v / pv) + pv / v) / LN2
    assert torch.allclose(r["vb"][1:], want[1:], rtol=1e-11, atol=1e-15), (r["vb"], want)
    assert float(want[1:].min()) > 0  # (beta_t > the posterior variance for t >= 1)
    assert float(r["mse"].abs().max()) < 1e-18


@pytest.mark.parametrize("c", [0.0, -1.0, 0.37])
def test_prior_of_a_constant_image(c):
    T = od.GaussianTables(1000)
    ab = float(T.alphas_bar[-1])
    l = math.log(1.0 - ab)
    got = bc.prior(torch.full((3, 2, 5, 5), c), ab, l, F64)
    c32 = float(torch.tensor(c, dtype=torch.float32))
    want = 0.5 * (-1.0 - l + (1.0 - ab) + ab * c32 * c32) / LN2
    assert got.shape == (3,) and torch.allclose(got, torch.full((3,), want, dtype=F64), rtol=1e-12, atol=1e-18), (got, want)
    assert want > 0


# ------------------------------------------------------------------------------------------------------------------ parameterisations
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("var_type", ["fixed_small", "learned_range"])
def test_the_four_parameterisations_of_one_prediction_give_the_same_rows(var_type, clip):
    T = bc.chain("t8")[0]
    t, x0, eps, xt = exact_case(T)
    tab, lv_q = bc.tables(T, var_type, F64)
    rows = lv._rows(tab, t, xt, F64)
    eps_hat = eps + 0.1 * synth.normal("bpdh.dev", tuple(eps.shape)).double()
    x0_hat = gp.x_start(eps_hat, xt, rows, "epsilon")
    v = synth.uniform("bpdh.v", tuple(eps.shape), lo=-1.0, hi=1.0).double()
    out = {}
    for mt in bc.MEAN_TYPES:
        o = gp.target(rows, eps_hat, x0_hat, xt, mt)
        pred = torch.cat([o, v], dim=1) if var_type == "learned_range" else o
        out[mt] = bc.terms(tab, lv_q, pred, eps, x0, xt, t, mt, var_type, clip, F64)
    for mt in bc.MEAN_TYPES[1:]:
        for k in bc.KEYS:
            assert torch.allclose(out[mt][k], out["epsilon"][k], rtol=1e-8, atol=1e-14), (mt, k, out[mt][k], out["epsilon"][k])
    assert float(out["epsilon"]["mse"].min()) > 1e-5  # (the prediction is off by 0.1 n: the rows are not trivially zero)


def test_f32_switch_evaluates_in_f32():
    T, t = bc.chain("t8")
    c = bc.case(T, t, 105, "v", "learned_range")
    r = bc.terms(c["tab"], c["lv_q"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], "v", "learned_range", True, torch.float32)
    assert all(r[k].dtype == torch.float32 and r[k].shape == (bc.ROWS,) for k in bc.KEYS)
    assert bc.prior(c["x0"], 0.5, math.log(0.5), torch.float32).dtype == torch.float32


# ------------------------------------------------------------------------------------------------------------------ chunk planner
@pytest.mark.parametrize("t_chunk", [1, 3, 8, 1000, None])
@pytest.mark.parametrize("n", [1, 7, 8, 1000])
def test_chunk_planner_visits_every_index_once_from_high_to_low(n, t_chunk):
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import BPD_ROWS, plan_bpd_chunks

    for batch in (1, 64, 300):
        chunks = plan_bpd_chunks(n, batch, t_chunk)
        flat = [j for c in chunks for j in c]
        assert flat == list(range(n))[::-1]
        k = t_chunk if t_chunk is not None else max(1, BPD_ROWS // batch)
        assert all(len(c) == k for c in chunks[:-1]) and 1 <= len(chunks[-1]) <= k
        if t_chunk is None:
            assert k * batch <= BPD_ROWS or k == 1


def test_chunk_planner_subsets_and_errors():
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import plan_bpd_chunks

    assert plan_bpd_chunks(8, 2, 2, timesteps=[0, 5, 3]) == [[5, 3], [0]]
    assert plan_bpd_chunks(8, 2, None, timesteps=torch.tensor([7, 0])) == [[7, 0]]
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="t_chunk"):
            plan_bpd_chunks(8, 2, bad)
    for bad in ([8], [-1], [1, 1], []):
        with pytest.raises(ValueError, match="timesteps"):
            plan_bpd_chunks(8, 2, None, timesteps=bad)


# ------------------------------------------------------------------------------------------------------------------ argument errors
class _Stub(torch.nn.Module):
    """never run: every call below is refused before the model is"""

    def __init__(self, out_channels=None):
        super().__init__()
        if out_channels is not None:
            self.out_channels = out_channels

    def forward(self, **kw):
        raise AssertionError("the denoiser ran: the argument check came too late")


def test_bad_arguments_raise_before_any_device_work():
    from diffulab_amd import Diffuser
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion

    gd = GaussianDiffusion(n_steps=8)
    x = torch.zeros(2, 3, 8, 8)  # a CPU tensor: any device work would raise a RuntimeError instead
    m = _Stub()
    for kw, name in (({"t_chunk": 0}, "t_chunk"), ({"timesteps": [8]}, "timesteps"), ({"timesteps": [2, 2]}, "timesteps"),
                     ({"noise": torch.zeros(2, 7, 3, 8, 8)}, "noise"), ({"noise": torch.zeros(2, 3, 8, 8)}, "noise")):
        with pytest.raises(ValueError, match=name):
            gd.calc_bpd_loop(m, {"x": x}, **kw)
    with pytest.raises(ValueError, match="latent_diffusion"):
        GaussianDiffusion(n_steps=8, latent_diffusion=True).calc_bpd_loop(m, {"x": x})
    lvd = GaussianDiffusion(n_steps=8, sampler_parameters={"var_type": "learned_range"})
    for ch in (3, 4):  # odd, and even but not 2C
        with pytest.raises(ValueError, match="model"):
            lvd.calc_bpd_loop(_Stub(out_channels=ch), {"x": x})
    d = Diffuser(_Stub(out_channels=3), sampling_method="ddim", model_type="gaussian_diffusion", n_steps=8,
                 extra_args={"sampler_parameters": {"var_type": "learned"}})
    with pytest.raises(ValueError, match="model"):
        d.evaluate_bpd({"x": x})
    with pytest.raises(ValueError, match="t_chunk"):
        d.evaluate_bpd({"x": x}, t_chunk=-3)
    inputs = {"x": x}
    with pytest.raises(ValueError):
        gd.calc_bpd_loop(m, inputs, t_chunk=0)
    assert list(inputs) == ["x"] and inputs["x"] is x


def test_rectified_flow_is_refused_by_name(tmp_path):
    from diffulab_amd import Diffuser
    from diffulab_amd.diffuse.modelizations.flow import NO_VARIATIONAL_BOUND, Flow
    from diffulab_amd.training import BaseTrainer

    assert "rectified flow has no variational bound" in NO_VARIATIONAL_BOUND and "ODE likelihood" in NO_VARIATIONAL_BOUND
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="rectified flow has no variational bound"):
        Flow(n_steps=4).calc_bpd_loop(_Stub(), {"x": x})
    d = Diffuser(_Stub(), sampling_method="euler", model_type="rectified_flow", n_steps=4)
    with pytest.raises(NotImplementedError, match="ODE likelihood"):
        d.evaluate_bpd({"x": x})
    tr = BaseTrainer(n_epoch=1, save_path=tmp_path, project_name="p")
    with pytest.raises(NotImplementedError) as e:
        tr.train(d, None, [], val_dataloader=[], val_bpd_batches=1)
    assert str(e.value) == NO_VARIATIONAL_BOUND
    with pytest.raises(ValueError, match="val_bpd_batches"):
        tr.train(d, None, [], val_bpd_batches=-1)


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_ops_binds_every_argument():
    from diffulab_amd import _lib

    protos = _lib.parse_header()
    assert protos["dl_vb_terms"][2] == ["pred", "eps", "x0", "xt", "t", "tables", "T", "lv_q", "mean_type", "var_mode", "clip_denoised",
                                        "partial", "vb", "xstart_mse", "mse", "rows", "chw", "stream"]
    assert protos["dl_prior_bpd"][2] == ["x0", "alphas_bar_last", "log_one_minus_ab", "partial", "out", "batch", "chw", "stream"]
    assert protos["dl_prior_bpd"][1][1:3] == [ctypes.c_float, ctypes.c_float]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tree = ast.parse(open(os.path.join(root, "diffulab_amd", "ops.py")).read())
    bound = {n.args[0].value: len(n.args) - 1 for n in ast.walk(tree)
             if isinstance(n, ast.Call) and getattr(n.func, "id", "") == "_call" and n.args and isinstance(n.args[0], ast.Constant)}
    for name in ("dl_vb_terms", "dl_prior_bpd"):
        assert bound[name] == len(protos[name][2]), (name, bound[name])


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from diffulab_amd import _lib

    L = _lib.lib()
    c = L.cdll
    assert {"dl_vb_terms", "dl_prior_bpd"} <= set(L.protos)
    buf = ctypes.create_string_buffer(1024)
    P = ctypes.c_void_p(ctypes.addressof(buf))  # a non-null dummy, never dereferenced: the calls below are refused on the host
    i64, F = ctypes.c_int64, ctypes.c_float

    def refused(name, *args):
        assert getattr(c, name)(*args) == -1 and name in c.dl_last_error().decode(), (name, c.dl_last_error().decode())

    def vb(pred=P, eps=P, x0=P, xt=P, t=P, tab=P, T=8, lvq=P, mt=0, vm=-1, partial=None, o1=P, o2=P, o3=P, R=2, chw=64):
        refused("dl_vb_terms", pred, eps, x0, xt, t, tab, T, lvq, mt, vm, 1, partial, o1, o2, o3, i64(R), i64(chw), None)

    for k in ("pred", "eps", "x0", "xt", "t", "tab", "lvq", "o1", "o2", "o3"):
        vb(**{k: None})
    vb(T=0)
    vb(mt=4)
    vb(mt=-1)
    vb(vm=2)
    vb(vm=-2)
    vb(R=0)
    vb(chw=0)
    vb(chw=4097)  # a second share per row needs the scratch
    vb(R=1 << 31, chw=8192, partial=P)  # rows x shares past the grid limit

    def pr(x0=P, ab=0.5, l=-0.7, partial=None, out=P, B=2, chw=64):
        refused("dl_prior_bpd", x0, F(ab), F(l), partial, out, i64(B), i64(chw), None)

    pr(x0=None)
    pr(out=None)
    pr(B=0)
    pr(chw=0)
    pr(ab=0.0)
    pr(ab=1.0)
    pr(l=0.1)
    pr(chw=4097)
