"""GPU tests of the bits-per-dimension evaluation: the per-row kernels (dl_vb_terms, dl_prior_bpd), `GaussianDiffusion.calc_bpd_loop`
/ `Diffuser.evaluate_bpd` over them, and the trainer's `val_bpd_batches`.

Expected values: the f64 evaluation of tests/bpd_common.py on the same f32 inputs (for the loop: on the x_t and the predictions the
denoiser saw, captured with a forward hook), and closed forms where there are any.

Tolerance, the suite's rule for f32 element-wise kernels (tests/test_learned_variance_gpu.py): the kernel and the f32 CPU evaluation of
the restatement are both f32 evaluations of the same formulas on the same inputs, so the f32 CPU evaluation's own error against f64 is
measured per case and, per output array, every row is allowed 2 * max|f32 CPU - f64| + 3e-6 * max|f64|.  Every figure is printed
before it is asserted.  Measured figures: DESIGN.md section 2.

Chains: "8 steps" and "20 steps" are the 1000-step linear schedule respaced (`set_steps`), which is how this project makes a short
chain; the linear formula itself has betas above 1 at 8 steps.
"""

import ctypes
import json
import math
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

import bpd_common as bc  # noqa: E402
import elementwise_bounds as eb  # noqa: E402
import learned_variance_common as lv  # noqa: E402
from oracle import diffusion as od  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
CHWS = (105, 256, 4100)  # 3 * 5 * 7: no multiple of 4 or 64; one full block; one past a 4096-element share (second reduction stage)
LN2 = math.log(2.0)


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as _ops

    return _ops


@lru_cache(maxsize=None)
def reference(chain: str, chw: int, mean_type: str, var_type: str, clip: bool):
    """(inputs, f64 rows, f32 CPU rows) of one case: computed once, shared, never modified"""
    T, t = bc.chain(chain)
    c = bc.case(T, t, chw, mean_type, var_type, tag=chain)
    args = (c["tab"], c["lv_q"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], mean_type, var_type, clip)
    return c, bc.terms(*args, torch.float64), bc.terms(*args, torch.float32)


def var_mode(ops, var_type: str) -> int:
    return ops.VAR_MODES.get(var_type, ops.VAR_FIXED)


def run(ops, c, mean_type: str, var_type: str, clip: bool, out=None):
    d = {k: c[k].to(DEV) for k in ("pred", "eps", "x0", "xt", "t", "tab", "lv_q")}
    return ops.vb_terms(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], d["lv_q"], ops.MEAN_TYPES[mean_type],
                        var_mode(ops, var_type), clip, out=out)


def check_inputs(c, ref):
    """the conditions the comparison rests on, on the reference values: no t == 0 probability near the 1e-12 clamp, nothing but the
    elements at exactly +-1 near the bin thresholds, and both open bins met in the t == 0 rows"""
    x0 = c["x0"]
    assert float(ref["prob"][ref["first"]].min()) > 10 * 1e-12
    assert bool(((x0.abs() - 0.999).abs() > 1e-3)[x0.abs() != 1.0].all())
    first = x0[c["t"] == 0]
    assert int((first.abs() == 1.0).sum()) >= 6 and bool((first == 1.0).any()) and bool((first == -1.0).any())


def check_rows(what: str, got, ref, cpu32):
    for k, g in zip(bc.KEYS, got):
        err, e32, bound = bc.bound(g, ref[k], cpu32[k])
        print(f"{what} {k}: max|ref| {float(ref[k].abs().max()):.6g}  f32-cpu max err {e32:.3e}  kernel max err {err:.3e}  bound {bound:.3e}")
        assert bool(torch.isfinite(g).all()) and err <= bound, (what, k, err, bound)


# ------------------------------------------------------------------------------------------------------------------ kernel against f64
@pytest.mark.parametrize("var_type", bc.VAR_TYPES)
@pytest.mark.parametrize("mean_type", bc.MEAN_TYPES)
def test_vb_terms_against_f64(ops, mean_type, var_type):
    for chw in CHWS:
        for clip in (False, True):
            c, ref, cpu32 = reference("t8", chw, mean_type, var_type, clip)
            check_inputs(c, ref)
            got = run(ops, c, mean_type, var_type, clip)
            assert all(g.shape == (bc.ROWS,) and g.dtype == torch.float32 for g in got)
            check_rows(f"t8 {mean_type}/{var_type} chw {chw} clip {int(clip)}", got, ref, cpu32)


@pytest.mark.parametrize("mean_type,var_type", [("epsilon", "learned_range"), ("v", "fixed_large"), ("xprev", "fixed_small"),
                                                ("xstart", "learned")])
def test_vb_terms_on_the_respaced_20_step_chain(ops, mean_type, var_type):
    c, ref, cpu32 = reference("r20", 256, mean_type, var_type, True)
    assert c["tab"].shape == (6, 20)
    check_inputs(c, ref)
    check_rows(f"r20 {mean_type}/{var_type}", run(ops, c, mean_type, var_type, True), ref, cpu32)


# ------------------------------------------------------------------------------------------------------------------ existing kernels
@pytest.mark.parametrize("var_type", lv.VAR_TYPES)
@pytest.mark.parametrize("mean_type", bc.MEAN_TYPES)
def test_mean_of_vb_is_the_training_kernels_bound(ops, mean_type, var_type):
    """learned variances, no clamp: dl_gd_loss_fwd's loss[1] is the batch mean of the same term"""
    for chw in (256, 4100):
        c, ref, cpu32 = reference("t8", chw, mean_type, var_type, False)
        vb = run(ops, c, mean_type, var_type, False)[0]
        d = {k: c[k].to(DEV) for k in ("pred", "eps", "x0", "xt", "t", "tab")}
        both = ops.gd_loss_fwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], ops.MEAN_TYPES[mean_type], None,
                               ops.VAR_MODES[var_type])
        _, e32, bound = bc.bound(vb, ref["vb"], cpu32["vb"])
        diff = abs(float(vb.double().mean()) - float(both[1]))
        print(f"{mean_type}/{var_type} chw {chw}: mean vb {float(vb.double().mean()):.9g}  dl_gd_loss_fwd {float(both[1]):.9g}  "
              f"|diff| {diff:.3e}  bound {bound:.3e}")
        assert diff <= bound


@pytest.mark.parametrize("var_type", ["fixed_small", "fixed_large"])
def test_mean_of_mse_is_the_plain_mse_head(ops, var_type):
    """DL_VAR_FIXED, epsilon, no clamp: the eps derived from the x0 derived from the prediction is the prediction"""
    for chw in CHWS:
        c, ref, cpu32 = reference("t8", chw, "epsilon", var_type, False)
        mse = run(ops, c, "epsilon", var_type, False)[2]
        plain = ops.mse_loss_fwd(c["pred"].to(DEV), c["eps"].to(DEV), None, ops.LOSS_EPS)
        _, e32, bound = bc.bound(mse, ref["mse"], cpu32["mse"])
        diff = abs(float(mse.double().mean()) - float(plain))
        print(f"{var_type} chw {chw}: mean mse {float(mse.double().mean()):.9g}  dl_mse_loss_fwd {float(plain):.9g}  |diff| {diff:.3e}  "
              f"bound {bound:.3e}")
        assert diff <= bound


# ------------------------------------------------------------------------------------------------------------------ bits, footprint
@pytest.mark.parametrize("var_type", ["fixed_large", "learned_range"])
def test_two_runs_are_bit_identical_and_exactly_r_floats_are_written(ops, var_type):
    for chw in CHWS:
        c, _, _ = reference("t8", chw, "v", var_type, True)
        a = run(ops, c, "v", var_type, True)
        w = [eb.Guarded(1, bc.ROWS, torch.float32, DEV) for _ in range(3)]
        run(ops, c, "v", var_type, True, out=tuple(g.win[0] for g in w))
        for g, k, first in zip(w, bc.KEYS, a):
            g.check(f"dl_vb_terms {var_type} chw {chw}: {k}")
            assert int((~eb.is_poison(g.buf)).sum()) == bc.ROWS
            assert torch.equal(g.win[0].view(torch.int32), first.view(torch.int32)), (chw, k)
        x0 = c["x0"].to(DEV)
        p = ops.prior_bpd(x0, 0.25, math.log(0.75))
        g = eb.Guarded(1, bc.ROWS, torch.float32, DEV)
        ops.prior_bpd(x0, 0.25, math.log(0.75), out=g.win[0])
        g.check(f"dl_prior_bpd chw {chw}")
        assert int((~eb.is_poison(g.buf)).sum()) == bc.ROWS and torch.equal(g.win[0].view(torch.int32), p.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ prior
@pytest.mark.parametrize("chain", ["t8", "mid"])
def test_prior_bpd_against_f64_and_the_closed_form(ops, chain):
    """ "t8": alphas_bar[T-1] of the linear chain (4e-5: the three constant terms cancel to 8e-10); "mid": a chain that ends at 0.25"""
    ab = float(bc.chain("t8")[0].alphas_bar[-1]) if chain == "t8" else 0.25
    l = math.log(1.0 - ab)
    ab32, l32 = bc.f32(ab), bc.f32(l)
    for chw in CHWS:
        x0 = reference("t8", chw, "epsilon", "fixed_small", False)[0]["x0"]
        got = ops.prior_bpd(x0.to(DEV), ab, l)
        ref, cpu32 = bc.prior(x0, ab32, l32, torch.float64), bc.prior(x0, ab32, l32, torch.float32)
        err, e32, bound = bc.bound(got, ref, cpu32)
        print(f"prior {chain} chw {chw}: max|ref| {float(ref.max()):.6g}  f32-cpu max err {e32:.3e}  kernel max err {err:.3e}  bound {bound:.3e}")
        assert got.shape == (bc.ROWS,) and err <= bound
        for cst in (0.0, 1.0, -0.37):
            xc = torch.full((bc.ROWS, chw), cst)
            c32 = float(xc[0, 0])
            want = torch.full((bc.ROWS,), 0.5 * (-1.0 - l + (1.0 - ab) + ab * c32 * c32) / LN2, dtype=torch.float64)
            got = ops.prior_bpd(xc.to(DEV), ab, l)
            err, e32, bound = bc.bound(got, want, bc.prior(xc, ab32, l32, torch.float32))
            print(f"prior {chain} chw {chw} constant {cst}: closed form {float(want[0]):.6e}  f32-cpu err {e32:.3e}  kernel err {err:.3e}  "
                  f"bound {bound:.3e}")
            assert err <= bound


# ------------------------------------------------------------------------------------------------------------------ argument errors
def test_bad_arguments_return_invalid_and_launch_nothing(ops):
    from diffulab_amd import _lib

    cd = _lib.lib().cdll
    c, _, _ = reference("t8", 105, "epsilon", "fixed_small", False)
    d = {k: c[k].to(DEV) for k in ("pred", "eps", "x0", "xt", "t", "tab", "lv_q")}
    outs = [eb.poison_(torch.empty(bc.ROWS, device=DEV)) for _ in range(3)]
    i64, F = ctypes.c_int64, ctypes.c_float
    P = {k: ctypes.c_void_p(v.data_ptr()) for k, v in d.items()}
    O = [ctypes.c_void_p(o.data_ptr()) for o in outs]

    def vb(R=bc.ROWS, chw=105, mt=0, vm=-1, T=8, **null):
        a = {k: (None if k in null else v) for k, v in P.items()}
        o = [None if f"o{i}" in null else p for i, p in enumerate(O)]
        rc = cd.dl_vb_terms(a["pred"], a["eps"], a["x0"], a["xt"], a["t"], a["tab"], T, a["lv_q"], mt, vm, 1, None, o[0], o[1], o[2],
                            i64(R), i64(chw), None)
        assert rc == -1 and "dl_vb_terms" in cd.dl_last_error().decode(), (rc, cd.dl_last_error().decode())

    for k in list(P) + ["o0", "o1", "o2"]:
        vb(**{k: True})
    vb(R=0)
    vb(chw=0)
    vb(T=0)
    vb(mt=4)
    vb(vm=2)
    vb(chw=4097)  # two shares per row and no scratch
    for args in ((None, F(0.5), F(-0.7), None, O[0], i64(bc.ROWS), i64(105)), (P["x0"], F(0.5), F(-0.7), None, None, i64(bc.ROWS), i64(105)),
                 (P["x0"], F(0.5), F(-0.7), None, O[0], i64(0), i64(105)), (P["x0"], F(0.5), F(-0.7), None, O[0], i64(bc.ROWS), i64(0)),
                 (P["x0"], F(1.5), F(-0.7), None, O[0], i64(bc.ROWS), i64(105)), (P["x0"], F(0.5), F(0.7), None, O[0], i64(bc.ROWS), i64(105))):
        assert cd.dl_prior_bpd(*args, None) == -1 and "dl_prior_bpd" in cd.dl_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(eb.is_poison(o).all()) for o in outs)


# ------------------------------------------------------------------------------------------------------------------ the loop
B, SHAPE = 2, (2, 3, 8, 8)


def diffusion(var_type: str, mean_type: str = "epsilon", steps: int = 8):
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion

    gd = GaussianDiffusion(n_steps=1000, sampler_parameters={"var_type": var_type, "mean_type": mean_type})
    gd.set_steps(steps)
    return gd


class TrueEps(torch.nn.Module):
    """returns the noise x_t was made with: row k B + b of a pass is sample b at the chain index its (remapped) timestep stands for.
    Row-independent, so the chunking cannot change a bit.  Keeps what it was given, for the restatement."""

    def __init__(self, noise, timestep_map):
        super().__init__()
        self.noise, self.map, self.seen = noise, torch.tensor(timestep_map, device=DEV), []

    def forward(self, x, timesteps, p=0, **kw):
        assert p == 0 and not kw
        j = torch.searchsorted(self.map, timesteps.to(self.map.dtype))
        b = torch.arange(x.shape[0], device=x.device) % self.noise.shape[0]
        out = self.noise[b, j].contiguous()
        self.seen.append((x.clone(), j.clone(), out.clone()))
        return {"x": out}


def restate(gd, seen, x0, noise, var_type, mean_type, clip, n_t):
    """the loop's arrays from what the denoiser saw: (f64, f32 CPU) dicts of [B, n_t] arrays, columns in ascending index order"""
    T = od.GaussianTables(1000, n_steps=gd.steps)
    tab, lv_q = bc.tables(T, var_type)
    assert torch.equal(tab, gd.sampler._tables(torch.device("cpu"))), "the restatement and the sampler read the same table"
    xt = torch.cat([s[0] for s in seen]).cpu()
    j = torch.cat([s[1] for s in seen]).cpu()
    pred = torch.cat([s[2] for s in seen]).float().cpu()
    nb = x0.shape[0]
    b = torch.arange(xt.shape[0]) % nb
    x0r, eps = x0.cpu()[b], noise.cpu()[b, j]
    out = []
    for dtype in (torch.float64, torch.float32):
        r = bc.terms(tab, lv_q, pred, eps, x0r, xt, j.to(torch.int32), mean_type, var_type, clip, dtype)
        cols = {}
        for k in bc.KEYS:
            a = torch.empty(nb, gd.steps, dtype=dtype)
            a[b, j] = r[k]
            cols[k] = a[:, sorted(set(j.tolist()))]
            assert cols[k].shape == (nb, n_t)
        cols["prob"], cols["first"] = r["prob"], r["first"]
        out.append(cols)
    return out


def check_loop(what, out, ref, cpu32, keys=bc.KEYS):
    for k in keys:
        err, e32, bound = bc.bound(out[k], ref[k], cpu32[k])
        print(f"{what} {k}: max|ref| {float(ref[k].abs().max()):.6g}  f32-cpu max err {e32:.3e}  loop max err {err:.3e}  bound {bound:.3e}")
        assert out[k].dtype == torch.float32 and err <= bound, (what, k, err, bound)


@pytest.mark.parametrize("var_type", ["fixed_small", "fixed_large"])
def test_loop_with_a_true_eps_denoiser(var_type):
    gd = diffusion(var_type)
    x0 = synth.uniform("bpdl.x0", SHAPE, lo=-1.0, hi=1.0).to(DEV)
    noise = synth.normal("bpdl.noise", (B, 8) + SHAPE[1:]).to(DEV)
    outs = {}
    for k in (1, 3, 8):
        m = TrueEps(noise, gd.timestep_map)
        outs[k] = gd.calc_bpd_loop(m, {"x": x0}, clip_denoised=False, t_chunk=k, noise=noise)
        assert len(m.seen) == -(-8 // k) and m.seen[0][0].shape[0] == k * B
    out = outs[3]
    assert set(out) == {"vb", "xstart_mse", "mse", "prior_bpd", "total_bpd"}
    assert all(out[k].shape == (B, 8) for k in bc.KEYS) and out["prior_bpd"].shape == (B,) and out["total_bpd"].shape == (B,)
    for k in (1, 8):  # row-independent stub: the chunking changes no bit
        for key in out:
            assert torch.equal(out[key].view(torch.int32), outs[k][key].view(torch.int32)), (k, key)
    assert torch.equal(out["total_bpd"], out["prior_bpd"] + out["vb"].sum(1))
    ref, cpu32 = restate(gd, m.seen, x0, noise, var_type, "epsilon", False, 8)
    # (the two squared errors of an exact prediction are rounding noise around zero: printed by the restatement's side only)
    check_loop(f"true eps {var_type}", out, ref, cpu32, keys=("vb",))
    print(f"true eps {var_type}: max xstart_mse {float(out['xstart_mse'].max()):.3e}  max mse {float(out['mse'].max()):.3e}")
    _, _, tol = bc.bound(out["vb"], ref["vb"], cpu32["vb"])
    T = od.GaussianTables(1000, n_steps=8)
    if var_type == "fixed_small":  # the posterior itself: no KL left
        print(f"fixed_small max|vb[:, 1:]| {float(out['vb'][:, 1:].abs().max()):.3e}  tolerance {tol:.3e}")
        assert float(out["vb"][:, 1:].abs().max()) <= tol
    else:
        v = torch.cat([T.posterior_variance[1:2], T.betas[1:]])
        pv = torch.cat([T.posterior_variance[1:2], T.posterior_variance[1:]])
        want = (0.5 * (-1.0 + torch.log(v / pv) + pv / v) / LN2)[1:]
        err = float((out["vb"][:, 1:].double().cpu() - want).abs().max())
        print(f"fixed_large closed form {want.tolist()}  max err {err:.3e}  tolerance {tol:.3e}")
        assert err <= tol
    assert float(out["mse"].max()) < 1e-6 and float(out["xstart_mse"].max()) < 1e-6
    # a subset of the chain: its columns, and no total
    sub = gd.calc_bpd_loop(TrueEps(noise, gd.timestep_map), {"x": x0}, clip_denoised=False, noise=noise, timesteps=[0, 5])
    assert set(sub) == {"vb", "xstart_mse", "mse", "prior_bpd"} and sub["vb"].shape == (B, 2)
    for key in bc.KEYS:
        assert torch.equal(sub[key].view(torch.int32), out[key][:, [0, 5]].contiguous().view(torch.int32)), key
    ab = float(T.alphas_bar[-1])
    ab32, l32 = bc.f32(ab), bc.f32(math.log(1.0 - ab))
    err, e32, bound = bc.bound(out["prior_bpd"], bc.prior(x0.cpu(), ab32, l32), bc.prior(x0.cpu(), ab32, l32, torch.float32))
    assert err <= bound


def _dit(output_channels):
    from diffulab_amd import MMDiT

    torch.manual_seed(0)
    m = MMDiT(simple_dit=True, input_channels=4, output_channels=output_channels, inner_dim=128, embedding_dim=64, num_heads=2,
              mlp_ratio=4, patch_size=2, depth=2, n_classes=10, classifier_free=True)  # 16 x 16 / 2 x 2: 64 tokens per sample
    with torch.no_grad():  # the output head starts at zero
        dict(m.named_parameters())["last_layer.linear.weight"].normal_(std=0.02)
    return m.to(DEV).eval()


@pytest.mark.parametrize("var_type,mean_type,steps,t_chunk", [("fixed_small", "epsilon", 8, 3), ("learned_range", "v", 20, None),
                                                              ("fixed_large", "v", 8, None)])
def test_loop_with_a_tiny_dit(var_type, mean_type, steps, t_chunk):
    from diffulab_amd import Diffuser

    C = 4
    m = _dit(2 * C if var_type in lv.VAR_TYPES else C)
    d = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000,
                 extra_args={"sampler_parameters": {"var_type": var_type, "mean_type": mean_type},
                             "loss_target": "mean_type" if mean_type == "v" else "epsilon"})
    d.set_steps(steps)
    gd = d.diffusion
    x0 = synth.uniform("bpdl.dit.x0", (B, C, 16, 16), lo=-1.0, hi=1.0).to(DEV)
    keep = x0.clone()
    y = synth.integers("bpdl.dit.y", (B,), 10).to(DEV)
    noise = synth.normal("bpdl.dit.noise", (B, steps, C, 16, 16)).to(DEV)
    tmap = torch.tensor(gd.timestep_map, device=DEV)
    seen = []

    def hook(mod, args, kwargs, out):
        assert kwargs["p"] == 0 and kwargs["y"].shape[0] == kwargs["x"].shape[0] and torch.equal(kwargs["y"][:B], y)
        seen.append((kwargs["x"].clone(), torch.searchsorted(tmap, kwargs["timesteps"].to(tmap.dtype)), out["x"].clone()))

    h = m.register_forward_hook(hook, with_kwargs=True)
    try:
        inputs = {"x": x0, "y": y}
        out = d.evaluate_bpd(inputs, noise=noise, t_chunk=t_chunk)
    finally:
        h.remove()
    assert list(inputs) == ["x", "y"] and inputs["x"] is x0 and torch.equal(x0, keep)  # not mutated, unlike compute_loss
    assert len(seen) == (-(-steps // t_chunk) if t_chunk else 1)
    ref, cpu32 = restate(gd, seen, x0, noise, var_type, mean_type, True, steps)
    assert float(ref["prob"][ref["first"]].min()) > 10 * 1e-12
    check_loop(f"tiny DiT {mean_type}/{var_type} T {steps}", out, ref, cpu32)
    assert torch.equal(out["total_bpd"], out["vb"].sum(1) + out["prior_bpd"]) and bool(torch.isfinite(out["total_bpd"]).all())


# ------------------------------------------------------------------------------------------------------------------ trainer
def test_trainer_logs_bpd_outside_the_checkpoint_criterion(tmp_path):
    from torch.utils.data import DataLoader

    from diffulab_amd import Diffuser, MMDiT
    from diffulab_amd.datasets import SyntheticDataset
    from diffulab_amd.training import BaseTrainer, FusedAdamW

    def go(name, **kw):
        torch.manual_seed(0)
        m = MMDiT(simple_dit=True, input_channels=4, output_channels=8, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4,
                  patch_size=2, depth=2, n_classes=10, classifier_free=True)
        d = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000,
                     extra_args={"sampler_parameters": {"var_type": "learned_range"}})
        d.set_steps(20)
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
        mk = lambda n, seed: DataLoader(SyntheticDataset(n, (4, 16, 16), 10, seed), batch_size=16, drop_last=True)  # noqa: E731
        tr = BaseTrainer(n_epoch=1, save_path=tmp_path, project_name=name, use_ema=True, ema_update_after_step=0, ema_update_every=1)
        tr.train(diffuser=d, optimizer=opt, train_dataloader=mk(32, 1), val_dataloader=mk(32, 2), log_validation_images=False,
                 p_classifier_free_guidance=0.1, **kw)
        rows = [json.loads(ln) for ln in (tmp_path / name / "metrics.jsonl").read_text().splitlines()]
        val = {k: v for r in rows for k, v in r.items() if k.startswith("val/")}
        return tr, val

    tr, val = go("with", val_bpd_batches=1)
    print(val)
    assert {"val/loss", "val/vb", "val/bpd", "val/prior_bpd"} <= set(val)
    assert all(math.isfinite(val[k]) for k in ("val/bpd", "val/prior_bpd")) and val["val/bpd"] > val["val/prior_bpd"] > 0
    crit = sum(v for k, v in val.items() if k not in ("val/bpd", "val/prior_bpd"))
    assert abs(tr.val_total - crit) <= 1e-9 * abs(crit)
    tr0, val0 = go("without")
    assert "val/bpd" not in val0 and "val/prior_bpd" not in val0 and {"val/loss", "val/vb"} <= set(val0)
    assert abs(tr0.val_total - sum(val0.values())) <= 1e-9 * abs(sum(val0.values()))


# ------------------------------------------------------------------------------------------------------------------ example
def test_the_example_runs():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(root, "examples", "evaluate_bpd.py"), "--train-steps", "4", "--chain", "20",
                        "--batch", "4"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("bits/dim") == 2 and "quartile 3 (t in [15, 20))" in r.stdout and "4 samples, 20 timesteps" in r.stdout
