"""GPU tests of guided sampling: the per-sample kernels (dl_cfg_rescale_coef, dl_abs_quantile_rows, dl_x0_threshold), the four `_g`
step kernels, the loops of `Flow.denoise` / `GaussianDiffusion.denoise` against the restatement of tests/guidance_common.py, and
end-to-end runs on the real engines.

Selection: exact.  `lohi` is compared bit for bit with the order statistics of a CPU torch.sort of |x| in f32; q = lo + f (hi - lo) may
sit 3 * 2^-24 * (|lo| + |hi|) + 2^-149 from its f64 value (three roundings, or two with the FMA contracted).

Rescale coefficient: the relative error of r against the f64 restatement may be 4 x that of the f32 restatement on the same inputs,
and never less than 16 * 2^-24 (the floor serves the runs in which the f32 restatement happens to land on the f64 value).

Steps and loops: the rule of tests/test_image_cond_gpu.py.  The product and the f32 evaluation of the restatement are both f32
evaluations of the same formulas on the same inputs; the product may be 4 x as far from the f64 evaluation as the f32 one is.  Per
output of a step kernel the two distances are taken over the three kernel shapes together (a single element can land on its f64
value by chance); per loop over the starting x, every step's x_prev and estimated_x0, and the final sample.  Both figures come from
the restatement, never from the product; the tests print them.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as eb  # noqa: E402
import gd_param_common as gp  # noqa: E402
import guidance_common as gc  # noqa: E402
import learned_variance_common as lv  # noqa: E402
from oracle import diffusion as od  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
U = 2.0**-24
TINY = 2.0**-149
KERNEL_SHAPES = [(1, 1, 1), (2, 3, 35), (3, 4, 257)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as _ops

    return _ops


@pytest.fixture(scope="module")
def T():
    return od.GaussianTables(1000, n_steps=50)


def bits(t):
    return t.contiguous().view(torch.int32)


def clean(t):
    return torch.nan_to_num(t.detach().double().cpu(), 0, 0, 0)  # DDIM's logprob at t == 0: sigma == 0


def var_mode(ops, var_type):
    return ops.VAR_FIXED if var_type == "fixed" else ops.VAR_MODES[var_type]


def step_times(B, late=False):
    """timesteps on the 50-step chain.  The comparisons against f64 stay in its first quarter: further up 1 / sqrt_ab (epsilon) and
    1 / coef1 (xprev) reach 10^2, x0 is some 10^2 wide, only a handful of elements stay inside a threshold of 1 .. 2.5, and a maximum
    over a handful of cancelled values is no statistic to hold a factor of 4 against.  The exact checks (late) use the whole chain."""
    if late:
        return torch.tensor([[25], [0, 49], [0, 25, 49]][B - 1], dtype=torch.int32)
    return torch.tensor([[7], [0, 12], [3, 5, 10]][B - 1], dtype=torch.int32)


# ------------------------------------------------------------------------------------------------------------------ the selection
STAGE = 8192  # SEL_STAGE of csrc/sampler.hip: rows up to here keep their keys in LDS, longer rows recompute them in every pass
SELECT_N = [1, 2, 105, 255, 256, 257, 1028, 4099, STAGE, STAGE + 1]


def select_rows(kind, n):
    """three different rows [3, n] of one kind"""
    if kind == "normal":
        return synth.normal(f"gg.sel.{n}", (3, n))
    if kind == "negative":
        return -synth.normal(f"gg.neg.{n}", (3, n)).abs() - 0.125
    if kind == "equal":
        return torch.tensor([0.75, -0.75, 3.0e-39]).view(3, 1).expand(3, n).contiguous()  # (the third: one denormal value)
    if kind == "three":  # the same multiset in every row, in another order and with other signs: |x| in {0.25, 1.5, 3.0}
        vals = torch.tensor([0.25, 1.5, 3.0])[torch.arange(n) % 3]
        rows = [vals.roll(5 * r)[torch.randperm(n, generator=torch.Generator().manual_seed(r))] for r in range(3)]
        sign = torch.where(synth.normal(f"gg.sgn.{n}", (3, n)) > 0, 1.0, -1.0)
        return (torch.stack(rows) * sign).contiguous()
    assert kind == "wide"  # every radix digit decides somewhere: magnitudes 1e-30 .. 1e30, neighbours in the low mantissa bytes,
    m = n // 3 + 1         # -0.0 / 0.0 and denormals
    mags = 10.0 ** synth.uniform(f"gg.mag.{n}", (3, m), lo=-30.0, hi=30.0).double()
    near = 1.0 + synth.integers(f"gg.near.{n}", (3, m), 70000).double() * 2.0**-23
    spec = torch.tensor([-0.0, 0.0, 1e-40, -3e-45, 1.1754944e-38, -1e-39, 2.0, -2.0], dtype=torch.float64)[torch.arange(3 * m).view(3, m) % 8]
    pool = torch.cat([mags, near, spec], dim=1).float()
    sign = torch.where(synth.normal(f"gg.wsgn.{n}", pool.shape) > 0, 1.0, -1.0)
    pool = pool * sign
    perm = torch.randperm(pool.shape[1], generator=torch.Generator().manual_seed(n))
    return pool[:, perm][:, :n].contiguous()


def positions(kind, n):
    """(k, f) of p = tiny, 0.5, 0.995, 1.0, and for the three-valued rows the positions that straddle the tie boundaries"""
    pos = {gc.quantile_position(p, n) for p in (1e-9, 0.5, 0.995, 1.0)}
    assert any(k == 0 for k, _ in pos) and any(k == n - 1 for k, _ in pos)
    if kind == "three" and n >= 3:
        c0 = (n + 2) // 3          # copies of 0.25
        c1 = c0 + (n + 1) // 3     # ... and of 0.25 or 1.5
        for k in (c0 - 2, c0 - 1, c0, c1 - 1):
            if 0 <= k < n:
                pos.add((k, 0.25))
    return sorted(pos)


@pytest.mark.parametrize("kind", ["normal", "equal", "three", "wide", "negative"])
@pytest.mark.parametrize("n", SELECT_N)
def test_selection_is_exact(ops, kind, n):
    x = select_rows(kind, n)
    assert x.shape == (3, n) and bool(torch.isfinite(x).all())
    dx = x.to(DEV)
    for k, f in positions(kind, n):
        lo, hi = gc.order_stats(x, k, torch.float32)
        q, lohi = ops.abs_quantile_rows(dx, k, f, want_lohi=True)
        q2, lohi2 = ops.abs_quantile_rows(dx, k, f, want_lohi=True)
        got = lohi.cpu()
        assert torch.equal(bits(got[:, 0]), bits(lo)) and torch.equal(bits(got[:, 1]), bits(hi)), (kind, n, k, got, lo, hi)
        want = lo.double() + float(f) * (hi.double() - lo.double())
        bound = 3 * U * (lo.double().abs() + hi.double().abs()) + TINY
        err = (q.double().cpu() - want).abs()
        assert bool((err <= bound).all()), (kind, n, k, f, float((err / bound).max()))
        assert torch.equal(bits(q), bits(q2)) and torch.equal(bits(lohi), bits(lohi2))
        assert torch.equal(bits(ops.abs_quantile_rows(dx, k, f)), bits(q))  # lohi is optional
    if kind == "three" and n >= 3:  # the boundary really is straddled
        c0 = (n + 2) // 3
        lo, hi = gc.order_stats(x, c0 - 1, torch.float32)
        assert bool((lo == 0.25).all()) and bool((hi == (1.5 if n > c0 else 0.25)).all())


def test_selection_writes_inside_its_windows(ops):
    for n in (1, 257, STAGE + 1):
        x = select_rows("normal", n).to(DEV)
        k, f = gc.quantile_position(0.995, n)
        from diffulab_amd.ops import _call, _p, _s

        gq, gl = eb.Guarded(1, 3, torch.float32, DEV), eb.Guarded(1, 6, torch.float32, DEV)
        _call("dl_abs_quantile_rows", _p(x), k, f, _p(gq.win), _p(gl.win), 3, n, _s())
        gq.check(f"dl_abs_quantile_rows n {n}: q")
        gl.check(f"dl_abs_quantile_rows n {n}: lohi")


# ------------------------------------------------------------------------------------------------------------------ the step inputs
def step_case(B, C, hw, var_type, scale=1.0, late=False):
    k = 1 if var_type == "fixed" else 2
    key = f"{B}.{C}.{hw}"
    xt, nz = synth.normal(f"gg.xt.{key}", (B, C, hw)), synth.normal(f"gg.nz.{key}", (B, C, hw))
    pred = (scale * synth.normal(f"gg.pred.{key}.{k}", (B, k * C, hw))).contiguous()
    pu = (scale * synth.normal(f"gg.pu.{key}.{k}", (B, k * C, hw))).contiguous()
    mul = synth.uniform(f"gg.mul.{key}", (B,), lo=0.5, hi=1.0)
    thr = synth.uniform(f"gg.thr.{key}", (B,), lo=1.0, hi=2.5)
    return xt, nz, pred, pu, mul, thr, step_times(B, late)


def gaussian_tables(T, var_type):
    return (gp.fixed_tables(T) if var_type == "fixed" else lv.tables(T)), gp.ddim_tables(T), gc.coefs_of(T)


# ------------------------------------------------------------------------------------------------------------------ dl_x0_threshold
@pytest.mark.parametrize("var_type", ["fixed", "learned_range"])
@pytest.mark.parametrize("mean_type", gc.MEAN_TYPES)
def test_threshold_selects_from_the_x0_the_step_forms(ops, T, mean_type, var_type):
    mt, vm, halves = gc.MEAN_TYPES.index(mean_type), var_mode(ops, var_type), var_type != "fixed"
    for B, C, hw in KERNEL_SHAPES:
        xt, nz, pred, pu, mul, thr, tt = step_case(B, C, hw, var_type, late=True)
        n = C * hw
        tab, tab3, coefs = (v.to(DEV) for v in gaussian_tables(T, var_type))
        d_xt, d_nz, d_pred, d_pu, d_mul, d_t = (v.to(DEV) for v in (xt, nz, pred, pu, mul, tt))
        for sampler in ("ddpm", "ddim"):
            for use_pu, use_mul in ((False, False), (True, False), (True, True), (False, True)):
                a_pu, a_mul, g = (d_pu if use_pu else None), (d_mul if use_mul else None), (3.0 if use_pu else 0.0)
                if sampler == "ddpm":
                    x0 = ops.ddpm_step_g(d_pred, a_pu, g, a_mul, None, d_xt, d_nz, d_t, tab, mt, vm, False)[1]
                    tables, cf = tab, tab[2:4]
                else:
                    x0 = ops.ddim_step_g(d_pred, a_pu, g, a_mul, None, d_xt, d_nz, d_t, tab3, coefs, mt, vm, False, 0.5)[1]
                    tables, cf = tab3, coefs
                assert bool(torch.isfinite(x0).all())
                flat = x0.cpu().view(B, n)
                for p, cap in ((1e-9, None), (0.5, 1.5), (0.995, None), (1.0, 2.0)):
                    k, f = gc.quantile_position(p, n)
                    s, lohi = ops.x0_threshold(d_pred, a_pu, g, a_mul, d_xt, d_t, tables, cf, mt, k, f, cap, halves, want_lohi=True)
                    lo, hi = gc.order_stats(flat, k, torch.float32)
                    got = lohi.cpu()
                    tag = (mean_type, var_type, sampler, (B, C, hw), use_pu, use_mul, p)
                    assert torch.equal(bits(got[:, 0]), bits(lo)) and torch.equal(bits(got[:, 1]), bits(hi)), (tag, got, lo, hi)
                    q = lo.double() + float(f) * (hi.double() - lo.double())
                    want = q.clamp_min(1.0) if cap is None else q.clamp_min(1.0).clamp_max(cap)
                    sc = s.double().cpu()
                    assert bool(((sc - want).abs() <= 3 * U * (lo.double().abs() + hi.double().abs()) + TINY).all()), (tag, sc, want)
                    assert bool((sc >= 1.0).all()) and (cap is None or bool((sc <= cap).all()))
                    assert torch.equal(bits(ops.x0_threshold(d_pred, a_pu, g, a_mul, d_xt, d_t, tables, cf, mt, k, f, cap, halves)), bits(s))


def test_threshold_beyond_the_staged_size(ops, T):
    """a sample longer than the LDS staging recomputes its keys in every pass: the same exact result"""
    B, C, hw = 2, 3, (STAGE // 3) + 7
    xt, nz, pred, pu, mul, thr, tt = step_case(B, C, hw, "fixed", late=True)
    n = C * hw
    assert n > STAGE
    tab = gp.fixed_tables(T).to(DEV)
    d_xt, d_nz, d_pred, d_pu, d_mul, d_t = (v.to(DEV) for v in (xt, nz, pred, pu, mul, tt))
    x0 = ops.ddpm_step_g(d_pred, d_pu, 3.0, d_mul, None, d_xt, d_nz, d_t, tab, 3, ops.VAR_FIXED, False)[1]
    k, f = gc.quantile_position(0.995, n)
    s, lohi = ops.x0_threshold(d_pred, d_pu, 3.0, d_mul, d_xt, d_t, tab, tab[2:4], 3, k, f, None, False, want_lohi=True)
    lo, hi = gc.order_stats(x0.cpu().view(B, n), k, torch.float32)
    assert torch.equal(bits(lohi.cpu()[:, 0]), bits(lo)) and torch.equal(bits(lohi.cpu()[:, 1]), bits(hi))


# ------------------------------------------------------------------------------------------------------------------ dl_cfg_rescale_coef
@pytest.mark.parametrize("g", [1.5, 7.0])
@pytest.mark.parametrize("halves", [False, True])
def test_rescale_coefficient_against_f64(ops, g, halves):
    var_type = "learned" if halves else "fixed"
    for B, C, hw in KERNEL_SHAPES:
        _, _, pred, pu, _, _, _ = step_case(B, C, hw, var_type)
        c, u = pred[:, :C], pu[:, :C]
        d_pred, d_pu = pred.to(DEV), pu.to(DEV)
        for phi in (0.0, 0.7, 1.0):
            r = ops.cfg_rescale_coef(d_pred, d_pu, g, phi, halves)
            assert r.shape == (B,) and torch.equal(bits(r), bits(ops.cfg_rescale_coef(d_pred, d_pu, g, phi, halves)))
            if phi == 0.0 or C * hw == 1:
                assert torch.equal(r.cpu(), torch.ones(B)), (phi, r)
                continue
            want = gc.rescale_coef(c, u, g, phi, torch.float64)
            e32 = float(((gc.rescale_coef(c, u, g, phi, torch.float32).double() - want) / want).abs().max())
            err = float(((r.double().cpu() - want) / want).abs().max())
            tol = max(4 * e32, 16 * U)
            print(f"\ncoef ({B}, {C}, {hw}) halves {halves} g {g} phi {phi}: f32 restatement rel err {e32:.3e}  kernel rel err {err:.3e}  "
                  f"tolerance {tol:.3e}")
            assert err <= tol, (err, tol)
    # a constant combined prediction: S_o == 0
    flat = torch.full((2, 3, 35), 0.75, device=DEV)
    assert torch.equal(ops.cfg_rescale_coef(flat, flat, g, 1.0).cpu(), torch.ones(2))
    gr = eb.Guarded(1, 3, torch.float32, DEV)
    _, _, pred, pu, _, _, _ = step_case(3, 4, 257, var_type)
    ops.cfg_rescale_coef(pred.to(DEV), pu.to(DEV), g, 0.7, halves, out=gr.win.view(3))
    gr.check("dl_cfg_rescale_coef")


# ------------------------------------------------------------------------------------------------------------------ the step kernels
GAUSSIAN_FORMS = [(m, v) for m in gc.MEAN_TYPES for v in gc.VAR_TYPES]


def old_gaussian(ops, sampler, mean_type, var_type, pred, pu, g, xt, nz, t, tab, tab3, coefs, clamp):
    """the entry point a plain call of this form takes today"""
    mt, vm = gc.MEAN_TYPES.index(mean_type), var_mode(ops, var_type)
    if sampler == "ddpm":
        if mean_type == "v":
            return ops.ddpm_step_v(pred, pu, g, xt, nz, t, tab, vm, clamp)
        if var_type == "fixed":
            return ops.ddpm_step(pred, pu, g, xt, nz, t, tab, mt, clamp)
        return ops.ddpm_step_lv(pred, pu, g, xt, nz, t, tab, mt, vm, clamp)
    if mean_type == "v":
        return ops.ddim_step_v(pred, pu, g, xt, nz, t, tab3, vm, clamp, 0.5)
    return ops.ddim_step(pred, pu, g, xt, nz, t, tab3, coefs, mt, clamp, 0.5, halves=var_type != "fixed")


def new_gaussian(ops, sampler, mean_type, var_type, pred, pu, g, mul, thr, xt, nz, t, tab, tab3, coefs, clamp, out=None):
    mt, vm = gc.MEAN_TYPES.index(mean_type), var_mode(ops, var_type)
    if sampler == "ddpm":
        return ops.ddpm_step_g(pred, pu, g, mul, thr, xt, nz, t, tab, mt, vm, clamp, out=out)
    return ops.ddim_step_g(pred, pu, g, mul, thr, xt, nz, t, tab3, coefs, mt, vm, clamp, 0.5, out=out)


def same_bits(a, b, tag):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None), (tag, i)
        if x is not None:  # (nan == nan as bits: DDIM's logprob at t == 0)
            assert torch.equal(bits(x), bits(y)), (tag, i)


@pytest.mark.parametrize("mean_type,var_type", GAUSSIAN_FORMS)
@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_gaussian_g_steps_without_arrays_are_the_old_entry_points(ops, T, sampler, mean_type, var_type):
    for B, C, hw in KERNEL_SHAPES:
        xt, nz, pred, pu, _, _, tt = step_case(B, C, hw, var_type, late=True)
        tab, tab3, coefs = (v.to(DEV) for v in gaussian_tables(T, var_type))
        xt, nz, pred, pu, tt = (v.to(DEV) for v in (xt, nz, pred, pu, tt))
        ones = torch.ones(B, device=DEV)
        for a_pu, g in ((None, 0.0), (pu, 3.0)):
            for clamp in (False, True):
                old = old_gaussian(ops, sampler, mean_type, var_type, pred, a_pu, g, xt, nz, tt, tab, tab3, coefs, clamp)
                tag = (sampler, mean_type, var_type, (B, C, hw), g, clamp)
                same_bits(new_gaussian(ops, sampler, mean_type, var_type, pred, a_pu, g, None, None, xt, nz, tt, tab, tab3, coefs, clamp), old, tag)
                same_bits(new_gaussian(ops, sampler, mean_type, var_type, pred, a_pu, g, ones, None, xt, nz, tt, tab, tab3, coefs, clamp), old, tag)


def test_flow_g_steps_without_arrays_are_the_old_entry_points(ops):
    for B, C, hw in KERNEL_SHAPES:
        xt, nz, pred, pu, _, _, _ = step_case(B, C, hw, "fixed")
        xt, nz, pred, pu = (v.to(DEV) for v in (xt, nz, pred, pu))
        ones = torch.ones(B, device=DEV)
        for a_pu, g in ((None, 0.0), (pu, 3.0)):
            old = ops.euler_step(xt, pred, a_pu, g, 0.75, 0.5)
            same_bits(ops.euler_step_g(xt, pred, a_pu, g, None, 0.75, 0.5), old, "euler")
            same_bits(ops.euler_step_g(xt, pred, a_pu, g, ones, 0.75, 0.5), old, "euler ones")
            old = ops.euler_maruyama_step(xt, pred, a_pu, g, nz, None, 0.75, 0.5, 0.6)
            same_bits(ops.euler_maruyama_step_g(xt, pred, a_pu, g, None, nz, None, 0.75, 0.5, 0.6)[:4], old[:4], "em")
            same_bits(ops.euler_maruyama_step_g(xt, pred, a_pu, g, ones, nz, None, 0.75, 0.5, 0.6)[:4], old[:4], "em ones")
            old = ops.euler_maruyama_step(xt, pred, a_pu, g, None, nz, 0.75, 0.5, 0.6)  # the x_prev_in form
            same_bits(ops.euler_maruyama_step_g(xt, pred, a_pu, g, ones, None, nz, 0.75, 0.5, 0.6)[:4], old[:4], "em x_prev_in")


def four_times_rule(errs, tag):
    """errs: {output key: [(|f32 - f64| max, |product - f64| max) per shape]}"""
    bad = []
    for key, pairs in errs.items():
        dist, got = max(p[0] for p in pairs), max(p[1] for p in pairs)
        print(f"\n{tag} {key}: f32 restatement vs f64 {dist:.3e}  product vs f64 {got:.3e}  tolerance {4 * dist:.3e}")
        if not (dist > 0.0 and got <= 4 * dist):
            bad.append((key, got, dist))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("mean_type,var_type", GAUSSIAN_FORMS)
@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
def test_gaussian_g_steps_with_arrays_against_f64(ops, T, sampler, mean_type, var_type):
    errs: dict = {}
    for B, C, hw in KERNEL_SHAPES:
        xt, nz, pred, pu, mul, thr, tt = step_case(B, C, hw, var_type)
        tab, tab3, coefs = gaussian_tables(T, var_type)
        d = [v.to(DEV) for v in (pred, pu, mul, thr, xt, nz, tt, tab, tab3, coefs)]
        for use_mul, use_thr in ((True, True), (True, False), (False, True)):
            a_mul, a_thr = (mul if use_mul else None), (thr if use_thr else None)
            outs = new_gaussian(ops, sampler, mean_type, var_type, d[0], d[1], 3.0, d[2] if use_mul else None, d[3] if use_thr else None,
                                d[4], d[5], d[6], d[7], d[8], d[9], False)
            ref = {}
            for dtype in (torch.float32, torch.float64):
                if sampler == "ddpm":
                    ref[dtype] = gc.ddpm_step(tab, pred, pu, 3.0, 0.0, None, None, tt, xt, nz, mean_type, var_type, dtype=dtype,
                                              x0_thr=a_thr, cfg_mul=a_mul)
                else:
                    ref[dtype] = gc.ddim_step(tab3, coefs, pred, pu, 3.0, 0.0, None, None, tt, xt, nz, 0.5, mean_type, var_type,
                                              dtype=dtype, x0_thr=a_thr, cfg_mul=a_mul)
            assert ref[torch.float32]["x_prev"].dtype == torch.float32
            for got, key in zip(outs, gp.STEP_KEYS):
                w64, w32 = clean(ref[torch.float64][key]), clean(ref[torch.float32][key])
                assert got.shape == xt.shape and w64.shape == xt.shape
                errs.setdefault(f"mul {int(use_mul)} thr {int(use_thr)} {key}", []).append(
                    (float((w32 - w64).abs().max()), float((clean(got) - w64).abs().max())))
            if use_thr:
                assert float(outs[1].abs().max()) <= 1.0
    four_times_rule(errs, f"{sampler}_step_g {mean_type} {var_type}")


def test_flow_g_steps_with_arrays_against_f64(ops):
    errs: dict = {}
    t_curr, t_prev, tmax, eta = 0.75, 0.5, 0.9, 0.7
    sigma = ((t_curr / (1 - min(t_curr, tmax))) ** 0.5) * eta
    for B, C, hw in KERNEL_SHAPES:
        xt, nz, pred, pu, mul, _, _ = step_case(B, C, hw, "fixed")
        d = [v.to(DEV) for v in (xt, nz, pred, pu, mul)]
        xp, x0 = ops.euler_step_g(d[0], d[2], d[3], 3.0, d[4], t_curr, t_prev)
        em = ops.euler_maruyama_step_g(d[0], d[2], d[3], 3.0, d[4], d[1], None, t_curr, t_prev, sigma)
        for dtype in (torch.float32, torch.float64):
            v = gc.guided(pred, pu, 3.0, 0.0, False, dtype, cfg_mul=mul)
            e = od.euler_step(xt.to(dtype), v, t_curr, t_prev)
            m = gc.euler_maruyama_step(xt.to(dtype), v, t_curr, t_prev, tmax, eta, nz.to(dtype))
            if dtype == torch.float32:
                e32, m32 = e, m
        for name, got, a32, a64 in (("euler x_prev", xp, e32["x_prev"], e["x_prev"]), ("euler x0", x0, e32["estimated_x0"], e["estimated_x0"]),
                                    ("em x_prev", em[0], m32["x_prev"], m["x_prev"]), ("em mean", em[1], m32["x_prev_mean"], m["x_prev_mean"]),
                                    ("em x0", em[2], m32["estimated_x0"], m["estimated_x0"]), ("em logprob", em[3], m32["logprob"], m["logprob"])):
            errs.setdefault(name, []).append((float((a32.double() - a64).abs().max()), float((got.double().cpu() - a64).abs().max())))
    four_times_rule(errs, "flow step_g")


@pytest.mark.parametrize("hw", [1, 63, 257])
def test_g_step_outputs_stay_inside_their_windows(ops, T, hw):
    B, C = 3, 4
    n = B * C * hw

    def windows(k):
        return [eb.Guarded(1, n, torch.float32, DEV) for _ in range(k)]

    for var_type in gc.VAR_TYPES:
        xt, nz, pred, pu, mul, thr, tt = (v.to(DEV) for v in step_case(B, C, hw, var_type))
        tab, tab3, coefs = (v.to(DEV) for v in gaussian_tables(T, var_type))
        for sampler in ("ddpm", "ddim"):
            w = windows(5)
            tt = tt if sampler == "ddpm" else tt.clamp_min(1)  # (DDIM's logprob is not finite at t == 0, where sigma == 0)
            new_gaussian(ops, sampler, "v", var_type, pred, pu, 3.0, mul, thr, xt, nz, tt, tab, tab3, coefs, True,
                         out=[g.win.view(B, C, hw) for g in w])
            for g, key in zip(w, gp.STEP_KEYS):
                g.check(f"dl_{sampler}_step_g {var_type} hw {hw}: {key}")
        gs, gl = eb.Guarded(1, B, torch.float32, DEV), eb.Guarded(1, 2 * B, torch.float32, DEV)
        from diffulab_amd.ops import _call, _p, _s

        _call("dl_x0_threshold", _p(pred), _p(pu), 3.0, _p(mul), _p(xt), _p(tt), _p(tab), tab.shape[1], 3, None, 0, 0.5, float("inf"),
              _p(gs.win), _p(gl.win), B, C * hw, pred.numel() // B, _s())
        gs.check(f"dl_x0_threshold {var_type} hw {hw}: s")
        gl.check(f"dl_x0_threshold {var_type} hw {hw}: lohi")
    xt, nz, pred, pu, mul, _, _ = (v.to(DEV) for v in step_case(B, C, hw, "fixed"))
    from diffulab_amd.ops import _call, _p, _s

    w = windows(2)
    _call("dl_euler_step_g", _p(xt), _p(pred), _p(pu), 3.0, _p(mul), 0.75, 0.25, _p(w[0].win), _p(w[1].win), B, C * hw, _s())
    w += windows(4)
    _call("dl_euler_maruyama_step_g", _p(xt), _p(pred), _p(pu), 3.0, _p(mul), _p(nz), None, 0.75, 0.25, 0.6, 0.3, _p(w[2].win),
          _p(w[3].win), _p(w[4].win), _p(w[5].win), B, C * hw, _s())
    for i, g in enumerate(w):
        g.check(f"flow step_g hw {hw}: output {i}")


# ------------------------------------------------------------------------------------------------------------------ the loops
STEPS = 6
SHAPE = (2, 3, 5, 7)
FLOW, GAUSSIAN = ("euler", "euler_maruyama"), ("ddpm", "ddim")
TRAINING = 1000
NEW = set(gc.NEW_ENTRY_POINTS)


def loop_inputs():
    y = synth.uniform("gg.y", (SHAPE[0],), lo=0.0, hi=6.0)
    noises = [synth.normal(f"gg.loop.{i}", SHAPE) for i in range(24)]
    return y, noises


def chain(sampler):
    """DDPM: six steps respaced from the 1000-step cosine chain; DDIM (whose respacing takes stride 1 only): a six-step cosine chain"""
    if sampler == "ddpm":
        return od.GaussianTables(TRAINING, n_steps=STEPS, schedule="cosine"), TRAINING
    return od.GaussianTables(STEPS, schedule="cosine"), STEPS


def make(sampler, mean_type="epsilon", bounded=False):
    from diffulab_amd import Diffuser

    if sampler in FLOW:
        model = gc.Stub(1.0).to(DEV)
        return Diffuser(model, sampling_method=sampler, model_type="rectified_flow", n_steps=STEPS), model
    training = chain(sampler)[1]
    model = gc.Stub(1.0 / training, bounded).to(DEV)
    extra = {"schedule": "cosine", "sampler_parameters": {"mean_type": mean_type}}
    if mean_type == "v":
        extra["loss_target"] = "mean_type"
    d = Diffuser(model, sampling_method=sampler, model_type="gaussian_diffusion", n_steps=training, extra_args=extra)
    if training != STEPS:
        d.set_steps(STEPS, schedule="cosine")
    return d, model


def restate(sampler, y, noises, dtype, eta=0.0, mean_type="epsilon", **kw):
    if sampler in FLOW:
        kw.pop("p", None), kw.pop("cap", None)
        return gc.flow_loop(gc.Stub(1.0), od.flow_timesteps(STEPS), SHAPE, y, noises, sampler, 0.7, dtype=dtype, **kw)
    T, training = chain(sampler)
    return gc.gaussian_loop(gc.Stub(1.0 / training), T, training, SHAPE, y, noises, sampler, eta, mean_type, dtype=dtype, **kw)


def hand_out(monkeypatch, noises):
    it = iter(noises)
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: next(it).to(device=ref.device, dtype=ref.dtype))
    monkeypatch.setattr(torch, "randn", lambda *size, device=None, dtype=None, **kw: next(it).to(device=device, dtype=dtype or torch.float32))


OPTIONS = {
    "rescale": dict(phi=0.7),
    "threshold": dict(p=0.9, cap=None),
    "all": dict(phi=0.7, p=0.9, cap=3.0, interval=(0.3, 0.7)),
}
LOOP_CASES = [(s, 0.0, "epsilon", "rescale") for s in FLOW] + [("euler", 0.0, "epsilon", "all"), ("euler_maruyama", 0.0, "epsilon", "all")]
LOOP_CASES += [(s, eta, mt, opt) for s, eta in (("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)) for mt, opt in
               (("epsilon", "rescale"), ("epsilon", "threshold"), ("v", "all"))]
LOOP_CASES += [("euler", 0.0, "epsilon", "image"), ("ddpm", 0.0, "v", "image")]


def generate_kwargs(sampler, opt):
    kw = OPTIONS["all" if opt == "image" else opt]
    out = dict(guidance_scale=5.0)
    if "phi" in kw:
        out["guidance_rescale"] = kw["phi"]
    if "interval" in kw:
        out["guidance_interval"] = kw["interval"]
    if kw.get("p") is not None and sampler in GAUSSIAN:
        out["dynamic_threshold"] = kw["p"]
        if kw.get("cap") is not None:
            out["threshold_max"] = kw["cap"]
    return out


@pytest.mark.parametrize("sampler,eta,mean_type,opt", LOOP_CASES)
def test_loops_against_the_restatement(sampler, eta, mean_type, opt, monkeypatch):
    y, noises = loop_inputs()
    kw = dict(OPTIONS["all" if opt == "image" else opt], guidance=5.0)
    gen = generate_kwargs(sampler, opt)
    if opt == "image":
        init = synth.uniform("gg.init", SHAPE, lo=-1.0, hi=1.0)
        mask = torch.zeros(SHAPE[0], 1, *SHAPE[2:])
        mask[..., 4:] = 1.0
        kw.update(init=init, mask=mask)
        gen.update(init_image=init.to(DEV), mask=mask.to(DEV))
    r64 = restate(sampler, y, noises, torch.float64, eta, mean_type, **dict(kw))
    r32 = restate(sampler, y, noises, torch.float32, eta, mean_type, **dict(kw))
    assert r32["x"].dtype == torch.float32
    want_xt, want_x0 = torch.stack(r64["xt"], dim=1), torch.stack(r64["x0"], dim=1)
    dist = max(float((torch.stack(r32["xt"], dim=1).double() - want_xt).abs().max()),
               float((torch.stack(r32["x0"], dim=1).double() - want_x0).abs().max()), float((r32["x"].double() - r64["x"]).abs().max()))
    assert dist > 0.0
    d, model = make(sampler, mean_type)
    hand_out(monkeypatch, noises)
    out = d.generate({"y": y.to(DEV)}, data_shape=SHAPE, use_tqdm=False, return_intermediates=True,
                     sampler_args={"eta": eta} if sampler == "ddim" else {}, **gen)
    assert out["xt"].shape == (SHAPE[0], STEPS + 1) + SHAPE[1:] and out["estimated_x0"].shape == (SHAPE[0], STEPS) + SHAPE[1:]
    got = max(float((out["xt"].double().cpu() - want_xt).abs().max()), float((out["estimated_x0"].double().cpu() - want_x0).abs().max()),
              float((out["x"].double().cpu() - r64["x"]).abs().max()))
    print(f"\n{sampler} eta {eta} {mean_type} {opt}: max|x| {float(want_xt.abs().max()):.3e}  f32 restatement vs f64 {dist:.3e}  "
          f"product vs f64 {got:.3e}  tolerance {4 * dist:.3e}")
    assert got <= 4 * dist, (got, dist)
    if "dynamic_threshold" in gen:
        assert float(out["estimated_x0"].abs().max()) <= 1.0
    if "guidance_interval" in gen:
        if sampler in FLOW:
            n_guided = gc.guided_steps_flow(od.flow_timesteps(STEPS), gen["guidance_interval"])
        else:
            n_guided = gc.guided_steps_gaussian(*chain(sampler), gen["guidance_interval"])
        assert 0 < n_guided < STEPS and model.calls == STEPS + n_guided
    else:
        assert model.calls == 2 * STEPS


@pytest.mark.parametrize("sampler", GAUSSIAN)
def test_threshold_of_a_model_inside_the_unit_box_changes_nothing(sampler):
    """|x0| <= 0.9 throughout (an x0 predictor behind a tanh): s = 1, and clamp(x0, -1, 1) / 1 returns x0's bits"""
    y, _ = loop_inputs()
    outs = []
    for kw in ({}, {"dynamic_threshold": 0.995}, {"dynamic_threshold": 0.995, "threshold_max": 2.0, "clamp_x": True}):
        d, model = make(sampler, "xstart", bounded=True)
        torch.manual_seed(11)
        outs.append(d.generate({"y": y.to(DEV)}, data_shape=SHAPE, use_tqdm=False, return_intermediates=True, **kw))
        assert model.calls == STEPS and float(outs[-1]["estimated_x0"].abs().max()) <= 0.9
    for o in outs[1:]:
        assert set(o) == set(outs[0]) and all(torch.equal(bits(o[k]), bits(outs[0][k])) for k in o)


@pytest.mark.parametrize("sampler", FLOW + GAUSSIAN)
def test_interval_counts_the_forwards_and_an_empty_one_is_unguided(sampler):
    y, _ = loop_inputs()
    interval = (0.3, 0.7)
    if sampler in FLOW:
        n_guided, empty = gc.guided_steps_flow(od.flow_timesteps(STEPS), interval), (0.0, 0.1)
    else:
        n_guided, empty = gc.guided_steps_gaussian(*chain(sampler), interval), (0.0, 0.5 / chain(sampler)[1])
    assert 0 < n_guided < STEPS

    def run(**kw):
        d, model = make(sampler)
        torch.manual_seed(7)
        out = d.generate({"y": y.to(DEV)}, data_shape=SHAPE, use_tqdm=False, return_intermediates=True, **kw)
        return out, model.calls

    out, calls = run(guidance_scale=5.0, guidance_interval=interval)
    assert calls == STEPS + n_guided
    full, calls = run(guidance_scale=5.0)
    assert calls == 2 * STEPS and not torch.equal(out["x"], full["x"])
    unguided, calls = run(guidance_scale=0)
    assert calls == STEPS
    none, calls = run(guidance_scale=5.0, guidance_interval=empty)
    assert calls == STEPS and all(torch.equal(bits(none[k]), bits(unguided[k])) for k in unguided)
    whole, calls = run(guidance_scale=5.0, guidance_interval=(0.0, 1.0))
    assert calls == 2 * STEPS and all(torch.equal(bits(whole[k]), bits(full[k])) for k in full)


@pytest.mark.parametrize("sampler", FLOW + GAUSSIAN)
def test_defaults_issue_the_calls_they_issued(sampler, ops, monkeypatch):
    y, _ = loop_inputs()
    names = []
    real = ops._call

    def spy(name, *args):
        names.append(name)
        return real(name, *args)

    monkeypatch.setattr(ops, "_call", spy)
    outs = []
    for kw in ({}, dict(guidance_rescale=0.0, guidance_interval=None, dynamic_threshold=None, threshold_max=None)):
        d, model = make(sampler)
        torch.manual_seed(5)
        outs.append(d.generate({"y": y.to(DEV)}, data_shape=SHAPE, use_tqdm=False, guidance_scale=5.0, return_intermediates=True, **kw))
        assert model.calls == 2 * STEPS
    assert len(names) == 2 * STEPS and names[:STEPS] == names[STEPS:] and not NEW & set(names), names
    assert all(torch.equal(bits(outs[0][k]), bits(outs[1][k])) for k in outs[0])
    names.clear()
    d, _ = make(sampler)
    gen = generate_kwargs(sampler, "all")
    d.generate({"y": y.to(DEV)}, data_shape=SHAPE, use_tqdm=False, **gen)
    assert NEW & set(names)
    if sampler == "ddpm":  # a guided, thresholded step is three launches after the forwards
        i = names.index("dl_cfg_rescale_coef")
        assert names[i:i + 3] == ["dl_cfg_rescale_coef", "dl_x0_threshold", "dl_ddpm_step_g"]


# ------------------------------------------------------------------------------------------------------------------ end to end
def _unet():  # the smallest shapes the engine accepts, as tests/test_image_cond_gpu.py sizes them
    from diffulab_amd.networks.denoisers import UNetModel

    return UNetModel(image_size=[16, 16], in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=[2],
                     channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True, n_classes=10,
                     classifier_free=True)


def _dit():
    from diffulab_amd import MMDiT

    return MMDiT(simple_dit=True, input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4,
                 patch_size=2, depth=2, n_classes=10, classifier_free=True)


def test_end_to_end_unet_ddim_v_with_all_three_options():
    from diffulab_amd import Diffuser

    torch.manual_seed(0)
    m = _unet()
    with torch.no_grad():  # the output head starts at zero
        dict(m.named_parameters())["out.2.weight"].normal_(std=0.2)
    m = m.to(DEV).eval()
    assert m.precision == "bf16"
    d = Diffuser(m, sampling_method="ddim", model_type="gaussian_diffusion", n_steps=4,
                 extra_args={"schedule": "cosine", "sampler_parameters": {"mean_type": "v"}, "loss_target": "mean_type"})
    y = synth.integers("gge.y", (4,), 10).to(DEV)
    out = d.generate({"y": y}, data_shape=(4, 1, 16, 16), use_tqdm=False, guidance_scale=5, guidance_rescale=0.7,
                     guidance_interval=(0.3, 0.8), dynamic_threshold=0.995, threshold_max=4.0, return_intermediates=True)
    assert out["x"].shape == (4, 1, 16, 16) and bool(torch.isfinite(out["x"]).all()) and bool(torch.isfinite(out["xt"]).all())
    assert out["estimated_x0"].shape == (4, 4, 1, 16, 16) and float(out["estimated_x0"].abs().max()) <= 1.0


def test_end_to_end_dit_euler_with_rescale_and_interval():
    from diffulab_amd import Diffuser

    torch.manual_seed(0)
    m = _dit()
    with torch.no_grad():
        dict(m.named_parameters())["last_layer.linear.weight"].normal_(std=0.02)
    m = m.to(DEV).eval()
    assert m.precision == "bf16"
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=4)
    y = synth.integers("gge.y", (4,), 10).to(DEV)
    out = d.generate({"y": y}, data_shape=(4, 4, 16, 16), use_tqdm=False, guidance_scale=5, guidance_rescale=0.7,
                     guidance_interval=(0.3, 0.8))  # (64 tokens: the smallest grid the bf16 engine takes at this batch)
    assert out["x"].shape == (4, 4, 16, 16) and bool(torch.isfinite(out["x"]).all())


def test_the_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "guided_sampling.py"), "--train-steps", "4", "--steps", "4"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "estimated_x0" in ln]
    assert len(lines) >= 2, r.stdout
