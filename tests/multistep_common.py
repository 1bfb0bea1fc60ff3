"""Plain-torch / plain-Python restatement of the two second-order multistep samplers as `Diffuser.generate` runs them (imported by the
test modules; not a conftest): variable-step Adams-Bashforth 2 on the rectified-flow velocity ("ab2") and DPM-Solver++(2M) on the DDPM
chains ("dpmpp_2m", Lu et al. 2022).  The reference has neither, so this file states the semantics, from the formulas and not from the
product code.

    ab2        dt = t_curr - t_prev, w = dt / (2 dt_last):  x_prev = x - dt ((1 + w) vc - w v_last)  with a history, else x - dt vc
    dpmpp_2m   alpha_i = sqrt(ab_i), sigma_i = sqrt(1 - ab_i), lambda_i = log(alpha_i / sigma_i), index -1: ab = 1
               h = lambda_{t-1} - lambda_t, a = sigma_{t-1} / sigma_t, e = -alpha_{t-1} expm1(-h)
               first order (b, c) = (e, 0); second order r = (lambda_t - lambda_{t+1}) / h, (b, c) = (e (1 + 1/(2r)), -e / (2r))
               t == 0: (a, b, c) = (0, 1, 0);  x_prev = a x_t + b x0_t + c x0_last
    history    flow: this step's t_curr is the previous step's t_prev (float equality); Gaussian: this index is the previous one - 1,
               and the steps at t == 1 and t == 0 are first order whatever the history

Every step and loop takes a `dtype`: torch.float32 evaluates as the product does, torch.float64 evaluates the same formulas on the
same f32 inputs without rounding.  Host scalars enter both as the f32 values the kernels are handed.

Per-element bounds of the two kernels (`ab2_bounds`, `dpmpp_bounds`), each k * 2^-24 * (the sum of the absolute terms) + 2^-149 with k
the longest chain of roundings any term passes through, plus one unit for the second-order terms.  With A = |u| + |g| (|c| + |u|)
(|c| without a combine) the magnitude of the combined prediction and m = |cfg_mul| (1 without):
    ab2 v_out     c - u, g *, u +, mul *: 4 roundings                                    5 (m A)
    ab2 x0_est    ... t_curr *, x -: 6                                                   7 (|x| + |t_curr| m A)
    ab2 x_prev    ... 1 + w, (1 + w) *, - w v_last, dt *, x -: 9                         10 (|x| + |dt| (|1 + w| m A + |w v_last|))
    dpmpp x0_est  the prediction's 4, the coefficient's 3 (1 - ab, sqrt, / sab), the product, the difference: 9; the threshold's
                  division one more: with X = |xt| / sab + sigma / sab m A (epsilon), sab |xt| + sigma m A (v), m A (xstart)
                  and s the threshold (1 without; clamps are 1-Lipschitz)                11 X / s
    dpmpp x_prev  b x0 carries x0's error; three products and two sums on top: 3         15 |b| X / s + 4 (|a xt| + |c x0_last|)
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

import gd_param_common as gp
import guidance_common as gc
import image_cond_common as ic
from oracle import diffusion as od

U = 2.0**-24
TINY = 2.0**-149
NEW_ENTRY_POINTS = ("dl_ab2_step", "dl_dpmpp_2m_step")
f32r = gc.f32r


# ------------------------------------------------------------------------------------------------------------------ coefficients
def ab2_weight(dt: float, dt_last: float) -> float:
    return dt / (2.0 * dt_last)


def half_log_snr(ab: float) -> float:
    return math.log(math.sqrt(ab) / math.sqrt(1.0 - ab))


def dpmpp_coefs(alphas_bar, t: int, second_order: bool, last_two_first_order: bool = True) -> tuple[float, float, float]:
    """(a, b, c) in double from the chain's fp64 alphas_bar.  last_two_first_order False leaves the step at t == 1 second order (the
    variant the rule exists to exclude)."""
    ab = [float(v) for v in alphas_bar]
    if t == 0:
        return 0.0, 1.0, 0.0
    lam_t, lam_p = half_log_snr(ab[t]), half_log_snr(ab[t - 1])
    h = lam_p - lam_t
    a = math.sqrt(1.0 - ab[t - 1]) / math.sqrt(1.0 - ab[t])
    e = -math.sqrt(ab[t - 1]) * math.expm1(-h)
    if not second_order or (last_two_first_order and t < 2):
        return a, e, 0.0
    r = (lam_t - half_log_snr(ab[t + 1])) / h
    return a, e * (1.0 + 1.0 / (2.0 * r)), -e / (2.0 * r)


# ------------------------------------------------------------------------------------------------------------------ closed-form model
# data N(M, S^2) per element: the exact velocity / noise fields and the exact end of the probability-flow ODE
M, S = 0.3, 0.5


def flow_field(x: Tensor, t: float) -> Tensor:
    V = (1 - t) ** 2 * S * S + t * t
    return -M + (t - (1 - t) * S * S) / V * (x - (1 - t) * M)


def flow_exact(x1: Tensor) -> Tensor:
    return M + S * x1


def gauss_eps(x: Tensor, ab: float) -> Tensor:
    sig2 = 1.0 - ab
    return math.sqrt(sig2) / (ab * S * S + sig2) * (x - math.sqrt(ab) * M)


def gauss_exact(xT: Tensor, ab_T: float) -> Tensor:
    return M + S * (xT - math.sqrt(ab_T) * M) / math.sqrt(ab_T * S * S + (1.0 - ab_T))


def flow_solve(x1: Tensor, timesteps: list[float], method: str) -> Tensor:
    """fp64, the exact field: method "euler" or "ab2" """
    x = x1.double()
    last = None
    for t_curr, t_prev in zip(timesteps[:-1], timesteps[1:]):
        v = flow_field(x, t_curr)
        dt = t_curr - t_prev
        if method == "ab2" and last is not None:
            w = ab2_weight(dt, last[1])
            x = x - dt * ((1 + w) * v - w * last[0])
        else:
            x = x - dt * v
        last = (v, dt)
    return x


def gauss_solve(xT: Tensor, alphas_bar, method: str, last_two_first_order: bool = True) -> Tensor:
    """fp64, the exact field, from index T - 1 down: method "ddim" (eta 0, written as alpha_{t-1} x0 + sigma_{t-1} eps) or "dpmpp_2m" """
    ab = [float(v) for v in alphas_bar]
    x = xT.double()
    x0_last = None
    for t in range(len(ab) - 1, -1, -1):
        eps = gauss_eps(x, ab[t])
        x0 = (x - math.sqrt(1.0 - ab[t]) * eps) / math.sqrt(ab[t])
        if method == "ddim":
            ab_p = ab[t - 1] if t > 0 else 1.0
            x = math.sqrt(ab_p) * x0 + math.sqrt(1.0 - ab_p) * eps
        else:
            a, b, c = dpmpp_coefs(ab, t, x0_last is not None, last_two_first_order)
            x = a * x + b * x0 + (c * x0_last if c != 0.0 else 0.0)
        x0_last = x0
    return x


# ------------------------------------------------------------------------------------------------------------------ the two steps
def _per_sample(v: Tensor | None, like: Tensor, dtype):
    return None if v is None else v.to(dtype).view(-1, *([1] * (like.dim() - 1)))


def ab2_step(x, v, vu, g, mul, v_last, t_curr: float, dt: float, w: float, dtype=torch.float64) -> dict[str, Tensor]:
    """t_curr, dt, w: the f32 values the kernel is handed.  v_last None: the Euler step"""
    x = x.to(dtype)
    vc = gc.guided(v, vu, g, 0.0, False, dtype, cfg_mul=mul)
    d = vc if v_last is None else (1.0 + w) * vc - w * v_last.to(dtype)
    return {"x_prev": x - d * dt, "estimated_x0": x - vc * t_curr, "v_out": vc}


def _magnitude(c, u, g, mul):
    A = c.double().abs() if u is None else u.double().abs() + abs(g) * (c.double().abs() + u.double().abs())
    return A if mul is None else _per_sample(mul, A, torch.float64).abs() * A


def ab2_bounds(x, v, vu, g, mul, v_last, t_curr: float, dt: float, w: float) -> dict[str, Tensor]:
    mA, ax = _magnitude(v, vu, g, mul), x.double().abs()
    inner = mA if v_last is None else abs(1.0 + w) * mA + abs(w) * v_last.double().abs()
    return {"v_out": 5 * U * mA + TINY, "estimated_x0": 7 * U * (ax + abs(t_curr) * mA) + TINY, "x_prev": 10 * U * (ax + abs(dt) * inner) + TINY}


def _mean_half(pred, halves: bool):
    return None if pred is None else (torch.chunk(pred, 2, dim=1)[0] if halves else pred)


def dpmpp_step(tab: Tensor, pred, pu, g, mul, thr, xt, x0_last, t, mean_type: str, var_type: str, clamp_x: bool, a: float, b: float,
               c: float, dtype=torch.float64, p: float | None = None, cap: float | None = None) -> dict[str, Tensor]:
    """tab f32 [>= 2, T] = sqrt_ab, ab; a, b, c: the f32 values the kernel is handed.  thr: a given threshold array, or p (and cap):
    the dynamic threshold of the x0 formed here"""
    halves = var_type != "fixed"
    o = _mean_half(gc.guided(pred, pu, g, 0.0, halves, dtype, cfg_mul=mul), halves)
    x = xt.to(dtype)
    shape = (-1,) + (1,) * (x.dim() - 1)
    sab, ab = (tab[k][t.long()].to(dtype).view(shape) for k in range(2))
    x0 = gp.x_start(o, x, [sab, ab, torch.ones_like(sab), torch.zeros_like(sab)], mean_type)
    if thr is not None or p is not None:
        x0 = gc.apply_threshold(x0, thr.to(dtype) if thr is not None else gc.threshold_of(x0, p, cap, dtype))
    if clamp_x:
        x0 = x0.clamp(-1, 1)
    xp = b * x0
    if a != 0.0:
        xp = xp + a * x
    if x0_last is not None and c != 0.0:
        xp = xp + c * x0_last.to(dtype)
    return {"x_prev": xp, "estimated_x0": x0}


def dpmpp_bounds(tab: Tensor, pred, pu, g, mul, thr, xt, x0_last, t, mean_type: str, var_type: str, a: float, b: float,
                 c: float) -> dict[str, Tensor]:
    halves = var_type != "fixed"
    mA = _magnitude(_mean_half(pred, halves), _mean_half(pu, halves), g, mul)
    ax = xt.double().abs()
    shape = (-1,) + (1,) * (xt.dim() - 1)
    sab, ab = (tab[k][t.long()].double().view(shape) for k in range(2))
    sig = (1.0 - ab).sqrt()
    X = {"epsilon": ax / sab + sig / sab * mA, "v": sab * ax + sig * mA, "xstart": mA}[mean_type]
    if thr is not None:
        X = X / _per_sample(thr, X, torch.float64)
    rest = abs(a) * ax + (0.0 if x0_last is None else abs(c) * x0_last.double().abs())
    return {"estimated_x0": 11 * U * X + TINY, "x_prev": U * (15 * abs(b) * X + 4 * rest) + TINY}


# ------------------------------------------------------------------------------------------------------------------ the two loops
def _predictions(model, x, t_value, y, dtype, is_guided):
    return gc._predictions(model, x, t_value, y, dtype, is_guided)


def flow_loop(model, timesteps: list[float], y: Tensor, noises: list[Tensor], guidance: float = 0.0, phi: float = 0.0, interval=None,
              init: Tensor | None = None, mask: Tensor | None = None, strength: float = 1.0, resample: int = 1,
              dtype=torch.float64, orders: list | None = None) -> dict:
    """-> {"x", "xt": [starting x, x_prev after the blend of every step's last repeat], "x0": [that repeat's estimated_x0], "mean":
    [that repeat's x_prev as the step made it, before the blend]}.  Noises: eps0, then the re-noise draw between two repeats.  orders
    (if given) receives 1 or 2 for every launch"""
    draw = iter(noises)
    eps0 = next(draw).to(dtype)
    steps = len(timesteps) - 1
    k, x = steps, eps0
    if init is not None:
        init = init.to(dtype)
        k = ic.strength_steps(steps, strength)
        t0 = f32r(timesteps[steps - k])
        x = (1 - t0) * init + t0 * eps0
    i0 = steps - k
    xt, x0s, means = [x], [], []
    last = None  # (v_out, the t_prev stepped to, dt)
    for j, (t_curr, t_prev) in enumerate(zip(timesteps[i0:-1], timesteps[i0 + 1:])):
        repeats = resample if (init is not None and j + 1 < k) else 1
        for r in range(repeats):
            is_guided = guidance > 0 and gc.in_interval(interval, t_curr)
            v, vu = _predictions(model, x, t_curr, y, dtype, is_guided)
            mul = gc.rescale_coef(v, vu, guidance, phi, dtype) if is_guided and phi > 0 else None
            dt = t_curr - t_prev
            valid = last is not None and last[1] == t_curr
            w = f32r(ab2_weight(dt, last[2])) if valid else 0.0
            out = ab2_step(x, v, vu, guidance, mul, last[0] if valid else None, f32r(t_curr), f32r(dt), w, dtype)
            if orders is not None:
                orders.append(2 if valid else 1)
            last = (out["v_out"], t_prev, dt)
            xp = out["x_prev"]
            if mask is not None:
                xp = ic.blend_ref(xp, init, eps0, mask, f32r(1.0 - t_prev), f32r(t_prev), dtype)
            x = xp
            if r + 1 < repeats:
                a, s = (f32r(c) for c in ic.flow_renoise_coefs(t_curr, t_prev))
                x = a * xp + s * next(draw).to(dtype)
        xt.append(xp)
        x0s.append(out["estimated_x0"])
        means.append(out["x_prev"])
    return {"x": x, "xt": xt, "x0": x0s, "mean": means}


def gaussian_loop(model, T: od.GaussianTables, training_steps: int, y: Tensor, noises: list[Tensor], mean_type: str = "epsilon",
                  guidance: float = 0.0, phi: float = 0.0, interval=None, p: float | None = None, cap: float | None = None,
                  init: Tensor | None = None, mask: Tensor | None = None, strength: float = 1.0, resample: int = 1,
                  dtype=torch.float64, orders: list | None = None) -> dict:
    """the chain of `T` (fixed variances); the stub sees the training index timestep_map[t].  Noises: eps0, then per repeat the known
    region's draw (mask, t > 0) and the re-noise draw (when another repeat follows): the sampler itself draws nothing.  "mean": every
    step's x_prev as the step made it, before the blend -- what the product records as xt_mean"""
    draw = iter(noises)
    eps0 = next(draw).to(dtype)
    B = eps0.shape[0]
    k, x = T.steps, eps0
    if init is not None:
        init = init.to(dtype)
        k = ic.strength_steps(T.steps, strength)
        x = od.ddpm_add_noise(T, init, torch.full((B,), k - 1, dtype=torch.int32), eps0)
    tab = gp.ddim_tables(T)
    xt, x0s, means = [x], [], []
    last = None  # (x0_est, the index of the step that formed it)
    for t in range(k - 1, -1, -1):
        repeats = resample if (init is not None and t > 0) else 1
        tt = torch.full((B,), t, dtype=torch.int32)
        tau = T.timestep_map[t] if T.timestep_map else t
        for r in range(repeats):
            is_guided = guidance > 0 and gc.in_interval(interval, gc.gaussian_level(T.timestep_map, training_steps, t))
            pred, pu = _predictions(model, x, tau, y, dtype, is_guided)
            mul = gc.rescale_coef(pred, pu, guidance, phi, dtype) if is_guided and phi > 0 else None
            valid = last is not None and last[1] == t + 1 and t >= 2
            a, b, c = (f32r(v) for v in dpmpp_coefs(T.alphas_bar, t, valid))
            out = dpmpp_step(tab, pred, pu, guidance, mul, None, x, last[0] if valid else None, tt, mean_type, "fixed", False, a, b, c,
                             dtype, p, cap)
            if orders is not None:
                orders.append(2 if valid else 1)
            last = (out["estimated_x0"], t)
            xp = out["x_prev"]
            if mask is not None:
                if t > 0:
                    ka, kb = f32r(T.sqrt_alphas_bar[t - 1]), f32r((1.0 - T.alphas_bar[t - 1]).sqrt())
                    xp = ic.blend_ref(xp, init, next(draw), mask, ka, kb, dtype)
                else:
                    xp = ic.blend_ref(xp, init, None, mask, 1.0, 0.0, dtype)
            x = xp
            if r + 1 < repeats:
                ra, rs = (f32r(cf) for cf in ic.gaussian_renoise_coefs(T.betas, t))
                x = ra * xp + rs * next(draw).to(dtype)
        xt.append(xp)
        x0s.append(out["estimated_x0"])
        means.append(out["x_prev"])
    return {"x": x, "xt": xt, "x0": x0s, "mean": means}
