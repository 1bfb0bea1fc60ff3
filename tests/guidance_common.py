"""Plain-torch restatement of guided sampling as `Diffuser.generate` runs it (imported by the test modules; not a conftest): CFG rescale
(Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", 2023, sec. 3.4), dynamic thresholding (Saharia et al.,
Imagen, 2022) and the guidance interval (Kynkaanniemi et al., 2024).  The reference has none of them, so this file states the semantics.

Every function takes a `dtype`: torch.float32 evaluates as the product does, torch.float64 evaluates the same formulas on the same
f32 inputs without rounding.  The sampler steps build on tests/gd_param_common.py / learned_variance_common.py / the oracle.

The loops take the run's noises as a list, in the order the product draws them (tests/image_cond_common.py).
"""

from __future__ import annotations

import math

import torch
from torch import Tensor, nn

import gd_param_common as gp
import image_cond_common as ic
import learned_variance_common as lv
from oracle import diffusion as od

MEAN_TYPES = ("epsilon", "xstart", "xprev", "v")
VAR_TYPES = ("fixed", "learned", "learned_range")
NEW_ENTRY_POINTS = ("dl_cfg_rescale_coef", "dl_abs_quantile_rows", "dl_x0_threshold", "dl_euler_step_g", "dl_euler_maruyama_step_g",
                    "dl_ddpm_step_g", "dl_ddim_step_g")


# ------------------------------------------------------------------------------------------------------------------ the quantile
def quantile_position(p: float, n: int) -> tuple[int, float]:
    """torch.quantile's `linear` rule: pos = p (n - 1) in double, k = floor(pos), f = float32(pos - k).  (Where that fraction rounds
    up to 1.0 the position is (k + 1, 0): the same value.)"""
    pos = float(p) * (n - 1)
    k = min(int(math.floor(pos)), n - 1)
    f = float(torch.tensor(pos - k, dtype=torch.float64).to(torch.float32))
    if f >= 1.0:
        k, f = min(k + 1, n - 1), 0.0
    return k, f


def order_stats(x: Tensor, k: int, dtype=torch.float64) -> tuple[Tensor, Tensor]:
    """x [B, n] -> (lo, hi): the k-th and min(k + 1, n - 1)-th smallest |x| of every row (0-based)"""
    v = x.to(dtype).abs().sort(dim=1).values
    return v[:, k], v[:, min(k + 1, v.shape[1] - 1)]


def abs_quantile(x: Tensor, p: float, dtype=torch.float64) -> Tensor:
    """x [B, n] -> the p-quantile of |x| of every row: lo + f (hi - lo)"""
    k, f = quantile_position(p, x.shape[1])
    lo, hi = order_stats(x, k, dtype)
    return lo + torch.tensor(f, dtype=dtype) * (hi - lo)


def threshold_of(x0: Tensor, p: float, cap: float | None, dtype=torch.float64) -> Tensor:
    """s [B] = min(max(a, 1), cap), a the p-quantile of |x0| over each sample"""
    s = abs_quantile(x0.to(dtype).flatten(1), p, dtype).clamp_min(1.0)
    return s if cap is None else s.clamp_max(cap)


def apply_threshold(x0: Tensor, s: Tensor) -> Tensor:
    s = s.view(-1, *([1] * (x0.dim() - 1)))
    return torch.maximum(torch.minimum(x0, s), -s) / s


# ------------------------------------------------------------------------------------------------------------------ combine, rescale
def rescale_coef(c: Tensor, u: Tensor, g: float, phi: float, dtype=torch.float64) -> Tensor:
    """r [B] = 1 - phi + phi sqrt(S_c / S_o); r = 1 where S_o == 0"""
    c, u = c.to(dtype).flatten(1), u.to(dtype).flatten(1)
    o = u + g * (c - u)
    S_c = ((c - c.mean(dim=1, keepdim=True)) ** 2).sum(dim=1)
    S_o = ((o - o.mean(dim=1, keepdim=True)) ** 2).sum(dim=1)
    safe = torch.where(S_o > 0, S_o, torch.ones_like(S_o))
    return torch.where(S_o > 0, (1.0 - phi) + phi * (S_c / safe).sqrt(), torch.ones_like(S_o))


def guided(pred: Tensor, pred_uncond: Tensor | None, g: float, phi: float, halves: bool, dtype=torch.float64,
           cfg_mul: Tensor | None = None) -> Tensor:
    """the prediction the step works from: the plain combine, its mean half scaled by r (a variance half keeps the plain combine).
    cfg_mul [B]: a given factor instead of phi's (the kernels take any; it then also scales an uncombined prediction)"""
    pred = pred.to(dtype)
    C = pred.shape[1] // 2 if halves else pred.shape[1]
    o = pred
    r = None if cfg_mul is None else cfg_mul.to(dtype)
    if pred_uncond is not None:
        pu = pred_uncond.to(dtype)
        o = pu + g * (pred - pu)
        if r is None and phi > 0:
            r = rescale_coef(pred[:, :C], pu[:, :C], g, phi, dtype)
    if r is not None:
        o = torch.cat([r.view(-1, *([1] * (pred.dim() - 1))) * o[:, :C], o[:, C:]], dim=1)
    return o


# ------------------------------------------------------------------------------------------------------------------ the steps
def ddpm_step(tab: Tensor, pred, pred_uncond, g, phi, p, cap, t, xt, noise, mean_type: str, var_type: str, clamp_x: bool = False,
              dtype=torch.float64, x0_thr: Tensor | None = None, cfg_mul: Tensor | None = None) -> dict[str, Tensor]:
    """tab: gp.fixed_tables(T) for var_type "fixed", lv.tables(T) otherwise.  x0_thr / cfg_mul: given arrays instead of p's / phi's"""
    halves = var_type != "fixed"
    o = guided(pred, pred_uncond, g, phi, halves, dtype, cfg_mul)
    xt, noise = xt.to(dtype), noise.to(dtype)
    rows = gp._rows(tab, t, xt, dtype)
    if halves:
        o, v = torch.chunk(o, 2, dim=1)
        lvar = lv.log_variance(v, rows, var_type)
        var = lvar.exp()
    else:
        var, lvar = rows[4].expand_as(xt), rows[5].expand_as(xt)
    x0 = gp.x_start(o, xt, rows, mean_type)
    if x0_thr is not None or p is not None:
        x0 = apply_threshold(x0, x0_thr.to(dtype) if x0_thr is not None else threshold_of(x0, p, cap, dtype))
    if clamp_x:
        x0 = x0.clamp(-1, 1)
    mean = gp.posterior_mean(rows, x0, xt)
    mask = (t > 0).to(dtype).view(rows[0].shape)
    x_prev = mean + mask * noise * torch.exp(0.5 * lvar)
    vs = var.clamp_min(1e-20)
    logprob = (-((x_prev - mean) ** 2) / (2.0 * vs) - torch.log(2 * torch.pi * vs) * 0.5) * mask
    return {"x_prev": x_prev, "estimated_x0": x0, "x_prev_mean": mean, "x_prev_std": vs.sqrt(), "logprob": logprob}


def ddim_step(tab3: Tensor, coefs: Tensor, pred, pred_uncond, g, phi, p, cap, t, xt, noise, eta: float, mean_type: str, var_type: str,
              clamp_x: bool = False, dtype=torch.float64, x0_thr: Tensor | None = None, cfg_mul: Tensor | None = None) -> dict[str, Tensor]:
    """tab3 = gp.ddim_tables(T); coefs f32 [2, T] = posterior_mean_coef1, coef2 (mean_type xprev reads them)"""
    halves = var_type != "fixed"
    o = guided(pred, pred_uncond, g, phi, halves, dtype, cfg_mul)
    if halves:
        o = torch.chunk(o, 2, dim=1)[0]
    shape = (-1,) + (1,) * (xt.dim() - 1)
    rows = [tab3[k][t.long()].to(dtype).view(shape) for k in range(2)] + [coefs[k][t.long()].to(dtype).view(shape) for k in range(2)]
    x0 = gp.x_start(o, xt.to(dtype), rows, mean_type)
    if x0_thr is not None or p is not None:
        x0 = apply_threshold(x0, x0_thr.to(dtype) if x0_thr is not None else threshold_of(x0, p, cap, dtype))
    if clamp_x:
        x0 = x0.clamp(-1, 1)
    return gp.ddim_step(tab3, x0, t, xt, noise, eta, dtype)


def f32r(v: float) -> float:
    return float(torch.tensor(float(v), dtype=torch.float64).to(torch.float32))


def euler_maruyama_step(x: Tensor, v: Tensor, t_curr: float, t_prev: float, tmax: float, eta: float, noise: Tensor) -> dict[str, Tensor]:
    """euler_meruyama.py:39-57 in the dtype of x.  The host scalars enter as the f32 values the kernel is handed (t_curr, dt, sigma,
    std = sigma sqrt(dt) formed in double first, sigma^2 / (2 t_curr) formed in double from the f32 sigma), so that the two dtypes
    differ by the device arithmetic alone."""
    sigma = ((t_curr / (1 - min(t_curr, tmax))) ** 0.5) * eta
    t32, dt32, sigma32, std32 = f32r(t_curr), f32r(t_curr - t_prev), f32r(sigma), f32r(sigma * (t_curr - t_prev) ** 0.5)
    drift = f32r(sigma32 * sigma32 / (2.0 * t32))
    mean = x - (v + drift * (x + (1 - t32) * v)) * dt32
    x_prev = mean + std32 * noise
    log_std = f32r(math.log(std32)) if x.dtype == torch.float32 else math.log(std32)
    logprob = -((x_prev - mean) ** 2 / (2 * std32 * std32) + log_std + 0.5 * math.log(2 * math.pi))
    return {"x_prev": x_prev, "x_prev_mean": mean, "estimated_x0": x - v * t32, "logprob": logprob}


def coefs_of(T: od.GaussianTables) -> Tensor:
    return torch.stack([T.posterior_mean_coef1, T.posterior_mean_coef2]).float()


# ------------------------------------------------------------------------------------------------------------------ the interval
def in_interval(interval, level: float) -> bool:
    return interval is None or interval[0] <= level <= interval[1]


def gaussian_level(timestep_map: list[int], training_steps: int, t: int) -> float:
    tau = timestep_map[t] if timestep_map else t
    return (tau + 1) / training_steps


def guided_steps_flow(timesteps: list[float], interval) -> int:
    return sum(in_interval(interval, t) for t in timesteps[:-1])


def guided_steps_gaussian(T: od.GaussianTables, training_steps: int, interval) -> int:
    return sum(in_interval(interval, gaussian_level(T.timestep_map, training_steps, t)) for t in range(T.steps))


# ------------------------------------------------------------------------------------------------------------------ stub denoiser
class Stub(nn.Module):
    """a denoiser with the interface the loops use: one parameter (device / dtype probe), a fixed smooth function of x, t, y and p
    (p = 1 drops the label term), counting its calls.  t_scale brings the timestep to O(1): 1 for flow, 1 / training_steps for the
    Gaussian chains."""

    def __init__(self, t_scale: float = 1.0, bounded: bool = False) -> None:
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1))
        self.t_scale, self.bounded = t_scale, bounded
        self.calls = 0

    def forward(self, x: Tensor, timesteps: Tensor, y: Tensor | None = None, p=0, **kw) -> dict[str, Tensor]:
        self.calls += 1
        shape = (-1,) + (1,) * (x.dim() - 1)
        t = timesteps.to(device=x.device, dtype=x.dtype).view(shape) * self.t_scale
        out = 0.5 * x + 0.1 * torch.roll(x, 1, -1) - t
        if y is not None:
            out = out + (1.0 - float(p)) * 0.3 * torch.sin(2.0 * x + y.to(device=x.device, dtype=x.dtype).view(shape))
        return {"x": 0.9 * torch.tanh(out) if self.bounded else out}


def _predictions(model: Stub, x: Tensor, t_value, y: Tensor, dtype, is_guided: bool):
    t = torch.full((x.shape[0],), t_value, dtype=dtype)
    pred = model(x=x, timesteps=t, y=y.to(dtype), p=0)["x"]
    return pred, (model(x=x, timesteps=t, y=y.to(dtype), p=1)["x"] if is_guided else None)


# ------------------------------------------------------------------------------------------------------------------ the two loops
def flow_loop(model: Stub, timesteps: list[float], shape, y: Tensor, noises: list[Tensor], sampler: str = "euler", eta: float = 0.7,
              guidance: float = 0.0, phi: float = 0.0, interval=None, init: Tensor | None = None, mask: Tensor | None = None,
              dtype=torch.float64) -> dict:
    """-> {"x", "xt": [starting x, every step's x_prev], "x0": [every step's estimated_x0]}.  With init (and mask): the image-to-image
    form at strength 1, as tests/image_cond_common.py states it"""
    draw = iter(noises)
    eps0 = next(draw).to(dtype)
    x = eps0 if init is None else (1 - timesteps[0]) * init.to(dtype) + timesteps[0] * eps0
    xt, x0s = [x], []
    for t_curr, t_prev in zip(timesteps[:-1], timesteps[1:]):
        is_guided = guidance > 0 and in_interval(interval, t_curr)
        v, vu = _predictions(model, x, t_curr, y, dtype, is_guided)
        v = guided(v, vu, guidance, phi, False, dtype)
        if sampler == "euler":
            out = od.euler_step(x, v, t_curr, t_prev)
        else:
            out = od.euler_maruyama_step(x, v, t_curr, t_prev, timesteps[1], eta, noise=next(draw).to(dtype))
        x = out["x_prev"]
        if mask is not None:
            x = ic.blend_ref(x, init.to(dtype), eps0, mask, 1.0 - t_prev, t_prev, dtype)
        xt.append(x)
        x0s.append(out["estimated_x0"])
    return {"x": x, "xt": xt, "x0": x0s}


def gaussian_loop(model: Stub, T: od.GaussianTables, training_steps: int, shape, y: Tensor, noises: list[Tensor], sampler: str = "ddpm",
                  eta: float = 0.0, mean_type: str = "epsilon", guidance: float = 0.0, phi: float = 0.0, interval=None,
                  p: float | None = None, cap: float | None = None, init: Tensor | None = None, mask: Tensor | None = None,
                  dtype=torch.float64) -> dict:
    """the chain of `T` (fixed_small variances); the stub sees the training index timestep_map[t].  With init (and mask): the
    image-to-image form at strength 1"""
    draw = iter(noises)
    eps0 = next(draw).to(dtype)
    B = shape[0]
    f32 = lambda v: float(torch.as_tensor(float(v), dtype=torch.float64).float())  # noqa: E731
    x = eps0 if init is None else od.ddpm_add_noise(T, init.to(dtype), torch.full((B,), T.steps - 1, dtype=torch.int32), eps0)
    tab, tab3, coefs = gp.fixed_tables(T), gp.ddim_tables(T), coefs_of(T)
    xt, x0s = [x], []
    for t in range(T.steps - 1, -1, -1):
        tt = torch.full((B,), t, dtype=torch.int32)
        tau = T.timestep_map[t] if T.timestep_map else t
        is_guided = guidance > 0 and in_interval(interval, gaussian_level(T.timestep_map, training_steps, t))
        pred, pu = _predictions(model, x, tau, y, dtype, is_guided)
        nz = next(draw).to(dtype)
        if sampler == "ddpm":
            out = ddpm_step(tab, pred, pu, guidance, phi, p, cap, tt, x, nz, mean_type, "fixed", dtype=dtype)
        else:
            out = ddim_step(tab3, coefs, pred, pu, guidance, phi, p, cap, tt, x, nz, eta, mean_type, "fixed", dtype=dtype)
        x = out["x_prev"]
        if mask is not None:
            if t > 0:
                a, b = f32(T.sqrt_alphas_bar[t - 1]), f32((1.0 - T.alphas_bar[t - 1]).sqrt())
                x = ic.blend_ref(x, init.to(dtype), next(draw), mask, a, b, dtype)
            else:
                x = ic.blend_ref(x, init.to(dtype), None, mask, 1.0, 0.0, dtype)
        xt.append(x)
        x0s.append(out["estimated_x0"])
    return {"x": x, "xt": xt, "x0": x0s}
