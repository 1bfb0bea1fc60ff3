"""Plain-torch restatement of the learned-variance sampler step and of the hybrid loss (imported by the test modules; not a conftest).

Step: reference samplers/gaussian_diffusion/ddpm.py:212-222 (get_variance), 268-282 (the chunk of the [B, 2C, H, W] prediction) and
330-363 (step), with the `randn_like` of :302 passed in.  DDIM (ddim.py:89) discards the variance half.
Loss: L_simple + L_vlb of Nichol & Dhariwal, "Improved Denoising Diffusion Probabilistic Models" (2021), eq. 16, with the predicted
mean frozen inside the bound -- the reference announces it and leaves it unwritten (gaussian_diffusion.py:267).

Every function takes `tab`, the f32 [6, T] table the kernels read (sqrt_ab, ab, posterior_mean_coef1, coef2,
posterior_log_variance_clipped, betas: the `.float()` gathers of the fp64 schedule), and a `dtype`: torch.float32 evaluates as the
reference does, torch.float64 evaluates the same formulas on the same f32 inputs without rounding, which is what the GPU tests compare
the kernels with.
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from oracle import diffusion as od
from oracle import synth

MEAN_TYPES = ("epsilon", "xstart", "xprev")
VAR_TYPES = ("learned", "learned_range")
STEP_KEYS = ("x_prev", "estimated_x0", "x_prev_mean", "x_prev_std", "logprob")


def tables(T: od.GaussianTables) -> Tensor:
    return torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.posterior_mean_coef1, T.posterior_mean_coef2,
                        T.posterior_log_variance_clipped, T.betas]).float()


def _rows(tab: Tensor, t: Tensor, like: Tensor, dtype) -> list[Tensor]:
    shape = (-1,) + (1,) * (like.dim() - 1)
    return [tab[k][t.long()].to(dtype).view(shape) for k in range(6)]


def x_start(o: Tensor, xt: Tensor, rows, mean_type: str) -> Tensor:
    sab, ab, c1, c2 = rows[:4]
    if mean_type == "xstart":
        return o
    if mean_type == "epsilon":
        return (1.0 / sab) * xt - ((torch.ones_like(o) - ab).sqrt() / sab) * o  # ddpm.py:118-121
    return (1.0 / c1) * o - (c2 / c1) * xt  # ddpm.py:99-102


def log_variance(v: Tensor, rows, var_type: str) -> Tensor:
    if var_type == "learned":
        return v
    w = (v + 1) / 2  # ddpm.py:218-221
    return w * rows[5].log() + (1 - w) * rows[4]


def cfg_combine(pred: Tensor, pred_uncond: Tensor, g: float) -> Tensor:
    return pred_uncond + g * (pred - pred_uncond)  # gaussian_diffusion.py:253-255, on the whole 2C tensor


def ddpm_step(tab: Tensor, pred: Tensor, t: Tensor, xt: Tensor, noise: Tensor, mean_type: str, var_type: str, clamp_x: bool = False,
              dtype=torch.float32) -> dict[str, Tensor]:
    pred, xt, noise = pred.to(dtype), xt.to(dtype), noise.to(dtype)
    rows = _rows(tab, t, xt, dtype)
    o, v = torch.chunk(pred, 2, dim=1)
    x0 = x_start(o, xt, rows, mean_type)
    if clamp_x:
        x0 = x0.clamp(-1, 1)
    mean = rows[2] * x0 + rows[3] * xt
    lv = log_variance(v, rows, var_type)
    var = lv.exp()
    mask = (t > 0).to(dtype).view(rows[0].shape)
    x_prev = mean + mask * noise * torch.exp(0.5 * lv)
    vs = var.clamp_min(1e-20)
    logprob = (-((x_prev - mean) ** 2) / (2.0 * vs) - torch.log(2 * torch.pi * vs) * 0.5) * mask
    return {"x_prev": x_prev, "estimated_x0": x0, "x_prev_mean": mean, "x_prev_std": vs.sqrt(), "logprob": logprob}


def ddim_step(T: od.GaussianTables, pred: Tensor, t: Tensor, xt: Tensor, noise: Tensor, eta: float, mean_type: str = "epsilon",
              clamp_x: bool = False) -> dict[str, Tensor]:
    """the oracle's fixed-variance DDIM step on the mean half"""
    return od.ddim_step(T, torch.chunk(pred, 2, dim=1)[0], t, xt, noise, eta, mean_type, clamp_x)


# ------------------------------------------------------------------------------------------------------------------ hybrid loss
K_TANH = math.sqrt(2.0 / math.pi)
LN2 = math.log(2.0)


def approx_cdf(z: Tensor) -> Tensor:
    return 0.5 * (1.0 + torch.tanh(K_TANH * (z + 0.044715 * z**3)))


def approx_cdf_grad(z: Tensor) -> Tensor:
    th = torch.tanh(K_TANH * (z + 0.044715 * z**3))
    return 0.5 * (1.0 - th * th) * K_TANH * (1.0 + 3 * 0.044715 * z * z)


def hybrid_parts(tab: Tensor, pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, mean_type: str, var_type: str,
                 dtype=torch.float64) -> dict[str, Tensor]:
    """every intermediate of the loss, differentiable with respect to `pred` (the mean is detached inside the bound)"""
    pred = pred.to(dtype)
    eps, x0, xt = eps.to(dtype), x0.to(dtype), xt.to(dtype)
    rows = _rows(tab, t, xt, dtype)
    c1, c2, lv_q = rows[2], rows[3], rows[4]
    o, v = torch.chunk(pred, 2, dim=1)
    mse = ((eps - o) ** 2).mean()
    m_p = (c1 * x_start(o, xt, rows, mean_type) + c2 * xt).detach()  # stop-gradient: the bound trains the variance only
    m_q = c1 * x0 + c2 * xt
    lv_p = log_variance(v, rows, var_type)
    kl = 0.5 * (-1.0 + lv_p - lv_q + torch.exp(lv_q - lv_p) + (m_q - m_p) ** 2 * torch.exp(-lv_p))
    c, s = x0 - m_p, torch.exp(-0.5 * lv_p)
    zp, zm = s * (c + 1.0 / 255.0), s * (c - 1.0 / 255.0)
    P, Q = approx_cdf(zp), approx_cdf(zm)
    lo, hi = x0 < -0.999, x0 > 0.999
    prob = torch.where(lo, P, torch.where(hi, 1.0 - Q, P - Q))
    nll = -torch.log(prob.clamp(min=1e-12))
    first = (t == 0).view(rows[0].shape).expand_as(kl)
    term = torch.where(first, nll, kl)
    vb = (term.flatten(1).mean(1) / LN2).mean()
    return {"mse": mse, "vb": vb, "prob": prob, "first": first, "lv_p": lv_p, "lv_q": lv_q, "m_p": m_p, "m_q": m_q, "zp": zp, "zm": zm,
            "lo": lo, "hi": hi, "o": o, "rows": rows}


def hybrid_loss(tab, pred, eps, x0, xt, t, mean_type, var_type, dtype=torch.float64) -> tuple[Tensor, Tensor]:
    p = hybrid_parts(tab, pred, eps, x0, xt, t, mean_type, var_type, dtype)
    return p["mse"], p["vb"]


def hybrid_backward(tab, pred, eps, x0, xt, t, mean_type, var_type, g_mse: float = 1.0, g_vb: float = 1.0, dtype=torch.float64) -> Tensor:
    """d(g_mse * mse + g_vb * vb) / d pred, written out by hand: what the backward kernel computes"""
    with torch.no_grad():
        p = hybrid_parts(tab, pred, eps, x0, xt, t, mean_type, var_type, dtype)
        n = p["o"].numel()
        d_o = g_mse * 2.0 * (p["o"] - eps.to(dtype)) / n
        lv_p, lv_q = p["lv_p"], p["lv_q"]
        r, q = torch.exp(lv_q - lv_p), (p["m_q"] - p["m_p"]) ** 2 * torch.exp(-lv_p)
        d_kl = 0.5 * (1.0 - r - q)
        zp, zm = p["zp"], p["zm"]
        dP, dQ = approx_cdf_grad(zp) * (-0.5 * zp), approx_cdf_grad(zm) * (-0.5 * zm)  # d z / d lv_p = -z / 2
        dprob = torch.where(p["lo"], dP, torch.where(p["hi"], -dQ, dP - dQ))
        d_nll = torch.where(p["prob"] > 1e-12, -dprob / p["prob"], torch.zeros_like(dprob))
        d_lv = torch.where(p["first"], d_nll, d_kl)
        rows = p["rows"]
        dlv_dv = torch.ones_like(lv_q) if var_type == "learned" else 0.5 * (rows[5].log() - lv_q)
        d_v = g_vb / (n * LN2) * d_lv * dlv_dv
        return torch.cat([d_o, d_v], dim=1)


# ------------------------------------------------------------------------------------------------------------------ loss test inputs
LOSS_SHAPE = (5, 3, 8, 8)  # B * chw = 960: not a multiple of the 256-thread block
LOSS_T = (0, 0, 1, 500, 999)


def loss_case(T: od.GaussianTables, mean_type: str, var_type: str) -> dict[str, Tensor]:
    """f32 inputs of the loss tests.  x0 in [-0.99, 0.99] with a few elements at exactly -1 and +1 (the open-ended bins), so nothing
    but those lies within 1e-3 of the +-0.999 thresholds.  The mean half is the exact target of its parameterisation for a noise
    estimate eps + 0.1 n: at t == 0 the predicted mean is then within a few 1e-3 of x0, i.e. within a fraction of the 1/255 bin at
    the predicted scale, and no probability comes near the 1e-12 clamp.  The variance half is uniform in [-1, 1] for learned_range and
    the log-variance that interpolation gives for learned."""
    tab = tables(T)
    t = torch.tensor(LOSS_T, dtype=torch.int32)
    x0 = 0.99 * synth.uniform("lvl.x0", LOSS_SHAPE, lo=-1.0, hi=1.0)
    flat = x0.view(-1)
    flat[::37] = 1.0
    flat[5::41] = -1.0
    eps = synth.normal("lvl.eps", LOSS_SHAPE)
    xt = od.ddpm_add_noise(T, x0, t, eps)
    rows = _rows(tab, t, xt, torch.float32)
    eps_hat = eps + 0.1 * synth.normal("lvl.dev", LOSS_SHAPE)
    x0_hat = x_start(eps_hat, xt, rows, "epsilon")
    o = {"epsilon": eps_hat, "xstart": x0_hat, "xprev": rows[2] * x0_hat + rows[3] * xt}[mean_type]
    v = synth.uniform("lvl.v", LOSS_SHAPE, lo=-1.0, hi=1.0)
    if var_type == "learned":
        v = log_variance(v, rows, "learned_range")
    return {"tab": tab, "t": t, "x0": x0, "eps": eps, "xt": xt, "pred": torch.cat([o, v], dim=1).contiguous()}
