"""Plain-torch restatement of the four parameterisations of a DDPM denoiser's mean output, of the loss that trains each of them and
of the v-prediction sampler steps (imported by the test modules; not a conftest).

Targets: epsilon, x0 and the posterior mean are the reference's three `mean_type`s (samplers/gaussian_diffusion/ddpm.py:87-174); v is
Salimans & Ho, "Progressive Distillation for Fast Sampling of Diffusion Models" (2022): v = sqrt(ab) eps - sqrt(1 - ab) x0, hence
x0 = sqrt(ab) xt - sqrt(1 - ab) v.  Loss: (1 / n) sum w[t] (target - o)^2 and, for a learned-variance [B, 2C, ...] prediction, the
variational bound of tests/learned_variance_common.py with the predicted mean derived from o by the same parameterisation and frozen.
The reference has neither the loss (gaussian_diffusion.py:267 leaves it as a TODO) nor v.  Weights: Min-SNR-gamma of Hang et al.,
"Efficient Diffusion Training via Min-SNR Weighting Strategy" (2023).

As in learned_variance_common, every function takes `tab`, the f32 [6, T] table the kernels read, and a `dtype`: torch.float32
evaluates as the reference would, torch.float64 evaluates the same formulas on the same f32 inputs without rounding.
"""

from __future__ import annotations

import torch
from torch import Tensor

import learned_variance_common as lv
from oracle import diffusion as od
from oracle import synth

TARGETS = ("epsilon", "xstart", "xprev", "v")
REFERENCE_TARGETS = ("epsilon", "xstart", "xprev")
VAR_TYPES = ("fixed", "learned", "learned_range")
STEP_KEYS = lv.STEP_KEYS
CHAINS = {"full": (1000, (0, 0, 1, 500, 999)), "r50": (50, (0, 0, 1, 25, 49))}  # the chains of tests/golden/gd_targets.npz
FIXTURE_SHAPE = (5, 3, 8, 8)

_rows = lv._rows


def chain(name: str) -> tuple[od.GaussianTables, Tensor]:
    steps, ts = CHAINS[name]
    return od.GaussianTables(1000, n_steps=steps), torch.tensor(ts, dtype=torch.int32)


def fixture_inputs() -> tuple[Tensor, Tensor]:
    """the named draws tests/golden/make_gd_targets_golden.py feeds the reference"""
    return synth.uniform("gdt.x0", FIXTURE_SHAPE, lo=-1.0, hi=1.0), synth.normal("gdt.eps", FIXTURE_SHAPE)


def fixed_tables(T: od.GaussianTables) -> Tensor:
    """the [6, T] table of a fixed_small sampler: rows 4, 5 = posterior variance and its clipped log"""
    return torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.posterior_mean_coef1, T.posterior_mean_coef2, T.posterior_variance,
                        T.posterior_log_variance_clipped]).float()


def ddim_tables(T: od.GaussianTables) -> Tensor:
    return torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.alphas_bar_prev]).float()


# ------------------------------------------------------------------------------------------------------------------ targets, inverses
def target(rows, eps: Tensor, x0: Tensor, xt: Tensor, name: str) -> Tensor:
    sab, ab, c1, c2 = rows[:4]
    if name == "epsilon":
        return eps
    if name == "xstart":
        return x0
    if name == "xprev":
        return c1 * x0 + c2 * xt  # ddpm.py:156-174
    if name == "v":
        return sab * eps - (torch.ones_like(x0) - ab).sqrt() * x0
    raise ValueError(name)


def x_start(o: Tensor, xt: Tensor, rows, name: str) -> Tensor:
    if name == "v":
        return rows[0] * xt - (torch.ones_like(o) - rows[1]).sqrt() * o
    return lv.x_start(o, xt, rows, name)


def posterior_mean(rows, x0: Tensor, xt: Tensor) -> Tensor:
    return rows[2] * x0 + rows[3] * xt


# ------------------------------------------------------------------------------------------------------------------ min-SNR weights
def min_snr(alphas_bar: Tensor, name: str, gamma: float = 5.0) -> Tensor:
    """fp64 [T]; min(snr, gamma) is the weight of the x0 loss, and (x0 - x0_hat)^2 = (eps - eps_hat)^2 / snr = (v - v_hat)^2 / (snr + 1)"""
    ab = alphas_bar.double()
    snr = ab / (1 - ab)
    m = torch.minimum(snr, torch.full_like(snr, gamma))
    if name == "epsilon":
        return m / snr
    if name == "xstart":
        return m
    if name == "v":
        return m / (snr + 1)
    raise ValueError(f"min-SNR weighting is not defined for the target {name!r}")


# ------------------------------------------------------------------------------------------------------------------ loss
def _bound_pred(pred: Tensor, xt: Tensor, rows, name: str) -> Tensor:
    """the [B, 2C, ...] tensor whose "xstart" bound is the bound of `pred` under the parameterisation `name`: the mean half replaced by
    the x0 it stands for (a constant of the bound), the variance half left in the graph"""
    o, v = torch.chunk(pred, 2, dim=1)
    return torch.cat([x_start(o, xt, rows, name).detach(), v], dim=1)


def loss(tab: Tensor, pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, name: str, var_type: str,
         weight: Tensor | None = None, dtype=torch.float64) -> tuple[Tensor, Tensor | None]:
    """-> (weighted mse of the mean output, variational bound in bits / dim or None for fixed variances), differentiable in `pred`"""
    pred = pred.to(dtype)
    eps, x0, xt = eps.to(dtype), x0.to(dtype), xt.to(dtype)
    rows = _rows(tab, t, xt, dtype)
    o = pred if var_type == "fixed" else torch.chunk(pred, 2, dim=1)[0]
    w = torch.ones((), dtype=dtype) if weight is None else weight[t.long()].to(dtype).view(rows[0].shape)
    mse = (w * (target(rows, eps, x0, xt, name) - o) ** 2).mean()
    if var_type == "fixed":
        return mse, None
    return mse, lv.hybrid_parts(tab, _bound_pred(pred, xt, rows, name), eps, x0, xt, t, "xstart", var_type, dtype)["vb"]


def loss_backward(tab, pred, eps, x0, xt, t, name, var_type, weight=None, g_mse: float = 1.0, g_vb: float = 1.0,
                  dtype=torch.float64) -> Tensor:
    """d(g_mse * mse + g_vb * vb) / d pred, written out by hand: what the backward kernel computes"""
    with torch.no_grad():
        pred = pred.to(dtype)
        eps_, x0_, xt_ = eps.to(dtype), x0.to(dtype), xt.to(dtype)
        rows = _rows(tab, t, xt_, dtype)
        o = pred if var_type == "fixed" else torch.chunk(pred, 2, dim=1)[0]
        w = torch.ones((), dtype=dtype) if weight is None else weight[t.long()].to(dtype).view(rows[0].shape)
        d_o = g_mse * 2.0 * w * (o - target(rows, eps_, x0_, xt_, name)) / o.numel()
        if var_type == "fixed":
            return d_o
        C = o.shape[1]
        d_v = lv.hybrid_backward(tab, _bound_pred(pred, xt_, rows, name), eps, x0, xt, t, "xstart", var_type, g_mse=0.0, g_vb=g_vb,
                                 dtype=dtype)[:, C:]
        return torch.cat([d_o, d_v], dim=1)


# ------------------------------------------------------------------------------------------------------------------ loss test inputs
LOSS_CASES = {"small": ((5, 3, 8, 8), (0, 0, 1, 500, 999)),  # n = 960: not a multiple of the 256-thread block
              "two_blocks": ((3, 3, 23, 23), (0, 500, 999))}  # chw = 1587, n = 4761: two reduction blocks, sample boundaries inside one


def loss_case(T: od.GaussianTables, name: str, var_type: str, case: str = "small") -> dict[str, Tensor]:
    """f32 inputs of the loss tests, built as learned_variance_common.loss_case builds them: x0 in [-0.99, 0.99] with a few elements
    at exactly -1 and +1, the prediction the exact target of its parameterisation for a noise estimate eps + 0.1 n (so that no
    probability of the t == 0 term comes near the 1e-12 clamp), the variance half uniform in [-1, 1] for learned_range and the
    log-variance that interpolation gives for learned; fixed variances have the mean output alone."""
    shape, ts = LOSS_CASES[case]
    tab = lv.tables(T)
    t = torch.tensor(ts, dtype=torch.int32)
    x0 = 0.99 * synth.uniform(f"gdl.x0.{case}", shape, lo=-1.0, hi=1.0)
    flat = x0.view(-1)
    flat[::37] = 1.0
    flat[5::41] = -1.0
    eps = synth.normal(f"gdl.eps.{case}", shape)
    xt = od.ddpm_add_noise(T, x0, t, eps)
    rows = _rows(tab, t, xt, torch.float32)
    eps_hat = eps + 0.1 * synth.normal(f"gdl.dev.{case}", shape)
    o = target(rows, eps_hat, x_start(eps_hat, xt, rows, "epsilon"), xt, name)
    if var_type == "fixed":
        pred = o.contiguous()
    else:
        v = synth.uniform(f"gdl.v.{case}", shape, lo=-1.0, hi=1.0)
        if var_type == "learned":
            v = lv.log_variance(v, rows, "learned_range")
        pred = torch.cat([o, v], dim=1).contiguous()
    return {"tab": tab, "t": t, "x0": x0, "eps": eps, "xt": xt, "pred": pred}


def weightings(T: od.GaussianTables, name: str) -> dict[str, Tensor | None]:
    """the weight tables a loss test runs `name` with (f32 [T], as the kernel reads them); min-SNR has none for xprev"""
    out: dict[str, Tensor | None] = {"unweighted": None}
    if name != "xprev":
        out["min_snr"] = min_snr(T.alphas_bar, name).float()
    return out


# ------------------------------------------------------------------------------------------------------------------ v steps
def ddpm_step_v(tab: Tensor, pred: Tensor, t: Tensor, xt: Tensor, noise: Tensor, var_type: str, clamp_x: bool = False,
                dtype=torch.float32) -> dict[str, Tensor]:
    """DDPM.step (ddpm.py:330-363) on a v prediction; tab = fixed_tables(T) for "fixed", learned_variance_common.tables(T) otherwise"""
    pred, xt, noise = pred.to(dtype), xt.to(dtype), noise.to(dtype)
    rows = _rows(tab, t, xt, dtype)
    if var_type == "fixed":
        o, var, lvar = pred, rows[4].expand_as(xt), rows[5].expand_as(xt)
    else:
        o, v = torch.chunk(pred, 2, dim=1)
        lvar = lv.log_variance(v, rows, var_type)
        var = lvar.exp()
    x0 = x_start(o, xt, rows, "v")
    if clamp_x:
        x0 = x0.clamp(-1, 1)
    mean = posterior_mean(rows, x0, xt)
    mask = (t > 0).to(dtype).view(rows[0].shape)
    x_prev = mean + mask * noise * torch.exp(0.5 * lvar)
    vs = var.clamp_min(1e-20)
    logprob = (-((x_prev - mean) ** 2) / (2.0 * vs) - torch.log(2 * torch.pi * vs) * 0.5) * mask
    return {"x_prev": x_prev, "estimated_x0": x0, "x_prev_mean": mean, "x_prev_std": vs.sqrt(), "logprob": logprob}


def ddim_step(tab3: Tensor, x0: Tensor, t: Tensor, xt: Tensor, noise: Tensor, eta: float, dtype=torch.float32) -> dict[str, Tensor]:
    """DDIM.step (ddim.py:68-103) from the estimated x0 on; tab3 = ddim_tables(T)"""
    x0, xt, noise = x0.to(dtype), xt.to(dtype), noise.to(dtype)
    shape = (-1,) + (1,) * (xt.dim() - 1)
    sab, ab, abp = (tab3[k][t.long()].to(dtype).view(shape) for k in range(3))
    one = torch.ones_like(xt)
    eps = ((1 / sab) * xt - x0) / (1 / ab - 1).sqrt()
    sigma = eta * ((one - abp) / (one - ab)).sqrt() * (one - ab / abp).sqrt()
    mean = x0 * abp.sqrt() + (one - abp - sigma**2).sqrt() * eps
    mask = (t > 0).to(dtype).view(shape)
    x_prev = mean + mask * sigma * noise
    out = {"x_prev": x_prev, "estimated_x0": x0, "x_prev_mean": mean}
    if eta > 0:
        out["x_prev_std"] = sigma
        out["logprob"] = -((x_prev - mean) ** 2 / (2 * sigma**2) + torch.log(sigma) + 0.5 * torch.log(torch.tensor(2 * torch.pi, dtype=dtype)))
    return out


def ddim_step_v(tab3: Tensor, pred: Tensor, t: Tensor, xt: Tensor, noise: Tensor, eta: float, var_type: str, clamp_x: bool = False,
                dtype=torch.float32) -> dict[str, Tensor]:
    """the variance half of a learned-variance prediction is discarded (ddim.py:89)"""
    o = (pred if var_type == "fixed" else torch.chunk(pred, 2, dim=1)[0]).to(dtype)
    shape = (-1,) + (1,) * (xt.dim() - 1)
    rows = [tab3[k][t.long()].to(dtype).view(shape) for k in range(2)]
    x0 = x_start(o, xt.to(dtype), rows, "v")
    if clamp_x:
        x0 = x0.clamp(-1, 1)
    return ddim_step(tab3, x0, t, xt, noise, eta, dtype)
