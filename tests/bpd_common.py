"""Plain-torch restatement of the variational bound in bits per dimension, per (sample, timestep) row, as `dl_vb_terms` and
`dl_prior_bpd` evaluate it (imported by the test modules; not a conftest).

The bound is L_vlb of Nichol & Dhariwal, "Improved Denoising Diffusion Probabilistic Models" (2021), eq. 4-7, evaluated the way
`calc_bpd_loop` of their code base does: for every timestep the KL between the posterior q(x_{t-1} | x_t, x_0) and the model's
p(x_{t-1} | x_t) (t > 0) or the discretised-Gaussian negative log-likelihood of x_0 (t == 0), the squared error of the predicted x_0,
the squared error of the eps derived from it, and the prior term KL(q(x_T | x_0) || N(0, I)).  The reference has none of this.

Built on tests/learned_variance_common.py (`hybrid_parts` gives the bound's intermediates for an "xstart" prediction with a learned
log-variance; a fixed variance enters as the log-variance the sampler's table holds) and tests/gd_param_common.py (`x_start` of the four
parameterisations).  As there, every function takes the [6, T] table the kernels read and a `dtype`: torch.float32 evaluates in f32,
torch.float64 evaluates the same formulas on the same inputs without rounding.
"""

from __future__ import annotations

import torch
from torch import Tensor

import gd_param_common as gp
import learned_variance_common as lv
from oracle import diffusion as od
from oracle import synth

MEAN_TYPES = gp.TARGETS  # epsilon, xstart, xprev, v
VAR_TYPES = ("fixed_small", "fixed_large", "learned", "learned_range")
KEYS = ("vb", "xstart_mse", "mse")
LN2 = lv.LN2


def tables(T: od.GaussianTables, var_type: str, dtype=torch.float32) -> tuple[Tensor, Tensor]:
    """(the [6, T] table DDPM._tables builds for `var_type`, posterior_log_variance_clipped [T]); dtype float32 is what the kernels
    read, float64 keeps the schedule as it is"""
    plvc = T.posterior_log_variance_clipped
    if var_type == "fixed_small":
        r4, r5 = T.posterior_variance, plvc
    elif var_type == "fixed_large":
        r4 = torch.cat([T.posterior_variance[1:2], T.betas[1:]])
        r5 = torch.log(r4)
    else:
        r4, r5 = plvc, T.betas
    tab = torch.stack([T.sqrt_alphas_bar, T.alphas_bar, T.posterior_mean_coef1, T.posterior_mean_coef2, r4, r5])
    return tab.to(dtype), plvc.to(dtype)


def terms(tab: Tensor, lv_q: Tensor, pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, mean_type: str, var_type: str,
          clip_denoised: bool, dtype=torch.float64) -> dict[str, Tensor]:
    """-> "vb", "xstart_mse", "mse" [R] (one value per row of the batch dimension) and, for the tests' input conditions, "prob" (the
    t == 0 bin probability of every element) and "first" (t == 0, per element)"""
    pred, eps, x0, xt = pred.to(dtype), eps.to(dtype), x0.to(dtype), xt.to(dtype)
    rows = lv._rows(tab, t, xt, dtype)
    if var_type in lv.VAR_TYPES:
        o, v = torch.chunk(pred, 2, dim=1)
        how = var_type
    else:  # the model's log-variance is the table's row 5: a "learned" log-variance that does not depend on the prediction
        o, v, how = pred, rows[5].expand_as(xt), "learned"
    x0_pred = gp.x_start(o, xt, rows, mean_type)
    if clip_denoised:
        x0_pred = x0_pred.clamp(-1, 1)
    tab_q = tab.clone()
    tab_q[4] = lv_q  # hybrid_parts reads lv_q from row 4 (already there for learned variances)
    p = lv.hybrid_parts(tab_q, torch.cat([x0_pred, v], dim=1), eps, x0, xt, t, "xstart", how, dtype)
    lv_p, q = p["lv_p"], p["lv_q"]
    kl = 0.5 * (-1.0 + lv_p - q + torch.exp(q - lv_p) + (p["m_q"] - p["m_p"]) ** 2 * torch.exp(-lv_p))
    nll = -torch.log(p["prob"].clamp(min=1e-12))
    term = torch.where(p["first"], nll, kl)
    sab, ab = rows[0], rows[1]
    eps_pred = ((1.0 / sab) * xt - x0_pred) / (1.0 / ab - 1.0).sqrt()  # ddpm.py:324-326
    return {"vb": term.flatten(1).mean(1) / LN2, "xstart_mse": ((x0 - x0_pred) ** 2).flatten(1).mean(1),
            "mse": ((eps - eps_pred) ** 2).flatten(1).mean(1), "prob": p["prob"], "first": p["first"]}


def prior(x0: Tensor, alphas_bar_last: float, log_one_minus_ab: float, dtype=torch.float64) -> Tensor:
    """KL(q(x_T | x0) || N(0, I)) per row in bits per dimension, from the two scalars as given (the kernel gets their f32 values)"""
    x0 = x0.to(dtype)
    ab, l = torch.tensor(alphas_bar_last, dtype=dtype), torch.tensor(log_one_minus_ab, dtype=dtype)
    return (0.5 * (-1.0 - l + torch.exp(l) + ab * x0 * x0)).flatten(1).mean(1) / LN2


def f32(x: float) -> float:
    """the value a C `float` argument carries"""
    return float(torch.tensor(x, dtype=torch.float32))


def bound(got: Tensor, ref: Tensor, cpu32: Tensor) -> tuple[float, float, float]:
    """the suite's rule for an f32 kernel against f64 (tests/test_learned_variance_gpu.py): -> (worst |got - ref| over the rows, the f32
    CPU evaluation's worst error, the bound 2 * that + 3e-6 * max|ref|)"""
    ref = ref.double()
    e32 = float((cpu32.double() - ref).abs().max())
    return float((got.double().cpu() - ref).abs().max()), e32, 2 * e32 + 3e-6 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------------------------ test inputs
ROWS = 5


def chain(name: str) -> tuple[od.GaussianTables, Tensor]:
    """"t8": the 8-step linear chain, "r20": the 20-step one -- the 1000-step linear schedule respaced, which is how this project
    makes a short chain (`set_steps(8)`; the linear formula itself at 8 steps has betas above 1).  t = 0, 0, 1, T-2, T-1"""
    T = od.GaussianTables(1000, n_steps=8 if name == "t8" else 20)
    n = T.betas.numel()
    return T, torch.tensor([0, 0, 1, n - 2, n - 1], dtype=torch.int32)


def case(T: od.GaussianTables, t: Tensor, chw: int, mean_type: str, var_type: str, tag: str = "") -> dict[str, Tensor]:
    """f32 inputs [ROWS, chw] of the kernel tests, built as learned_variance_common.loss_case builds them: x0 in [-0.99, 0.99] with a
    few elements at exactly -1 and +1 (the open-ended bins), the prediction the exact target of its parameterisation for a noise
    estimate eps + 0.1 n (so that no probability of the t == 0 term comes near the 1e-12 clamp), the variance half uniform in [-1, 1]
    for learned_range and the log-variance that interpolation gives for learned; fixed variances have the mean output alone."""
    shape = (ROWS, chw)
    tab, lv_q = tables(T, var_type)
    x0 = 0.99 * synth.uniform(f"bpd.x0.{chw}{tag}", shape, lo=-1.0, hi=1.0)
    flat = x0.view(-1)
    flat[::37] = 1.0
    flat[5::41] = -1.0
    eps = synth.normal(f"bpd.eps.{chw}{tag}", shape)
    xt = od.ddpm_add_noise(T, x0, t, eps)
    rows = lv._rows(tab, t, xt, torch.float32)
    eps_hat = eps + 0.1 * synth.normal(f"bpd.dev.{chw}{tag}", shape)
    o = gp.target(rows, eps_hat, gp.x_start(eps_hat, xt, rows, "epsilon"), xt, mean_type)
    if var_type in lv.VAR_TYPES:
        v = synth.uniform(f"bpd.v.{chw}{tag}", shape, lo=-1.0, hi=1.0)
        if var_type == "learned":
            v = lv.log_variance(v, rows, "learned_range")
        pred = torch.cat([o, v], dim=1).contiguous()
    else:
        pred = o.contiguous()
    return {"tab": tab, "lv_q": lv_q, "t": t, "x0": x0, "eps": eps, "xt": xt, "pred": pred}
