"""Plain-torch restatement of the row head (`dl_gd_loss_rows_fwd` / `_bwd`) and a numpy restatement of the loss-second-moment
resampler (`dl_loss_history_update`, `dl_draw_timesteps`), imported by the test modules; not a conftest.

Training on the variational bound itself (L_vlb) with the timestep drawn by importance from a running second moment of the per-sample
loss is sec. 3.3 of Nichol & Dhariwal, "Improved Denoising Diffusion Probabilistic Models" (2021); the resampler is
`LossSecondMomentResampler` of their code base, written here from its description.  The reference has none of this.

Built on tests/learned_variance_common.py (the bound's formulas), tests/gd_param_common.py (the four parameterisations) and
tests/bpd_common.py (the comparison rule and the test inputs).  As there, every function takes the f32 [6, T] table the kernels read
and a `dtype`: torch.float32 evaluates in f32, torch.float64 evaluates the same formulas on the same f32 inputs without rounding.
"""

from __future__ import annotations

import numpy as np
import torch
from torch import Tensor

import bpd_common as bp
import gd_param_common as gp
import learned_variance_common as lv

LN2 = lv.LN2
LOSS_TYPES = ("mse", "vlb")
LEARNED = lv.VAR_TYPES


# ------------------------------------------------------------------------------------------------------------------ the row head
def bound_parts(tab: Tensor, pred: Tensor, x0: Tensor, xt: Tensor, t: Tensor, name: str, var_type: str, dtype,
                stop_gradient: bool) -> dict[str, Tensor]:
    """every intermediate of the bound's per-element term for a [B, 2C, ...] prediction whose mean output is read as `name`;
    stop_gradient detaches the predicted mean (the hybrid loss), otherwise the term is differentiable in both halves (L_vlb)"""
    rows = lv._rows(tab, t, xt, dtype)
    c1, c2, lv_q = rows[2], rows[3], rows[4]
    o, v = torch.chunk(pred, 2, dim=1)
    m_p = c1 * gp.x_start(o, xt, rows, name) + c2 * xt
    if stop_gradient:
        m_p = m_p.detach()
    m_q = c1 * x0 + c2 * xt
    lv_p = lv.log_variance(v, rows, var_type)
    kl = 0.5 * (-1.0 + lv_p - lv_q + torch.exp(lv_q - lv_p) + (m_q - m_p) ** 2 * torch.exp(-lv_p))
    c, s = x0 - m_p, torch.exp(-0.5 * lv_p)
    zp, zm = s * (c + 1.0 / 255.0), s * (c - 1.0 / 255.0)
    P, Q = lv.approx_cdf(zp), lv.approx_cdf(zm)
    lo, hi = x0 < -0.999, x0 > 0.999
    prob = torch.where(lo, P, torch.where(hi, 1.0 - Q, P - Q))
    nll = -torch.log(prob.clamp(min=1e-12))
    first = (t == 0).view(rows[0].shape).expand_as(kl)
    return {"term": torch.where(first, nll, kl), "prob": prob, "first": first, "lv_p": lv_p, "lv_q": lv_q, "m_p": m_p, "m_q": m_q, "zp": zp,
            "zm": zm, "s": s, "lo": lo, "hi": hi, "rows": rows}


def per_timestep(table: Tensor | None, t: Tensor, dtype) -> Tensor:
    return torch.ones(t.numel(), dtype=dtype) if table is None else table[t.long()].to(dtype)


def rows(tab: Tensor, pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, name: str, var_type: str, weight: Tensor | None,
         imp: Tensor | None, loss_type: str, vb_scale: float, dtype=torch.float64) -> dict[str, Tensor]:
    """what dl_gd_loss_rows_fwd writes: "mse_row", "vb_row" (learned variances), "total_row" [B] and "loss" [2] (or [1]),
    differentiable in `pred`; plus "prob" / "first" of the t == 0 term for the tests' input conditions"""
    pred = pred.to(dtype)
    eps, x0, xt = eps.to(dtype), x0.to(dtype), xt.to(dtype)
    r = lv._rows(tab, t, xt, dtype)
    fixed = var_type == "fixed"
    o = pred if fixed else torch.chunk(pred, 2, dim=1)[0]
    w, im = per_timestep(weight, t, dtype), per_timestep(imp, t, dtype)
    mse_row = ((gp.target(r, eps, x0, xt, name) - o) ** 2).flatten(1).mean(1)
    out = {"mse_row": mse_row}
    if fixed:
        assert loss_type == "mse"
        out["total_row"] = w * mse_row
        out["loss"] = (im * (w * mse_row)).mean().view(1)
        return out
    p = bound_parts(tab, pred, x0, xt, t, name, var_type, dtype, stop_gradient=loss_type == "mse")
    vb_row = p["term"].flatten(1).mean(1) / LN2
    out.update(vb_row=vb_row, prob=p["prob"], first=p["first"])
    out["total_row"] = vb_row if loss_type == "vlb" else w * mse_row + vb_scale * vb_row
    out["loss"] = torch.stack([(im * (w * mse_row)).mean(), (im * vb_row).mean()])
    return out


def mean_output_derivative(rows_, name: str) -> Tensor:
    """d m_p / d o of the four parameterisations, m_p = c1 x_start(o) + c2 xt.  epsilon: -c1 sqrt(1 - ab) / sqrt_ab, the coefficient
    `x_start` multiplies o by, which is -c1 sqrt(1 / ab - 1) up to the f32 rounding of the two table rows (sqrt_ab^2 is ab to 2^-23)"""
    sab, ab, c1 = rows_[0], rows_[1], rows_[2]
    if name == "epsilon":
        return -c1 * ((1.0 - ab).sqrt() / sab)
    if name == "xstart":
        return c1
    if name == "xprev":
        return torch.ones_like(c1)
    if name == "v":
        return -c1 * (1.0 - ab).sqrt()
    raise ValueError(name)


def term_derivative(p: dict[str, Tensor], name: str) -> Tensor:
    """d term / d o, written out by hand: d term / d m_p = -(m_q - m_p) exp(-lv_p) for t > 0; for t == 0 through the two CDF
    arguments (d z / d m_p = -exp(-lv_p / 2)), zero where the 1e-12 clamp is active"""
    d_kl = -(p["m_q"] - p["m_p"]) * torch.exp(-p["lv_p"])
    dP, dQ, s = lv.approx_cdf_grad(p["zp"]), lv.approx_cdf_grad(p["zm"]), p["s"]
    dprob = torch.where(p["lo"], dP * -s, torch.where(p["hi"], dQ * s, (dP - dQ) * -s))
    d_nll = torch.where(p["prob"] > 1e-12, -dprob / p["prob"], torch.zeros_like(dprob))
    return torch.where(p["first"], d_nll, d_kl) * mean_output_derivative(p["rows"], name)


def rows_backward(tab, pred, eps, x0, xt, t, name, var_type, weight, imp, loss_type, g_mse: float = 1.0, g_vb: float = 1.0,
                  dtype=torch.float64) -> Tensor:
    """d(g_mse loss[0] + g_vb loss[1]) / d pred, written out by hand: what dl_gd_loss_rows_bwd computes"""
    with torch.no_grad():
        pred = pred.to(dtype)
        eps_, x0_, xt_ = eps.to(dtype), x0.to(dtype), xt.to(dtype)
        r = lv._rows(tab, t, xt_, dtype)
        fixed = var_type == "fixed"
        o = pred if fixed else torch.chunk(pred, 2, dim=1)[0]
        n = o.numel()
        shape = r[0].shape
        w, im = per_timestep(weight, t, dtype).view(shape), per_timestep(imp, t, dtype).view(shape)
        d_o = g_mse * im * w * 2.0 * (o - gp.target(r, eps_, x0_, xt_, name)) / n
        if fixed:
            return d_o
        p = bound_parts(tab, pred, x0_, xt_, t, name, var_type, dtype, stop_gradient=True)
        lv_p, lv_q = p["lv_p"], p["lv_q"]
        rr, q = torch.exp(lv_q - lv_p), (p["m_q"] - p["m_p"]) ** 2 * torch.exp(-lv_p)
        d_kl = 0.5 * (1.0 - rr - q)
        zp, zm = p["zp"], p["zm"]
        dP, dQ = lv.approx_cdf_grad(zp) * (-0.5 * zp), lv.approx_cdf_grad(zm) * (-0.5 * zm)  # d z / d lv_p = -z / 2
        dprob = torch.where(p["lo"], dP, torch.where(p["hi"], -dQ, dP - dQ))
        d_nll = torch.where(p["prob"] > 1e-12, -dprob / p["prob"], torch.zeros_like(dprob))
        d_lv = torch.where(p["first"], d_nll, d_kl)
        dlv_dv = torch.ones_like(lv_q) if var_type == "learned" else 0.5 * (r[5].log() - lv_q)
        cv = g_vb * im / (n * LN2)
        d_v = cv * d_lv * dlv_dv
        if loss_type == "vlb":
            d_o = d_o + cv * term_derivative(p, name)
        return torch.cat([d_o, d_v], dim=1)


def check_inputs(c: dict[str, Tensor], ref: dict[str, Tensor]) -> None:
    """the conditions the comparisons rest on, on the f64 side: no t == 0 probability near the 1e-12 clamp, nothing but the elements
    at exactly +-1 near the bin thresholds"""
    x0 = c["x0"]
    if "prob" in ref:
        assert float(ref["prob"].detach()[ref["first"]].min()) > 10 * 1e-12
    assert bool(((x0.abs() - 0.999).abs() > 1e-3)[x0.abs() != 1.0].all())


VAR_TABLE = {"fixed": "fixed_small", "learned": "learned", "learned_range": "learned_range"}  # gd_param_common's name -> bpd_common's
CHAINS = {"t8": 8, "r20": 20, "full": 1000}


def chain(name: str):
    """"t8" / "r20": bpd_common's respaced chains; "full": the 1000-step one.  t = 0, 0, 1, T-2, T-1"""
    if name != "full":
        return bp.chain(name)
    T = bp.od.GaussianTables(1000)
    return T, torch.tensor([0, 0, 1, 998, 999], dtype=torch.int32)


def imp_table(T: int) -> Tensor:
    """an importance table a sampling distribution could give: f32 [T], positive, between 0.4 and 2.7, no two neighbours equal"""
    i = torch.arange(T, dtype=torch.float64)
    return (0.4 + 2.3 * ((i * 0.6180339887498949) % 1.0)).float()


# ------------------------------------------------------------------------------------------------------------------ the resampler
class Resampler:
    """IDDPM's LossSecondMomentResampler: a history of the last H losses of every timestep, filled in array order; until every
    timestep has H of them the distribution is uniform, afterwards p = sqrt(mean_h hist^2), normalised, times 1 - uniform_prob,
    plus uniform_prob / T.  The history holds f32 values (the losses are f32); `tables(dtype)` forms p, imp = 1 / (T p) and the
    cumulative distribution from it in the given numpy dtype."""

    def __init__(self, T: int, H: int = 10, uniform_prob: float = 0.001) -> None:
        self.T, self.H, self.uniform_prob = T, H, uniform_prob
        self.hist = np.zeros((T, H), dtype=np.float32)
        self.count = np.zeros(T, dtype=np.int32)

    def update(self, ts, losses) -> None:
        for t, l in zip(np.asarray(ts).tolist(), np.asarray(losses, dtype=np.float32).tolist()):
            if self.count[t] == self.H:
                self.hist[t, :-1] = self.hist[t, 1:]
                self.hist[t, -1] = l
            else:
                self.hist[t, self.count[t]] = l
                self.count[t] += 1

    def warmed_up(self) -> bool:
        return bool((self.count == self.H).all())

    def tables(self, dtype=np.float64) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        T = self.T
        if self.warmed_up():
            w = np.sqrt(np.mean(self.hist.astype(dtype) ** 2, axis=-1, dtype=dtype))
            w = w / w.sum(dtype=dtype)
            p = (w * dtype(1.0 - dtype(self.uniform_prob)) + dtype(self.uniform_prob) / dtype(T)).astype(dtype)
        else:
            p = np.full(T, dtype(1.0) / dtype(T), dtype=dtype)
        imp = (dtype(1.0) / (dtype(T) * p)).astype(dtype)
        cdf = np.cumsum(p, dtype=dtype)
        cdf[-1] = 1.0
        return p, imp, cdf


def draw(cdf: np.ndarray, u: np.ndarray) -> np.ndarray:
    """the first index with cdf[i] > u"""
    return np.searchsorted(cdf, u, side="right")
