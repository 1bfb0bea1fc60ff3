"""Plain-torch restatement of the ODE likelihood of a rectified-flow model (`Flow.calc_nll_loop`) and of the three kernels under it
(`dl_patch_embed_dgrad`, `dl_hutchinson_step`, `dl_normal_nll_rows`), with their per-element error bounds.

Written from the formulas, not from the product code.  With z_t = (1 - t) x0 + t eps data sits at t = 0 and noise at t = 1; dx/dt =
v(x, t) is integrated upward over an ascending grid and
    log p0(x) = log N(x1; 0, I) + integral_0^1 div v dt,      div v ~ sum(eps * J^T eps)   (Hutchinson; Grathwohl et al. 2019).
Bounds have the project's form k * 2^-24 * (sum of absolute terms) + 2^-149: k counts the f32 roundings on the longest path to the
element (a sum of n terms in ANY order: n - 1 additions and one rounding per product, so n + 1 covers products, adds and one scale).
"""

from __future__ import annotations

import math

import torch
from torch import Tensor

from multistep_common import M as DATA_MEAN
from multistep_common import S as DATA_STD

U, TINY = 2.0**-24, 2.0**-149
LN2 = math.log(2.0)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
SHARE = 4096  # elements of a row one workgroup sums (dl_mse_loss_partials)


# ------------------------------------------------------------------------------------------------------------------ the loop
def jt_eps(field, x: Tensor, t: float, eps: Tensor) -> tuple[Tensor, Tensor]:
    """(v, J^T eps) of v = field(x, t) by autograd"""
    with torch.enable_grad():
        xin = x.detach().requires_grad_(True)
        v = field(xin, t)
        (g,) = torch.autograd.grad(v, xin, eps)
    return v.detach(), g.detach()


def nll_loop(field, x0: Tensor, timesteps: list[float], method: str, probes: Tensor, dequant_noise: Tensor | None = None,
             pixel: bool = True, dtype=torch.float64) -> dict[str, Tensor]:
    """field(x [R, ...], t) -> v; timesteps: the diffusion's grid in any order; probes [K, B, ...]; dequant_noise [B, ...] in [0, 1)
    or None (no dequantisation).  Returns the result dict of calc_nll_loop in `dtype`."""
    x0 = x0.to(dtype)
    if dequant_noise is not None:
        x0 = x0 + (dequant_noise.to(dtype) - 0.5) * (2.0 / 255.0)
    K, B = probes.shape[0], x0.shape[0]
    tail = tuple(x0.shape[1:])
    n_el = x0[0].numel()
    x = x0.repeat(K, *([1] * len(tail)))
    eps = probes.to(dtype).reshape(K * B, *tail)
    grid = sorted(float(t) for t in timesteps)
    terms, weights = [], []
    for t0, t1 in zip(grid[:-1], grid[1:]):
        h = t1 - t0
        v1, g1 = jt_eps(field, x, t0, eps)
        terms.append((g1 * eps).flatten(1).sum(1) / n_el)
        if method == "euler":
            x = x + h * v1
            weights.append(h)
            continue
        assert method == "heun"
        v2, g2 = jt_eps(field, x + h * v1, t1, eps)
        terms.append((g2 * eps).flatten(1).sum(1) / n_el)
        x = x + 0.5 * h * (v1 + v2)
        weights += [0.5 * h, 0.5 * h]
    table = torch.stack(terms, 1).view(K, B, len(terms)).mean(0)
    div = (table * torch.tensor(weights, dtype=dtype)).sum(1)
    x1 = x[:B]
    prior = 0.5 * (x1 * x1).flatten(1).mean(1) + HALF_LOG_2PI
    out = {"nll": prior - div, "prior": prior, "div": div, "div_terms": table, "x1": x1}
    if pixel:
        out["total_bpd"] = out["nll"] / LN2 + math.log2(127.5)
    return out


def gaussian_nll(x: Tensor) -> Tensor:
    """exact -log p(x) / D_el of the closed-form model of multistep_common (every element N(M, S^2) independently), nats, fp64"""
    x = x.double()
    return (0.5 * ((x - DATA_MEAN) / DATA_STD) ** 2 + math.log(DATA_STD) + HALF_LOG_2PI).flatten(1).mean(1)


def rademacher(shape, seed: int) -> Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2, shape, generator=g).double() * 2.0 - 1.0


# ------------------------------------------------------------------------------------------------------------------ dl_patch_embed_dgrad
def _weight_as(w: Tensor, C: int, p: int, order: str) -> Tensor:
    """w [D, C p p] read as [D, C, p1, p2] in feature order "cpp" (c p1 p2: the kernel's), "swap" ((p2 p1) exchanged) or "ppc" (p1 p2 c)"""
    D = w.shape[0]
    if order == "cpp":
        return w.view(D, C, p, p)
    if order == "swap":
        return w.view(D, C, p, p).transpose(2, 3)
    assert order == "ppc"
    return w.view(D, p, p, C).permute(0, 3, 1, 2)


def patch_embed_dgrad(dtok: Tensor, w: Tensor, B: int, C: int, H: int, W: int, p: int, order: str = "cpp") -> tuple[Tensor, Tensor]:
    """dimg[b, c, gy p + p1, gx p + p2] = sum_d dtok[(b, gy, gx), d] w[d, (c p + p1) p + p2] in fp64, and the same sum over the
    absolute values of its terms.  dtok [M, >= D] (padding columns ignored), w [D, C p p]"""
    D = w.shape[0]
    gh, gw = H // p, W // p
    t = dtok[: B * gh * gw, :D].double().view(B, gh, gw, D)
    wk = _weight_as(w.double(), C, p, order)
    img = torch.einsum("bghd,dcij->bcgihj", t, wk).reshape(B, C, H, W)
    mag = torch.einsum("bghd,dcij->bcgihj", t.abs(), wk.abs()).reshape(B, C, H, W)
    return img, mag


def patch_embed_dgrad_bound(mag: Tensor, D: int) -> Tensor:
    return (D + 1) * U * mag + TINY


# ------------------------------------------------------------------------------------------------------------------ the row kernels
def hutchinson_step(x, v, v0, a: float, b: float, g: Tensor, eps: Tensor, scale: float):
    """-> (x_out, its bound, row sums, their bound): x_out = x + a v + b v0 (None without x); sums[r] = scale * sum(g[r] * eps[r]).
    a, b and scale enter as the f32 values the kernel receives"""
    a, b, scale = (float(torch.tensor(c, dtype=torch.float32)) for c in (a, b, scale))
    prod = g.double().flatten(1) * eps.double().flatten(1)
    n = prod.shape[1]
    sums, smag = scale * prod.sum(1), abs(scale) * prod.abs().sum(1)
    xo = xb = None
    if x is not None:
        xo = x.double() + a * v.double()
        mag = x.double().abs() + abs(a) * v.double().abs()
        if v0 is not None:
            xo = xo + b * v0.double()
            mag = mag + abs(b) * v0.double().abs()
        xb = 4 * U * mag + TINY
    return xo, xb, sums, (n + 2) * U * smag + TINY


def normal_nll_rows(x: Tensor) -> tuple[Tensor, Tensor]:
    """-> (0.5 mean(x^2) + 0.5 log(2 pi) per row in fp64, its bound)"""
    sq = x.double().flatten(1) ** 2
    n = sq.shape[1]
    val = 0.5 * sq.mean(1) + HALF_LOG_2PI
    return val, (n + 2) * U * val.abs() + TINY
