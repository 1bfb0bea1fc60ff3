"""Tensor-level wrappers over the C ABI (``include/diffulab_hip.h``).

Torch is plumbing only here: it owns the device buffers and the stream; every computation below is a
hand-written HIP kernel in ``libdiffulab_hip.so``.  All functions write into caller-provided outputs
(so the engines can run allocation-free / graph-capturable) and return the output for convenience.
There is no fallback path: a missing library or a CPU tensor raises.
"""

from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch
from torch import Tensor

from ._lib import lib
from . import tuning

BF16, F32 = 0, 1
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
LOSS_FLOW, LOSS_EPS = 0, 1
MEAN_TYPES = {"epsilon": 0, "xstart": 1, "xprev": 2, "v": 3}  # "v": the gd_loss_* / vb_terms / *_step_v / *_step_g / x0_threshold entry points only
VAR_MODES = {"learned": 0, "learned_range": 1}
VAR_FIXED = -1
PATCH_CPP, PATCH_PPC = 0, 1


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _s() -> int:
    """the caller's current HIP stream (raw handle)"""
    if _raw_stream is not None:  # 0.1 us instead of 2.6 us for constructing a torch Stream object per launch
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _p(t: Tensor | None) -> int | None:
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("diffulab_amd ops need device tensors (no CPU fallback exists)")
    return t.data_ptr()


_LIB = None


def _call(name: str, *args) -> None:
    global _LIB
    if _LIB is None:
        _LIB = lib()
    _LIB.call(name, *args)
    if _REC is not None:
        _REC.calls.append((_LIB._fns[name][0], args))


# ------------------------------------------------------------------ launch plans
class LaunchPlan:
    """One engine pass (a training forward, a backward) as a flat list of C calls with their final arguments, recorded while the
    pass runs once and re-issued by `replay()` afterwards: the launch sequence of an engine is static for a given input shape, and
    on the host-bound configurations (the UNet at its configured batch: 716 launches, ~24 us of Python per launch against ~5 us
    inside the HIP runtime) the step time IS the time the host needs to walk the engine's Python.  (A hipGraph of the same step
    replays SLOWER than the eager launches on this runtime: DESIGN.md section 6, round 6.)  What makes a pass recordable: every
    action is a C-ABI call with plain arguments -- kernels, `dl_memset_zero`, `dl_stream_wait_stream` -- or a registered host
    closure (`rec`); every buffer the calls name is kept alive by the plan (`keep`); per-call inputs live in static buffers the
    caller copies into before a replay."""

    __slots__ = ("calls", "held", "state", "inputs", "out", "bwd", "ctx")

    def __init__(self) -> None:
        self.calls: list = []
        self.held: list = []
        self.state = self.inputs = self.out = self.bwd = None
        self.ctx = ()

    def replay(self) -> None:
        for fn, args in self.calls:
            if fn(*args):
                raise RuntimeError(f"launch plan: a replayed call failed: {lib().cdll.dl_last_error().decode()}")


_REC: LaunchPlan | None = None


class recording:
    """``with ops.recording(plan):`` every ops call inside is executed AND appended to the plan"""

    def __init__(self, plan: LaunchPlan) -> None:
        self.plan = plan

    def __enter__(self) -> LaunchPlan:
        global _REC
        self.prev, _REC = _REC, self.plan
        return self.plan

    def __exit__(self, *exc) -> None:
        global _REC
        _REC = self.prev


def is_recording() -> bool:
    return _REC is not None


def keep(obj):
    """the plan being recorded (if any) holds a reference to `obj` (a buffer or table whose raw address a recorded call carries)"""
    if _REC is not None:
        _REC.held.append(obj)
    return obj


def rec(fn) -> None:
    """run the host closure `fn` now; a plan being recorded re-runs it at the same position of every replay"""
    fn()
    if _REC is not None:
        def again(f=fn):
            f()
            return 0
        _REC.calls.append((again, ()))


def zero_(t: Tensor) -> Tensor:
    """t.zero_() as a C call on the current stream (recordable); t contiguous"""
    assert t.is_contiguous()
    _call("dl_memset_zero", _p(t), t.numel() * t.element_size(), _s())
    return t


def stream_wait(waiter: int, waited: int) -> None:
    """raw stream handles: what is queued on `waited` so far happens before what is queued on `waiter` from now on"""
    if waiter != waited:
        _call("dl_stream_wait_stream", waiter, waited)


# ------------------------------------------------------------------ diffusion heads
def flow_add_noise(x: Tensor, noise: Tensor, t: Tensor, out: Tensor | None = None) -> Tensor:
    out = torch.empty_like(x) if out is None else out
    B = x.shape[0]
    _call("dl_flow_add_noise", _p(x), _p(noise), _p(t), _p(out), B, x.numel() // B, _s())
    return out


def ddpm_add_noise(x: Tensor, noise: Tensor, t: Tensor, sqrt_ab: Tensor, ab: Tensor, out: Tensor | None = None) -> Tensor:
    out = torch.empty_like(x) if out is None else out
    B = x.shape[0]
    _call("dl_ddpm_add_noise", _p(x), _p(noise), _p(t), _p(sqrt_ab), _p(ab), _p(out), B, x.numel() // B, _s())
    return out


def mse_loss_fwd(pred: Tensor, a: Tensor, b: Tensor | None, mode: int) -> Tensor:
    n = pred.numel()
    npart = lib().call("dl_mse_loss_partials", n)
    partial = torch.empty(npart, device=pred.device, dtype=torch.float32)
    loss = torch.empty((), device=pred.device, dtype=torch.float32)
    _call("dl_mse_loss_fwd", _p(pred), _p(a), _p(b), _p(partial), _p(loss), n, mode, _s())
    return loss


def mse_loss_bwd(pred: Tensor, a: Tensor, b: Tensor | None, gscale: float, mode: int, out: Tensor | None = None,
                 gscale_dev: Tensor | None = None) -> Tensor:
    out = torch.empty_like(pred) if out is None else out
    _call("dl_mse_loss_bwd", _p(pred), _p(a), _p(b), float(gscale), _p(gscale_dev), _p(out), pred.numel(), mode, _s())
    return out


def vlb_loss_fwd(pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, tables: Tensor, mean_type: int, var_mode: int,
                 out: Tensor | None = None) -> Tensor:
    """-> f32 [2] = (mse of the mean half, variational bound in bits / dim) of a [B, 2C, ...] prediction (dl_vlb_loss_fwd)"""
    B, n = xt.shape[0], xt.numel()
    assert pred.numel() == 2 * n and eps.numel() == n and x0.numel() == n
    partial = torch.empty(2 * lib().call("dl_mse_loss_partials", n), device=pred.device, dtype=torch.float32)
    out = torch.empty(2, device=pred.device, dtype=torch.float32) if out is None else out
    _call("dl_vlb_loss_fwd", _p(pred), _p(eps), _p(x0), _p(xt), _p(t), _p(tables), tables.shape[1], mean_type, var_mode,
          _p(partial), _p(out), B, n // B, _s())
    return out


def vlb_loss_bwd(pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, tables: Tensor, mean_type: int, var_mode: int,
                 g_mse: Tensor | None, g_vb: Tensor | None, out: Tensor | None = None) -> Tensor:
    """dpred [B, 2C, ...] in one pass; g_mse / g_vb: the two scalars' upstream gradients as device scalars (None = 1)"""
    B, n = xt.shape[0], xt.numel()
    assert pred.numel() == 2 * n and eps.numel() == n and x0.numel() == n
    out = torch.empty_like(pred) if out is None else out
    _call("dl_vlb_loss_bwd", _p(pred), _p(eps), _p(x0), _p(xt), _p(t), _p(tables), tables.shape[1], mean_type, var_mode,
          _p(g_mse), _p(g_vb), _p(out), B, n // B, _s())
    return out


def gd_loss_fwd(pred: Tensor, eps: Tensor | None, x0: Tensor | None, xt: Tensor | None, t: Tensor, tables: Tensor, target: int,
                weight: Tensor | None, var_mode: int, out: Tensor | None = None, partial: Tensor | None = None) -> Tensor:
    """the loss of any parameterisation (dl_gd_loss_fwd).  var_mode VAR_FIXED: pred [B, C, ...] -> f32 scalar, the weighted mse;
    a learned var_mode: pred [B, 2C, ...] -> f32 [2] = (weighted mse of the mean half, variational bound in bits / dim).
    weight: f32 [T] per-timestep weight or None; eps / x0 / xt may be None where the mode does not read them; partial: the scratch
    of dl_mse_loss_partials(n) floats (twice that for learned variances), allocated here when None."""
    fixed = var_mode == VAR_FIXED
    B = pred.shape[0]
    n = pred.numel() if fixed else pred.numel() // 2
    assert all(v is None or v.numel() == n for v in (eps, x0, xt)) and (weight is None or weight.numel() == tables.shape[1])
    npart = lib().call("dl_mse_loss_partials", n)
    if partial is None:
        partial = torch.empty(npart if fixed else 2 * npart, device=pred.device, dtype=torch.float32)
    assert partial.numel() >= (npart if fixed else 2 * npart)
    if out is None:
        out = torch.empty(() if fixed else 2, device=pred.device, dtype=torch.float32)
    _call("dl_gd_loss_fwd", _p(pred), _p(eps), _p(x0), _p(xt), _p(t), _p(tables), tables.shape[1], target, _p(weight), var_mode,
          _p(partial), _p(out), B, n // B, _s())
    return out


def gd_loss_bwd(pred: Tensor, eps: Tensor | None, x0: Tensor | None, xt: Tensor | None, t: Tensor, tables: Tensor, target: int,
                weight: Tensor | None, var_mode: int, g_mse: Tensor | None, g_vb: Tensor | None, out: Tensor | None = None) -> Tensor:
    """dpred (the shape of pred) in one pass; g_mse / g_vb: the scalars' upstream gradients as device scalars (None = 1)"""
    B = pred.shape[0]
    n = pred.numel() if var_mode == VAR_FIXED else pred.numel() // 2
    assert all(v is None or v.numel() == n for v in (eps, x0, xt)) and (weight is None or weight.numel() == tables.shape[1])
    out = torch.empty_like(pred) if out is None else out
    _call("dl_gd_loss_bwd", _p(pred), _p(eps), _p(x0), _p(xt), _p(t), _p(tables), tables.shape[1], target, _p(weight), var_mode,
          _p(g_mse), _p(g_vb), _p(out), B, n // B, _s())
    return out


def vb_terms(pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, tables: Tensor, lv_q: Tensor, mean_type: int,
             var_mode: int, clip_denoised: bool, out: tuple[Tensor, Tensor, Tensor] | None = None) -> tuple[Tensor, Tensor, Tensor]:
    """-> (vb, xstart_mse, mse), f32 [R] each: the variational-bound term in bits / dim and the two squared errors of every row, one
    row per (sample, timestep) pair (dl_vb_terms).  pred [R, C, ...] (VAR_FIXED) or [R, 2C, ...]; eps, x0, xt [R, C, ...]; t int32
    [R]; tables f32 [6, T] = DDPM._tables; lv_q f32 [T] = posterior_log_variance_clipped; out: three f32 [R] windows, allocated here
    when None"""
    R, n = xt.shape[0], xt.numel()
    chw = n // R
    assert pred.numel() == (1 if var_mode == VAR_FIXED else 2) * n and eps.numel() == n and x0.numel() == n and t.numel() == R
    assert tables.shape[0] == 6 and lv_q.numel() == tables.shape[1]
    nshare = lib().call("dl_mse_loss_partials", chw)
    partial = torch.empty(3 * R * nshare, device=pred.device, dtype=torch.float32) if nshare > 1 else None
    vb, xstart_mse, mse = (torch.empty(R, device=pred.device, dtype=torch.float32) for _ in range(3)) if out is None else out
    _call("dl_vb_terms", _p(pred), _p(eps), _p(x0), _p(xt), _p(t), _p(tables), tables.shape[1], _p(lv_q), mean_type, var_mode,
          int(bool(clip_denoised)), _p(partial), _p(vb), _p(xstart_mse), _p(mse), R, chw, _s())
    return vb, xstart_mse, mse


def prior_bpd(x0: Tensor, alphas_bar_last: float, log_one_minus_ab: float, out: Tensor | None = None) -> Tensor:
    """-> f32 [B]: KL(q(x_T | x0) || N(0, I)) of every sample in bits / dim (dl_prior_bpd); the two scalars are alphas_bar[T-1] and
    log(1 - alphas_bar[T-1]), formed in fp64 by the caller"""
    B = x0.shape[0]
    chw = x0.numel() // B
    nshare = lib().call("dl_mse_loss_partials", chw)
    partial = torch.empty(B * nshare, device=x0.device, dtype=torch.float32) if nshare > 1 else None
    out = torch.empty(B, device=x0.device, dtype=torch.float32) if out is None else out
    _call("dl_prior_bpd", _p(x0), float(alphas_bar_last), float(log_one_minus_ab), _p(partial), _p(out), B, chw, _s())
    return out


def hutchinson_step(g: Tensor, eps: Tensor, out: Tensor, col: int, scale: float, x: Tensor | None = None, v: Tensor | None = None,
                    a: float = 0.0, v0: Tensor | None = None, b: float = 0.0, x_out: Tensor | None = None,
                    partial: Tensor | None = None) -> Tensor:
    """one evaluation of the ODE likelihood behind its input-gradient backward (dl_hutchinson_step): out[r, col] = scale *
    sum(g[r] * eps[r]) of the f32 table out [R, n]; with x_out also x_out = x + a v (+ b v0).  g, eps, x, v, v0, x_out: contiguous f32
    [R, ...]; partial: the scratch of R * dl_mse_loss_partials(chw) floats rows of more than 4096 elements need, allocated here when
    None"""
    R = g.shape[0]
    chw = g.numel() // R
    assert out.dim() == 2 and out.shape[0] == R and out.stride(1) == 1 and out.dtype == torch.float32 and 0 <= col < out.shape[1]
    assert all(q is None or (q.dtype == torch.float32 and q.is_contiguous() and q.numel() == R * chw) for q in (g, eps, x, v, v0, x_out))
    nshare = lib().call("dl_mse_loss_partials", chw)
    if partial is None and nshare > 1:
        partial = torch.empty(R * nshare, device=g.device, dtype=torch.float32)
    assert partial is None or partial.numel() >= R * nshare
    _call("dl_hutchinson_step", _p(x), _p(v), _p(v0), float(a), float(b), _p(x_out), _p(g), _p(eps), float(scale), _p(partial), _p(out),
          out.stride(0), col, R, chw, _s())
    return out


def normal_nll_rows(x: Tensor, out: Tensor | None = None) -> Tensor:
    """-> f32 [R]: 0.5 mean(x[r]^2) + 0.5 log(2 pi), the negative log-density of every row under N(0, I) in nats per dimension
    (dl_normal_nll_rows); x contiguous f32 [R, ...]"""
    R = x.shape[0]
    chw = x.numel() // R
    assert x.dtype == torch.float32 and x.is_contiguous()
    nshare = lib().call("dl_mse_loss_partials", chw)
    partial = torch.empty(R * nshare, device=x.device, dtype=torch.float32) if nshare > 1 else None
    out = torch.empty(R, device=x.device, dtype=torch.float32) if out is None else out
    _call("dl_normal_nll_rows", _p(x), _p(partial), _p(out), R, chw, _s())
    return out


LOSS_TYPES = {"mse": 0, "vlb": 1}


def gd_loss_rows_fwd(pred: Tensor, eps: Tensor | None, x0: Tensor | None, xt: Tensor | None, t: Tensor, tables: Tensor, target: int,
                     weight: Tensor | None, imp: Tensor | None, var_mode: int, loss_type: int, vb_scale: float,
                     out: tuple[Tensor, Tensor | None, Tensor, Tensor] | None = None) -> tuple[Tensor, Tensor | None, Tensor, Tensor]:
    """the row head (dl_gd_loss_rows_fwd) -> (mse_row f32 [B], vb_row f32 [B] or None with VAR_FIXED, total_row f32 [B], loss f32
    [2], of which VAR_FIXED writes loss[0] alone).  Arguments as `gd_loss_fwd`, plus imp f32 [T] or None (the importance weights),
    loss_type (LOSS_TYPES) and vb_scale, the weight of the bound in total_row."""
    fixed = var_mode == VAR_FIXED
    B = pred.shape[0]
    n = pred.numel() if fixed else pred.numel() // 2
    T = tables.shape[1]
    assert all(v is None or v.numel() == n for v in (eps, x0, xt)) and t.numel() == B
    assert all(v is None or v.numel() == T for v in (weight, imp))
    chw = n // B
    nshare = lib().call("dl_mse_loss_partials", chw)
    partial = torch.empty(2 * B * nshare, device=pred.device, dtype=torch.float32) if nshare > 1 else None
    if out is None:
        rows = torch.empty(3, B, device=pred.device, dtype=torch.float32)
        out = (rows[0], None if fixed else rows[1], rows[2], torch.empty(2, device=pred.device, dtype=torch.float32))
    mse_row, vb_row, total_row, loss = out
    _call("dl_gd_loss_rows_fwd", _p(pred), _p(eps), _p(x0), _p(xt), _p(t), _p(tables), T, target, _p(weight), _p(imp), var_mode,
          loss_type, float(vb_scale), _p(partial), _p(mse_row), _p(vb_row), _p(total_row), _p(loss), B, chw, _s())
    return mse_row, vb_row, total_row, loss


def gd_loss_rows_bwd(pred: Tensor, eps: Tensor | None, x0: Tensor | None, xt: Tensor | None, t: Tensor, tables: Tensor, target: int,
                     weight: Tensor | None, imp: Tensor | None, var_mode: int, loss_type: int, g_mse: Tensor | None,
                     g_vb: Tensor | None, out: Tensor | None = None) -> Tensor:
    """dpred (the shape of pred) of g_mse loss[0] + g_vb loss[1] in one pass (dl_gd_loss_rows_bwd); with loss_type "vlb" the bound
    sends its derivative into the mean output as well.  g_mse / g_vb: device scalars (None = 1)"""
    B = pred.shape[0]
    n = pred.numel() if var_mode == VAR_FIXED else pred.numel() // 2
    T = tables.shape[1]
    assert all(v is None or v.numel() == n for v in (eps, x0, xt)) and all(v is None or v.numel() == T for v in (weight, imp))
    out = torch.empty_like(pred) if out is None else out
    _call("dl_gd_loss_rows_bwd", _p(pred), _p(eps), _p(x0), _p(xt), _p(t), _p(tables), T, target, _p(weight), _p(imp), var_mode,
          loss_type, _p(g_mse), _p(g_vb), _p(out), B, n // B, _s())
    return out


def loss_history_update(t: Tensor | None, loss: Tensor | None, hist: Tensor, count: Tensor, p: Tensor, imp: Tensor, cdf: Tensor,
                        uniform_prob: float) -> None:
    """one training step of the loss-second-moment resampler (dl_loss_history_update), in place: the pairs (t[j], loss[j]) enter
    hist f32 [T, H] / count int32 [T] in array order, then p, imp, cdf f32 [T] are formed from the history.  t None: no pairs."""
    T, H = hist.shape
    n = 0 if t is None else t.numel()
    assert hist.dtype == torch.float32 and count.dtype == torch.int32 and hist.is_contiguous()
    assert count.numel() == T and p.numel() == T and imp.numel() == T and cdf.numel() == T
    assert n == 0 or (t.dtype == torch.int32 and loss.dtype == torch.float32 and loss.numel() == n)
    _call("dl_loss_history_update", _p(t), _p(loss), n, _p(hist), _p(count), _p(p), _p(imp), _p(cdf), T, H, float(uniform_prob), _s())


def draw_timesteps(u: Tensor, cdf: Tensor, out: Tensor | None = None) -> Tensor:
    """-> int32 [B]: the first index with cdf[i] > u[b] (dl_draw_timesteps); u f32 [B] in [0, 1), cdf f32 [T]"""
    assert u.dtype == torch.float32 and cdf.dtype == torch.float32
    out = torch.empty(u.numel(), device=u.device, dtype=torch.int32) if out is None else out
    _call("dl_draw_timesteps", _p(u), _p(cdf), cdf.numel(), _p(out), u.numel(), _s())
    return out


def flow_x_to_v(z: Tensor, xhat: Tensor, t: Tensor) -> Tensor:
    v = torch.empty_like(z)
    B = z.shape[0]
    _call("dl_flow_x_to_v", _p(z), _p(xhat), _p(t), _p(v), B, z.numel() // B, _s())
    return v


def flow_x_to_v_bwd(dv: Tensor, t: Tensor) -> Tensor:
    dx = torch.empty_like(dv)
    B = dv.shape[0]
    _call("dl_flow_x_to_v_bwd", _p(dv), _p(t), _p(dx), B, dv.numel() // B, _s())
    return dx


# ------------------------------------------------------------------ sampler steps
def euler_step(x: Tensor, v: Tensor, v_uncond: Tensor | None, guidance: float, t_curr: float, t_prev: float,
               want_x0: bool = True) -> tuple[Tensor, Tensor | None]:
    xp = torch.empty_like(x)
    x0 = torch.empty_like(x) if want_x0 else None
    _call("dl_euler_step", _p(x), _p(v), _p(v_uncond), float(guidance), float(t_curr), float(t_curr - t_prev), _p(xp),
          _p(x0), x.numel(), _s())
    return xp, x0


def euler_maruyama_step(x, v, v_uncond, guidance, noise, x_prev_in, t_curr, t_prev, sigma):
    dt = t_curr - t_prev
    std = sigma * dt**0.5
    xp, mean, x0, lp = (torch.empty_like(x) for _ in range(4))
    _call("dl_euler_maruyama_step", _p(x), _p(v), _p(v_uncond), float(guidance), _p(noise), _p(x_prev_in), float(t_curr),
          float(dt), float(sigma), float(std), _p(xp), _p(mean), _p(x0), _p(lp), x.numel(), _s())
    return xp, mean, x0, lp, std


def _check_pred(pred, pred_uncond, xt, halves: bool) -> None:
    """a Gaussian step's pred / pred_uncond are [B, C, ...] or, halves, the [B, 2C, ...] prediction of a learned-variance model"""
    assert pred.numel() == (2 if halves else 1) * xt.numel() and (pred_uncond is None or pred_uncond.numel() == pred.numel())


def _step_out(xt, out, eta: float | None = None):
    """(x_prev, x0, mean, std, logprob) of a Gaussian step: `out` where given, else allocated here; DDIM (eta given) has std and
    logprob only when eta > 0"""
    if out is not None:
        return out
    n = 5 if eta is None or eta > 0 else 3
    return (*(torch.empty_like(xt) for _ in range(n)), *(None,) * (5 - n))


def ddpm_step(pred, pred_uncond, guidance, xt, noise, t, tables, mean_type: int, clamp_x: bool):
    B = xt.shape[0]
    xp, x0, mean, std, lp = _step_out(xt, None)
    _call("dl_ddpm_step", _p(pred), _p(pred_uncond), float(guidance), _p(xt), _p(noise), _p(t), _p(tables),
          tables.shape[1], mean_type, int(clamp_x), _p(xp), _p(x0), _p(mean), _p(std), _p(lp), B, xt.numel() // B, _s())
    return xp, x0, mean, std, lp


def ddpm_step_lv(pred, pred_uncond, guidance, xt, noise, t, tables, mean_type: int, var_mode: int, clamp_x: bool, out=None):
    """learned variances: pred / pred_uncond are [B, 2C, ...], read in place; tables f32 [6, T] with rows 4, 5 =
    posterior_log_variance_clipped, betas; out: the five [B, C, ...] outputs, allocated here when None"""
    B = xt.shape[0]
    _check_pred(pred, pred_uncond, xt, True)
    xp, x0, mean, std, lp = _step_out(xt, out)
    _call("dl_ddpm_step_lv", _p(pred), _p(pred_uncond), float(guidance), _p(xt), _p(noise), _p(t), _p(tables),
          tables.shape[1], mean_type, var_mode, int(clamp_x), _p(xp), _p(x0), _p(mean), _p(std), _p(lp), B, xt.numel() // B, _s())
    return xp, x0, mean, std, lp


def ddim_step(pred, pred_uncond, guidance, xt, noise, t, tables, coefs, mean_type: int, clamp_x: bool, eta: float,
              halves: bool = False, out=None):
    """halves: pred / pred_uncond are the [B, 2C, ...] prediction of a learned-variance model; its mean half is read in place"""
    B = xt.shape[0]
    _check_pred(pred, pred_uncond, xt, halves)
    xp, x0, mean, std, lp = _step_out(xt, out, eta)
    _call("dl_ddim_step_lv" if halves else "dl_ddim_step", _p(pred), _p(pred_uncond), float(guidance), _p(xt), _p(noise), _p(t), _p(tables),
          tables.shape[1], mean_type, _p(coefs), int(clamp_x), float(eta), _p(xp), _p(x0), _p(mean), _p(std), _p(lp), B,
          xt.numel() // B, _s())
    return xp, x0, mean, std, lp


def ddpm_step_v(pred, pred_uncond, guidance, xt, noise, t, tables, var_mode: int, clamp_x: bool, out=None):
    """v-prediction: pred / pred_uncond [B, C, ...] and ddpm_step's tables (VAR_FIXED), or [B, 2C, ...] and ddpm_step_lv's"""
    B = xt.shape[0]
    _check_pred(pred, pred_uncond, xt, var_mode != VAR_FIXED)
    xp, x0, mean, std, lp = _step_out(xt, out)
    _call("dl_ddpm_step_v", _p(pred), _p(pred_uncond), float(guidance), _p(xt), _p(noise), _p(t), _p(tables), tables.shape[1],
          var_mode, int(clamp_x), _p(xp), _p(x0), _p(mean), _p(std), _p(lp), B, xt.numel() // B, _s())
    return xp, x0, mean, std, lp


def ddim_step_v(pred, pred_uncond, guidance, xt, noise, t, tables, var_mode: int, clamp_x: bool, eta: float, out=None):
    """v-prediction: pred / pred_uncond [B, C, ...] (VAR_FIXED) or [B, 2C, ...], whose mean half is read in place; tables f32 [3, T]"""
    B = xt.shape[0]
    _check_pred(pred, pred_uncond, xt, var_mode != VAR_FIXED)
    xp, x0, mean, std, lp = _step_out(xt, out, eta)
    _call("dl_ddim_step_v", _p(pred), _p(pred_uncond), float(guidance), _p(xt), _p(noise), _p(t), _p(tables), tables.shape[1],
          var_mode, int(clamp_x), float(eta), _p(xp), _p(x0), _p(mean), _p(std), _p(lp), B, xt.numel() // B, _s())
    return xp, x0, mean, std, lp


# guided sampling (CFG rescale, dynamic thresholding): per-sample coefficients that stay on the device, and the steps that read them
def cfg_rescale_coef(pred: Tensor, pred_uncond: Tensor, guidance: float, phi: float, halves: bool = False,
                     out: Tensor | None = None) -> Tensor:
    """-> r f32 [B], the CFG-rescale factor of every sample (dl_cfg_rescale_coef).  halves: pred / pred_uncond are the [B, 2C, ...]
    prediction of a learned-variance model; the mean half is read in place"""
    B = pred.shape[0]
    stride = pred.numel() // B
    assert pred_uncond.numel() == pred.numel() and (not halves or stride % 2 == 0)
    out = torch.empty(B, device=pred.device, dtype=torch.float32) if out is None else out
    _call("dl_cfg_rescale_coef", _p(pred), _p(pred_uncond), float(guidance), float(phi), _p(out), B, stride // 2 if halves else stride,
          stride, _s())
    return out


def abs_quantile_rows(x: Tensor, k: int, f: float, want_lohi: bool = False):
    """x f32 [B, n] -> q f32 [B] = lo + f (hi - lo) over |x| per row, lo / hi the k-th and min(k + 1, n - 1)-th smallest (exact
    selection, dl_abs_quantile_rows); with want_lohi also lohi f32 [B, 2]"""
    assert x.dim() == 2 and x.dtype == torch.float32 and x.is_contiguous()
    B, n = x.shape
    q = torch.empty(B, device=x.device, dtype=torch.float32)
    lohi = torch.empty(B, 2, device=x.device, dtype=torch.float32) if want_lohi else None
    _call("dl_abs_quantile_rows", _p(x), int(k), float(f), _p(q), _p(lohi), B, n, _s())
    return (q, lohi) if want_lohi else q


def x0_threshold(pred, pred_uncond, guidance, cfg_mul, xt, t, tables, coefs, mean_type: int, k: int, f: float,
                 threshold_max: float | None = None, halves: bool = False, want_lohi: bool = False):
    """-> s f32 [B], the dynamic threshold min(max(quantile of |x0|, 1), threshold_max) of every sample, x0 as the `*_step_g` kernels
    form it from the same arguments (dl_x0_threshold); tables: the step's own (rows 0, 1 are read); coefs f32 [2, T]: the posterior-mean
    coefficients, needed for mean_type xprev only"""
    B = xt.shape[0]
    _check_pred(pred, pred_uncond, xt, halves)
    s = torch.empty(B, device=xt.device, dtype=torch.float32)
    lohi = torch.empty(B, 2, device=xt.device, dtype=torch.float32) if want_lohi else None
    _call("dl_x0_threshold", _p(pred), _p(pred_uncond), float(guidance), _p(cfg_mul), _p(xt), _p(t), _p(tables), tables.shape[1],
          mean_type, _p(coefs), int(k), float(f), float("inf") if threshold_max is None else float(threshold_max), _p(s), _p(lohi), B,
          xt.numel() // B, pred.numel() // B, _s())
    return (s, lohi) if want_lohi else s


def euler_step_g(x: Tensor, v: Tensor, v_uncond: Tensor | None, guidance: float, cfg_mul: Tensor | None, t_curr: float, t_prev: float,
                 want_x0: bool = True) -> tuple[Tensor, Tensor | None]:
    B = x.shape[0]
    xp = torch.empty_like(x)
    x0 = torch.empty_like(x) if want_x0 else None
    _call("dl_euler_step_g", _p(x), _p(v), _p(v_uncond), float(guidance), _p(cfg_mul), float(t_curr), float(t_curr - t_prev), _p(xp),
          _p(x0), B, x.numel() // B, _s())
    return xp, x0


def euler_maruyama_step_g(x, v, v_uncond, guidance, cfg_mul, noise, x_prev_in, t_curr, t_prev, sigma):
    B = x.shape[0]
    dt = t_curr - t_prev
    std = sigma * dt**0.5
    xp, mean, x0, lp = (torch.empty_like(x) for _ in range(4))
    _call("dl_euler_maruyama_step_g", _p(x), _p(v), _p(v_uncond), float(guidance), _p(cfg_mul), _p(noise), _p(x_prev_in),
          float(t_curr), float(dt), float(sigma), float(std), _p(xp), _p(mean), _p(x0), _p(lp), B, x.numel() // B, _s())
    return xp, mean, x0, lp, std


def ddpm_step_g(pred, pred_uncond, guidance, cfg_mul, x0_thr, xt, noise, t, tables, mean_type: int, var_mode: int, clamp_x: bool,
                out=None):
    """any mean_type (v included) and var_mode: VAR_FIXED with pred [B, C, ...] and ddpm_step's tables, or a learned mode with
    [B, 2C, ...] and ddpm_step_lv's; cfg_mul / x0_thr f32 [B] or None"""
    B = xt.shape[0]
    _check_pred(pred, pred_uncond, xt, var_mode != VAR_FIXED)
    xp, x0, mean, std, lp = _step_out(xt, out)
    _call("dl_ddpm_step_g", _p(pred), _p(pred_uncond), float(guidance), _p(cfg_mul), _p(x0_thr), _p(xt), _p(noise), _p(t), _p(tables),
          tables.shape[1], mean_type, var_mode, int(clamp_x), _p(xp), _p(x0), _p(mean), _p(std), _p(lp), B, xt.numel() // B, _s())
    return xp, x0, mean, std, lp


def ddim_step_g(pred, pred_uncond, guidance, cfg_mul, x0_thr, xt, noise, t, tables, coefs, mean_type: int, var_mode: int,
                clamp_x: bool, eta: float, out=None):
    """as ddpm_step_g, with ddim_step's tables f32 [3, T] and coefs (needed for mean_type xprev only)"""
    B = xt.shape[0]
    _check_pred(pred, pred_uncond, xt, var_mode != VAR_FIXED)
    xp, x0, mean, std, lp = _step_out(xt, out, eta)
    _call("dl_ddim_step_g", _p(pred), _p(pred_uncond), float(guidance), _p(cfg_mul), _p(x0_thr), _p(xt), _p(noise), _p(t), _p(tables),
          tables.shape[1], mean_type, var_mode, _p(coefs), int(clamp_x), float(eta), _p(xp), _p(x0), _p(mean), _p(std), _p(lp), B,
          xt.numel() // B, _s())
    return xp, x0, mean, std, lp


# second-order multistep samplers: one launch per step, the step coefficients formed on the host in double
def ab2_step(x: Tensor, v: Tensor, v_uncond: Tensor | None, guidance: float, cfg_mul: Tensor | None, v_last: Tensor | None,
             t_curr: float, t_prev: float, w: float = 0.0, out=None) -> tuple[Tensor, Tensor, Tensor]:
    """-> (x_prev, x0_est, v_out); v_last None: the Euler step (w is not read).  v_out, the combined v, is the next step's v_last"""
    B = x.shape[0]
    assert v.numel() == x.numel() and (v_uncond is None or v_uncond.numel() == x.numel()) and (v_last is None or v_last.numel() == x.numel())
    xp, x0, vo = (torch.empty_like(x) for _ in range(3)) if out is None else out
    _call("dl_ab2_step", _p(x), _p(v), _p(v_uncond), float(guidance), _p(cfg_mul), _p(v_last), float(t_curr), float(t_curr - t_prev),
          float(w), _p(xp), _p(x0), _p(vo), B, x.numel() // B, _s())
    return xp, x0, vo


def dpmpp_2m_step(pred, pred_uncond, guidance, cfg_mul, x0_thr, xt, x0_last, t, tables, mean_type: int, var_mode: int, clamp_x: bool,
                  a: float, b: float, c: float, out=None) -> tuple[Tensor, Tensor]:
    """-> (x_prev, x0_est) with x_prev = a xt + b x0 + c x0_last, x0 formed as ddim_step_g forms it (tables f32 [>= 2, T]: ddim_step's);
    x0_last None needs c == 0; mean_type xprev is refused"""
    B = xt.shape[0]
    _check_pred(pred, pred_uncond, xt, var_mode != VAR_FIXED)
    assert x0_last is None or x0_last.numel() == xt.numel()
    xp, x0 = (torch.empty_like(xt) for _ in range(2)) if out is None else out
    _call("dl_dpmpp_2m_step", _p(pred), _p(pred_uncond), float(guidance), _p(cfg_mul), _p(x0_thr), _p(xt), _p(x0_last), _p(t), _p(tables),
          tables.shape[1], mean_type, var_mode, int(clamp_x), float(a), float(b), float(c), _p(xp), _p(x0), B, xt.numel() // B, _s())
    return xp, x0


def inpaint_blend(x: Tensor | None, ref: Tensor, noise: Tensor | None, mask: Tensor | None, a: float, b: float,
                  out: Tensor | None = None) -> Tensor:
    """known = a ref + b noise; with a mask ([B, 1, *spatial] or [B, C, *spatial], f32, 1 = generate) out = x where mask >= 1, known
    where mask <= 0, mask x + (1 - mask) known between; mask None (then x None): out = known, the re-noise form.  noise may be None
    when b == 0.  All tensors f32 and contiguous, ref [B, C, *spatial]; out may be x or ref, allocated here when None."""
    assert ref.dim() >= 2 and ref.dtype == torch.float32 and ref.is_contiguous()
    B, C = ref.shape[0], ref.shape[1]
    hw = ref.numel() // (B * C) if ref.numel() else 0
    for other in (x, noise, out):
        assert other is None or (other.shape == ref.shape and other.dtype == torch.float32 and other.is_contiguous())
    mc = 0
    if mask is not None:
        assert mask.dtype == torch.float32 and mask.is_contiguous() and mask.dim() == ref.dim()
        assert mask.shape[0] == B and mask.shape[2:] == ref.shape[2:], (tuple(mask.shape), tuple(ref.shape))
        mc = mask.shape[1]
    out = torch.empty_like(ref) if out is None else out
    _call("dl_inpaint_blend", _p(x), _p(ref), _p(noise), _p(mask), float(a), float(b), _p(out), B, C, hw, mc, _s())
    return out


# ------------------------------------------------------------------ GEMMs
def gemm_nt(a: Tensor, b: Tensor, out: Tensor, *, bias: Tensor | None = None, act: int = ACT_NONE,
            pre_out: Tensor | None = None, resid: Tensor | None = None, gate: Tensor | None = None,
            rows_per_gate: int = 1, M: int | None = None, N: int | None = None, K: int | None = None,
            scratch: Tensor | None = None) -> Tensor:
    """out[M,N] = epilogue(a[M,K] @ b[N,K]^T); a/b bf16 2-D (row stride = .stride(0)); out bf16 or f32.
    scratch (f32, plain f32 output only): the bit-reproducible form -- a split contraction keeps its partial images there and
    folds them in a fixed order instead of meeting in f32 atomics (dl_gemm_nt_f32_det)."""
    M = a.shape[0] if M is None else M
    N = b.shape[0] if N is None else N
    K = a.shape[1] if K is None else K
    if scratch is not None:
        assert out.dtype == torch.float32 and bias is None and act == ACT_NONE and pre_out is None and resid is None
        _call("dl_gemm_nt_f32_det", _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K, _p(scratch), scratch.numel(),
              _s())
        return out
    _call("dl_gemm_nt", _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, K, _p(bias), act,
          F32 if out.dtype == torch.float32 else BF16, _p(pre_out), _p(resid), resid.stride(0) if resid is not None else 0,
          _p(gate), gate.stride(0) if gate is not None else 0, rows_per_gate, _s())
    return out


class _NtProblem(ctypes.Structure):
    """ctypes mirror of dl_nt_problem_t (include/diffulab_hip.h)"""

    _fields_ = [("A", ctypes.c_void_p), ("lda", ctypes.c_int64), ("B", ctypes.c_void_p), ("ldb", ctypes.c_int64), ("C", ctypes.c_void_p),
                ("ldc", ctypes.c_int64), ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64), ("bias", ctypes.c_void_p),
                ("resid", ctypes.c_void_p), ("ldr", ctypes.c_int64)]


def gemm_nt_pair(problems: list[tuple]) -> None:
    """two independent bf16 products out_i[M_i, N_i] = a_i[M_i, K_i] @ b_i[N_i, K_i]^T (+ bias_i, + resid_i) as ONE launch when both are
    small (dl_gemm_nt_pair; otherwise the two gemm_nt launches it stands for): entries (a, b, out, bias, resid, M, N, K), M / N / K may
    be None.  Bit-identical to the separate calls."""
    arr = (_NtProblem * len(problems))()
    for q, (a, b, out, bias, resid, M, N, K) in zip(arr, problems):
        assert out.dtype == torch.bfloat16
        q.A, q.lda, q.B, q.ldb, q.C, q.ldc = _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0)
        q.M, q.N, q.K = (a.shape[0] if M is None else M), (b.shape[0] if N is None else N), (a.shape[1] if K is None else K)
        q.bias, q.resid, q.ldr = _p(bias), _p(resid), (resid.stride(0) if resid is not None else 0)
    keep(arr)
    _call("dl_gemm_nt_pair", ctypes.addressof(arr), len(problems), _s())


def gemm_nt_swiglu(x: Tensor, w_perm: Tensor, u: Tensor | None, h: Tensor, stationary: bool = False, max_workgroups: int = 0) -> bool:
    """fused MLP-up GEMM + SwiGLU; u=None skips the pre-activation store (inference).  False when the shape has no fused
    kernel (caller falls back to gemm_nt + swiglu_fwd).  stationary: try dl_gemm_nt_swiglu_stationary first (activation panel in
    registers, K <= 512; bit-identical outputs; max_workgroups as in the header) and keep the persistent tiles for shapes it refuses"""
    args = (_p(x), x.stride(0), _p(w_perm), w_perm.stride(0), _p(u), u.stride(0) if u is not None else 0, _p(h), h.stride(0), x.shape[0],
            h.shape[1], x.shape[1])
    rc = lib().cdll.dl_gemm_nt_swiglu_stationary(*args, int(max_workgroups), _s()) if stationary else -3
    if rc == -3:
        rc = lib().cdll.dl_gemm_nt_swiglu(*args, _s())
    if rc == -3:
        return False
    if rc != 0:
        raise RuntimeError(f"dl_gemm_nt_swiglu failed ({rc}): {lib().cdll.dl_last_error().decode()}")
    return True


def mlp_recompute_ok(M: int, D: int, F: int) -> bool:
    """shapes for which the training step keeps no SwiGLU pre-activations (the backward recomputes them: csrc/mlp_bwd.hip) --
    the rule implies that the fused MLP-up forward serves the shape too; DL_MLP_RECOMPUTE=0 turns it off"""
    import os

    # F % 128: the recompute kernel's unit tile (the fused MLP-up forward takes any 2F % 128 with >= 64 tiles).  D <= 512: measured
    # -3 % on the DiT-S/2 step (D = 384, F = 1536); at D = 768, F = 3072 it is neutral (DiT-B + REPA, B = 128) to +3..5 % (joint MMDiT:
    # the wider contraction makes the recomputed GEMM cost more than the bytes it saves).
    return (tuning.on("DL_MLP_RECOMPUTE") and M % 256 == 0 and D % 64 == 0 and D <= 512 and F % 128 == 0
            and (M // 256) * (F // 128) >= 64)


def mlp_u_buffer(alloc, M: int, D: int, F: int, train: bool):
    """the [M, 2F] pre-activation buffer of a block's workspace, or None when the training backward recomputes it"""
    return None if (train and mlp_recompute_ok(M, D, F)) else alloc(M, 2 * F)


def mlp_swiglu_bwd(dt: Tensor, w2t: Tensor, x: Tensor, wp: Tensor, u: Tensor | None, dh: Tensor, du: Tensor) -> None:
    """du = SwiGLU backward of dh = dt @ w2t^T: from the saved pre-activations u, or (u None) recomputed per tile"""
    if u is None:
        if not mlp_dswiglu_recompute(x, wp, dt, w2t, du):
            raise RuntimeError("no saved SwiGLU pre-activations and no recompute kernel for this shape")
        return
    gemm_nt(dt, w2t, dh)
    swiglu_bwd(dh, u, du)


def mlp_dswiglu_recompute(x: Tensor, wp: Tensor, dt: Tensor, w2t: Tensor, du: Tensor) -> bool:
    """du = SwiGLU backward of dh = dt @ w2t^T with u = x @ wp^T recomputed per tile (nothing saved, nothing written but du);
    False when the shape has no such kernel (caller: dgrad GEMM + swiglu_bwd on the saved u)"""
    M, F = x.shape[0], w2t.shape[0]
    return _maybe("dl_mlp_dswiglu_recompute", _p(x), x.stride(0), _p(wp), wp.stride(0), _p(dt), dt.stride(0), _p(w2t), w2t.stride(0),
                  _p(du), du.stride(0), M, F, x.shape[1], dt.shape[1], _s())


def _padded_rows(t: Tensor) -> Tensor:
    """a row buffer allocated as the leading slice of a zero-padded parent (rows rounded up to 64): the parent"""
    base = t._base
    if base is not None and base.dim() == t.dim() and base.shape[1:] == t.shape[1:] and base.data_ptr() == t.data_ptr() \
            and base.shape[0] == (t.shape[0] + 63) // 64 * 64 and base.stride() == t.stride():
        return base
    return t


def gemm_tn(a: Tensor, b: Tensor, out: Tensor, *, M: int | None = None, N: int | None = None, max_wgs: int = 0,
            scratch: Tensor | None = None) -> Tensor:
    """out[M,N] (f32) += a[R,M]^T @ b[R,N].  max_wgs > 0 caps the persistent workgroups (side-stream wgrads).  R must be a
    multiple of 64: operands that are leading slices of zero-padded row buffers are widened to their parents.
    scratch (f32, >= M*N): the bit-reproducible form (dl_gemm_tn_det: partial images per split + fixed-order fold, no atomics)."""
    M = a.shape[1] if M is None else M
    N = b.shape[1] if N is None else N
    if a.shape[0] % 64:
        a, b = _padded_rows(a), _padded_rows(b)
        assert a.shape[0] == b.shape[0], "gemm_tn operands with a ragged row count must be zero-padded row buffers"
    if scratch is not None:
        _call("dl_gemm_tn_det", _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, a.shape[0], _p(scratch),
              scratch.numel(), _s())
        return out
    _call("dl_gemm_tn_ex", _p(a), a.stride(0), _p(b), b.stride(0), _p(out), out.stride(0), M, N, a.shape[0], int(max_wgs), _s())
    return out


class _WGrad(ctypes.Structure):
    """ctypes mirror of dl_wgrad_t (include/diffulab_hip.h)"""

    _fields_ = [("dy", ctypes.c_void_p), ("ld_dy", ctypes.c_int64), ("x", ctypes.c_void_p), ("ld_x", ctypes.c_int64),
                ("g", ctypes.c_void_p), ("m_out", ctypes.c_int64), ("n_in", ctypes.c_int64)]


def gemm_tn_group(probs: list[tuple[Tensor, Tensor, Tensor]], slab: Tensor, max_wgs: int = 0) -> bool:
    """g_p[M_p, N_p] (f32, contiguous) += dy_p[R, M_p]^T @ x_p[R, N_p] for up to four (dy, x, g) over the same R rows in ONE launch
    without atomics (bit-reproducible): partial tiles per token range go to `slab` (f32 scratch, >= sum M_p N_p elements; 8 x that
    fills the chip) and are folded in a fixed order.  False: the 384 x 192 tile does not divide a shape (nothing was launched)."""
    arr = (_WGrad * len(probs))()
    if probs[0][0].shape[0] % 64:  # leading slices of zero-padded row buffers: widen to the parents like gemm_tn
        probs = [(_padded_rows(dy), _padded_rows(x), g) for dy, x, g in probs]
    R = probs[0][0].shape[0]
    for q, (dy, x, g) in zip(arr, probs):
        assert dy.shape[0] == R and x.shape[0] == R and g.is_contiguous()
        q.dy, q.ld_dy, q.x, q.ld_x, q.g, q.m_out, q.n_in = _p(dy), dy.stride(0), _p(x), x.stride(0), _p(g), g.shape[0], g.shape[1]
    global _LIB
    if _LIB is None:
        _LIB = lib()
    fn = _LIB._fns["dl_gemm_tn_group"][0]
    rc = fn(ctypes.addressof(arr), len(probs), R, _p(slab), slab.numel(), int(max_wgs), _s())
    if rc == -3:  # DL_ERR_UNSUPPORTED
        return False
    if rc != 0:
        raise RuntimeError(f"dl_gemm_tn_group failed ({rc}): {_LIB.cdll.dl_last_error().decode()}")
    return True


_SCRATCH: dict = {}


def shared_scratch(device, floats: int) -> Tensor:
    """grow-only f32 scratch per device for the partial-image forms (gemm_tn / gemm_nt / colsum with scratch=) of modules that own
    no workspace (REPA projection head, Perceiver resampler).  Its users run on one stream in issue order, each launch pair
    (partials, fold) completes before the next begins, so one buffer serves them all."""
    key = (torch.device(device).type, torch.device(device).index)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < floats:
        buf = torch.empty(int(floats), device=device, dtype=torch.float32)
        _SCRATCH[key] = buf
    return buf


def wgrad_tile_ok(m_out: int, n_in: int) -> bool:
    """dl_gemm_tn_group has a tile for a [m_out, n_in] weight gradient (whole 384 x 192 or whole 256 x 256 tiles)"""
    return (m_out % 384 == 0 and n_in % 192 == 0) or (m_out % 256 == 0 and n_in % 256 == 0)


class WgradGroups:
    """Collects the weight-gradient problems (dy, x, g) an engine's backward produces and issues them as dl_gemm_tn_group launches:
    up to four problems over the SAME token rows per launch, no atomics, bit-reproducible (csrc/gemm_w4.hip).  Problems are keyed
    by their row count (the two token streams of a joint block have different ones); a key's list is launched when it holds four
    problems and at flush().  `launch(fn)` runs fn where the engine wants its weight gradients (side stream behind an event).
    Shapes the 384 x 192 tile does not divide fall back to one dl_gemm_tn_ex launch per problem."""

    def __init__(self, slab: Tensor, launch, max_wgs: int = 0) -> None:
        self.slab, self.launch, self.max_wgs = slab, launch, max_wgs
        self.pending: dict[int, list[tuple[Tensor, Tensor, Tensor]]] = {}

    @staticmethod
    def slab_floats(D: int, F: int, ranges: int | None = None) -> int:
        """scratch for the four linears of a block with inner width D and MLP width F (qkv, proj, up, down) at `ranges` token ranges.
        Default: 8 up to D = 1024; wider blocks have enough 384 x 192 tiles to fill 256 CUs with fewer token ranges (the launch splits
        by the CUs per tile and by what the slab holds), so the slab stops growing with 8 D^2 (8.6 GB at D = 4096)"""
        per = 4 * D * D + 3 * D * F
        if ranges is None:
            ranges = 8 if D <= 1024 else max(1, min(8, 256 * 384 * 192 // per))
        return ranges * per

    @staticmethod
    def widths_ok(D: int, F: int) -> bool:
        """the four linears of a block with inner width D and MLP width F are whole 384 x 192 tiles or whole 256 x 256 tiles -- or
        (round 6: 640-wide models) at least one 256 x 256 tile in each direction with widths that are multiples of 8: the last tile of
        a row / column is then shifted back to end at the edge"""
        if (D % 384 == 0 and F % 192 == 0) or (D % 256 == 0 and F % 256 == 0):
            return True
        r256 = lambda v: (v + 255) // 256 * 256  # noqa: E731
        return D % 8 == 0 and F % 8 == 0 and D >= 256 and F >= 256 and 4 * r256(D) <= 5 * D and 4 * r256(F) <= 5 * F  # (<= 25 % recomputed)

    @staticmethod
    def shapes_ok(D: int, F: int, rows: int) -> bool:
        return WgradGroups.widths_ok(D, F) and rows % 32 == 0 and rows >= 2048

    def add(self, dy: Tensor, x: Tensor, g: Tensor) -> None:
        lst = self.pending.setdefault(dy.shape[0], [])
        lst.append((dy, x, g))
        if len(lst) == 4:
            self._issue(dy.shape[0])

    def _issue(self, key: int) -> None:
        probs = self.pending.pop(key, [])
        if not probs:
            return

        def run() -> None:
            if not gemm_tn_group(probs, self.slab, max_wgs=self.max_wgs):
                for dy, x, g in probs:
                    gemm_tn(dy, x, g, max_wgs=self.max_wgs)

        self.launch(run)

    def flush(self) -> None:
        for key in list(self.pending):
            self._issue(key)


# ------------------------------------------------------------------ block kernels
def ln_modulate_fwd(x, w, b, scale, shift, rows_per_mod, eps, out, mean, rstd, t=None, gate=None, x_out=None):
    """out = modulate(LN(x')) with x' = x (+ gate * t, written to x_out, when the gated residual is fused in)"""
    M, D = x.shape
    _call("dl_ln_modulate_fwd", _p(x), _p(w), _p(b), _p(scale), _p(shift), scale.stride(0), rows_per_mod, float(eps),
          _p(out), _p(mean), _p(rstd), _p(t), _p(gate), gate.stride(0) if gate is not None else 0, _p(x_out), M, D, _s())


def ln_modulate_bwd(dout, x, w, b, scale, rows_per_mod, mean, rstd, dres, dx, dscale, dshift, dwb_partial, gate_t=None,
                    gate=None, dt=None, dgate=None):
    """dscale / dshift (/ dgate): f32 views [groups, D] with the same row stride, accumulated into; dwb_partial f32
    [groups, 2, D] or None.  gate_t / gate / dt / dgate: fused backward of the gated residual that follows (see header)."""
    M, D = x.shape
    assert dscale.dtype == torch.float32 and dshift.dtype == torch.float32
    assert dgate is None or (dgate.dtype == torch.float32 and dgate.stride(0) == dscale.stride(0))
    _call("dl_ln_modulate_bwd", _p(dout), _p(x), _p(w), _p(b), _p(scale), scale.stride(0), rows_per_mod, _p(mean),
          _p(rstd), _p(dres), _p(dx), _p(dscale), _p(dshift), dscale.stride(0), _p(dwb_partial), _p(gate_t), _p(gate),
          gate.stride(0) if gate is not None else 0, _p(dt), _p(dgate), M, D, _s())


def row_gemm_ok(M: int, D: int, rows_per_mod: int) -> bool:
    """shapes served by the row-complete GEMMs (csrc/gemm_ln.hip): a 256 x 384 tile is a whole sample's whole rows.
    DL_ROW_GEMM=0 restores the GEMM + row-kernel launch pairs (A/B switch)"""
    return tuning.on("DL_ROW_GEMM") and D == 384 and rows_per_mod == 256 and M % 256 == 0 and M // 256 >= 8


def ln_modulate_gemm_fwd(a, w_sh, resid, gate, ln_w, ln_b, scale, shift, rows_per_mod, eps, t_out, x_out, xm_out, mean, rstd,
                         K=None) -> bool:
    """t = a @ w_sh^T; x' = resid + gate * t; xm = modulate(LN(x')) in one launch; False when the shape has no such kernel"""
    M, D = xm_out.shape
    return _maybe("dl_ln_modulate_gemm_fwd", _p(a), a.stride(0), _p(w_sh), w_sh.stride(0), M, a.shape[1] if K is None else K, _p(resid),
                  _p(gate), gate.stride(0) if gate is not None else 0, _p(ln_w), _p(ln_b), _p(scale), _p(shift), scale.stride(0),
                  rows_per_mod, float(eps), _p(t_out), _p(x_out), _p(xm_out), _p(mean), _p(rstd), D, _s())


def ln_modulate_gemm_bwd(a, wt_sh, x, ln_w, ln_b, scale, rows_per_mod, mean, rstd, dres, dx, dscale, dshift, dwb_partial,
                         gate_t=None, gate=None, dt=None, dgate=None, K=None) -> bool:
    """dout = a @ wt_sh^T (never written) -> LayerNorm-modulate backward; dscale / dshift / dgate / dwb_partial are WRITTEN"""
    M, D = x.shape
    assert dscale.dtype == torch.float32 and dshift.dtype == torch.float32 and dshift.stride(0) == dscale.stride(0)
    assert dgate is None or (dgate.dtype == torch.float32 and dgate.stride(0) == dscale.stride(0))
    return _maybe("dl_ln_modulate_gemm_bwd", _p(a), a.stride(0), _p(wt_sh), wt_sh.stride(0), M, a.shape[1] if K is None else K, _p(x),
                  _p(ln_w), _p(ln_b), _p(scale), scale.stride(0), rows_per_mod, _p(mean), _p(rstd), _p(dres), _p(dx), _p(dscale),
                  _p(dshift), dscale.stride(0), _p(dwb_partial), _p(gate_t), _p(gate), gate.stride(0) if gate is not None else 0,
                  _p(dt), _p(dgate), D, _s())


def gemm_nt_qk_norm_rope(a, w_qkv, scale_q, scale_k, cos, sin, qkv, q, k, rrms, B, N, H, dh, rot, eps=1e-6, n_off=0) -> bool:
    """qkv = a @ w_qkv^T plus RMSNorm + RoPE + head split of its q / k thirds in one launch"""
    return _maybe("dl_gemm_nt_qk_norm_rope", _p(a), a.stride(0), _p(w_qkv), w_qkv.stride(0), B, N, H, dh, rot, float(eps),
                  _p(scale_q), _p(scale_k), _p(cos), _p(sin), _p(qkv), _p(q), _p(k), _p(rrms), q.shape[2], n_off, _s())


def ln_modulate_bwd_tok(dout, x, w, b, scale, mean, rstd, dres, dx, dscale, dshift, dwb_partial, gate_t=None, gate=None, dt=None,
                        dgate=None):
    """per-token modulation: scale / gate rows per token; dscale / dshift / dgate bf16 row windows written per token"""
    M, D = x.shape
    assert dscale.dtype == torch.bfloat16 and dshift.stride(0) == dscale.stride(0)
    _call("dl_ln_modulate_bwd_tok", _p(dout), _p(x), _p(w), _p(b), _p(scale), scale.stride(0), _p(mean), _p(rstd), _p(dres), _p(dx),
          _p(dscale), _p(dshift), dscale.stride(0), _p(dwb_partial), dwb_partial.shape[0] if dwb_partial is not None else 0,
          _p(gate_t), _p(gate), gate.stride(0) if gate is not None else 0, _p(dt), _p(dgate), M, D, _s())


def ddt_cond_fwd(enc, temb, B, N, out):
    _call("dl_ddt_cond_fwd", _p(enc), enc.stride(0), _p(temb), temb.stride(0), B, N, out.shape[1], _p(out), _s())


def ddt_cond_bwd(dsz, enc, temb, B, N, denc, dtemb):
    _call("dl_ddt_cond_bwd", _p(dsz), _p(enc), enc.stride(0), _p(temb), temb.stride(0), B, N, dsz.shape[1], _p(denc), _p(dtemb), _s())


def gate_bwd(dout, t, gate, rows_per_mod, dt, dgate):
    M, D = dout.shape
    _call("dl_gate_bwd", _p(dout), _p(t), _p(gate), gate.stride(0), rows_per_mod, _p(dt), _p(dgate), dgate.stride(0), M,
          D, _s())


def qk_norm_rope_fwd(qkv, scale_q, scale_k, cos, sin, q, k, v, rrms, B, N, H, dh, rot, eps=1e-6, pos=None, n_off=0):
    """pos: int32 [B*N] table row of every token (None: its index in the sequence); q / k / v are [B, H, n_dst, dh] and the N
    tokens are written to rows [n_off, n_off + N)"""
    _call("dl_qk_norm_rope_fwd_ex", _p(qkv), _p(scale_q), _p(scale_k), _p(cos), _p(sin), _p(q), _p(k), _p(v), _p(rrms), B, N,
          H, dh, rot, float(eps), _p(pos), q.shape[2], n_off, _s())


def qk_norm_rope_bwd(dq, dk, dv, qkv, scale_q, scale_k, cos, sin, rrms, dqkv, dscale, B, N, H, dh, rot, pos=None, n_off=0):
    _call("dl_qk_norm_rope_bwd_ex", _p(dq), _p(dk), _p(dv), _p(qkv), _p(scale_q), _p(scale_k), _p(cos), _p(sin), _p(rrms),
          _p(dqkv), _p(dscale), B, N, H, dh, rot, _p(pos), dq.shape[2], n_off, _s())


def copy_rows3d(src, src_bs, src_rs, dst, dst_bs, dst_rs, B, rows, cols):
    """dst[b, r, :cols] = src[b, r, :cols] with explicit batch / row strides (elements); src / dst may be offset views"""
    _call("dl_copy_rows3d", _p(src), src_bs, src_rs, _p(dst), dst_bs, dst_rs, B, rows, cols, _s())


# ------------------------------------------------------------------ SPRINT token routing
def gather_tokens(src, idx, dst, B, N, k, D, keep=None):
    _call("dl_gather_tokens", _p(src), src.stride(0), _p(idx), _p(keep), _p(dst), dst.stride(0), B, N, k, D, _s())


def scatter_tokens_add(src, idx, dst, B, N, k, D):
    _call("dl_scatter_tokens_add", _p(src), src.stride(0), _p(idx), _p(dst), dst.stride(0), B, N, k, D, _s())


def restore_tokens(xd, inv, mask, out, B, N, k, D):
    _call("dl_restore_tokens", _p(xd), xd.stride(0), _p(inv), _p(mask), _p(out), out.stride(0), B, N, k, D, _s())


def masked_colsum(x, sel, out, R, C):
    _call("dl_masked_colsum", _p(x), x.stride(0), _p(sel), _p(out), R, C, _s())


def gated_residual_fwd(x, t, gate, rows_per_mod, out):
    M, D = x.shape
    _call("dl_gated_residual_fwd", _p(x), _p(t), _p(gate), gate.stride(0), rows_per_mod, _p(out), out.stride(0), M, D, _s())


def attn_fwd(q, k, v, out, lse, B, H, N, dh, scale):
    _call("dl_attn_fwd", _p(q), _p(k), _p(v), _p(out), _p(lse), B, H, N, dh, float(scale), _s())


def attn_bwd(q, k, v, out, dout, lse, dq, dk, dv, B, H, N, dh, scale):
    _call("dl_attn_bwd", _p(q), _p(k), _p(v), _p(out), _p(dout), _p(lse), _p(dq), _p(dk), _p(dv), B, H, N, dh,
          float(scale), _s())


ATTN_MAX_TOKENS = 32768  # longest Nq / Nk of dl_attn_*: multiples of 256 up to here (up to 2048 the tiled kernels, beyond the long ones)
_INT32_ELEMS = 2 ** 31


def check_row_extent(rows: int, width: int, what: str) -> None:
    """refuse a token-row buffer [rows, width] whose element offsets would pass 2^31: the row kernels, GEMMs and token gathers on the
    bf16 engines' paths index elements with 32-bit integers in places"""
    if rows * width >= _INT32_ELEMS:
        raise NotImplementedError(f"{what}: {rows} token rows x {width} columns = {rows * width} elements exceed the 2^31 elements the "
                                  "bf16 regime's kernels index; use a smaller batch")


def attn_needs_padding(N: int) -> bool:
    """token counts the resident / tiled attention kernels do not take as they are (multiples of 64 up to 256, of 256 up to 32768):
    the caller pads q / k / v to a multiple of 256 rows and masks the pad keys (dl_attn_fwd_ex / _bwd_ex with a key bias)"""
    return N % 64 != 0 or (N > 256 and N % 256 != 0)


def v_in_place(N: int) -> bool:
    """up to 256 tokens the attention kernels address V / dV inside the token-major qkv / dqkv rows (no head-split copy of V);
    DL_ATTN_V_IN_PLACE=0 restores the head-major V buffers (A/B switch)"""
    return N <= 256 and N % 64 == 0 and tuning.on("DL_ATTN_V_IN_PLACE")


def dit_block_fwd(blk, train: bool) -> None:
    """one adaLN-zero DiT block forward issued by the library (blk: diffulab_amd._block.DitBlock)"""
    _call("dl_dit_block_fwd", ctypes.addressof(blk), int(train), _s())


def dit_block_fwd_chain(blk, train: bool) -> bool:
    """the row-complete block forward as ONE per-sample chain launch (csrc/block_fused.hip; dl_dit_block_fwd takes it by itself when
    bit 3 of blk.row_gemms is set); False when the library does not serve the block that way"""
    return _maybe("dl_dit_block_fwd_chain", ctypes.addressof(blk), int(train), _s())


def dit_block_bwd(blk, main_stream: int, side_stream: int, side_wgs: int) -> None:
    _call("dl_dit_block_bwd", ctypes.addressof(blk), main_stream, side_stream, int(side_wgs))


def attn_fwd_qkv(q, k, qkv, out, lse, B, H, N, dh, scale):
    """N <= 256: V is read in place from the v third of the token-major qkv rows [B*N, 3*H*dh]"""
    D = H * dh
    _call("dl_attn_fwd_sv", _p(q), _p(k), qkv.data_ptr() + 2 * D * 2, N * 3 * D, dh, 3 * D, _p(out), _p(lse), B, H, N, dh,
          float(scale), _s())


def gemm_nt_ssq(a, w_sh, out, ssq, stationary: bool = False, max_workgroups: int = 0) -> bool:
    """out[M, N] = a w_sh^T (bf16, persistent 256 x 384 tiles) + ssq[M, T] += row sums of squares of the first T = ssq.shape[1] 384-wide
    column tiles (ssq f32, zeroed by the caller): the qkv GEMM that also leaves the QK-RMSNorm statistics.  False: no such kernel for
    the shape (the caller keeps gemm_nt + qk_norm_rope_fwd)"""
    args = (_p(a), a.stride(0), _p(w_sh), w_sh.stride(0), _p(out), out.stride(0), a.shape[0], w_sh.shape[0], a.shape[1], _p(ssq), ssq.shape[1])
    # stationary: dl_gemm_nt_ssq_stationary first (activation panel in registers, K <= 512: the same `out` and ssq bits, ssq written with plain stores)
    if stationary and _maybe("dl_gemm_nt_ssq_stationary", *args, int(max_workgroups), _s()):
        return True
    return _maybe("dl_gemm_nt_ssq", *args, _s())


def attn_fwd_qkn(qkv, ssq, scale_q, scale_k, cos, sin, q, k, rrms, out, lse, B, H, N, dh, rot, scale, eps=1e-6):
    """attention forward from the PRE-NORM token-major qkv rows: QK-RMSNorm (statistics = ssq of gemm_nt_ssq) + RoPE applied as q
    and k are staged; writes the normalised q, k head-major and rrms [M, 2] for the backward kernels (N <= 256)"""
    _call("dl_attn_fwd_qkn", _p(qkv), _p(ssq), _p(scale_q), _p(scale_k), _p(cos), _p(sin), float(eps), rot, _p(q), _p(k), _p(rrms), _p(out),
          _p(lse), B, H, N, dh, float(scale), _s())


def attn_bwd_qkv(q, k, qkv, out, dout, lse, dq, dk, dqkv, B, H, N, dh, scale):
    """N <= 256: V read from qkv, dV written into the v third of dqkv [B*N, 3*H*dh] (qk_norm_rope_bwd then takes dv=None)"""
    D = H * dh
    _call("dl_attn_bwd_sv", _p(q), _p(k), qkv.data_ptr() + 2 * D * 2, N * 3 * D, dh, 3 * D, _p(out), _p(dout), _p(lse), _p(dq),
          _p(dk), dqkv.data_ptr() + 2 * D * 2, N * 3 * D, dh, 3 * D, B, H, N, dh, float(scale), _s())


def attn_bwd_tok(q, k, qkv, out, dout, lse, dqkv, B, H, N, dh, scale):
    """N <= 256: V read from qkv; dQ, dK AND dV written token-major into dqkv [B*N, 3*H*dh] (qk_norm_rope_bwd_inplace follows)"""
    _call("dl_attn_bwd_tok", _p(q), _p(k), _p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), B, H, N, dh, float(scale), _s())


def qk_inplace_ok(ws: dict, B: int, tokens: int) -> bool:
    """an engine with the partials scratch ws["qk_part"] takes the token-major attention backward + in-place QK-norm backward for
    this launch: V in place (<= 256 tokens per sample) and at least 32768 token rows (below that the two-kernel form is faster)"""
    return ws.get("qk_part") is not None and v_in_place(tokens) and B * tokens >= 32768


def qk_norm_rope_bwd_inplace(qkv, scale_q, scale_k, cos, sin, rrms, dqkv, dscale, partials, B, N, H, dh, rot, pos=None) -> bool:
    """the q / k thirds of dqkv: gradient after norm + RoPE (token-major) -> gradient of the pre-norm q / k, in place; dscale f32
    [2, D] += the scale gradients through `partials` (f32 scratch >= 1024 * 2 * D) in a fixed order.  False: inner width > 512"""
    assert partials.numel() >= 1024 * 2 * H * dh and partials.dtype == torch.float32
    return _maybe("dl_qk_norm_rope_bwd_inplace", _p(qkv), _p(scale_q), _p(scale_k), _p(cos), _p(sin), _p(rrms), _p(dqkv), _p(dscale),
                  _p(partials), B, N, H, dh, rot, _p(pos), _s())


def attn_fwd_ex(q, k, v, out, lse, B, H, Nq, Nk, dh, scale, key_bias=None):
    """Nq queries against Nk keys (multiples of 256), optional additive key bias f32 [B, Nk] (0 / -inf)"""
    _call("dl_attn_fwd_ex", _p(q), _p(k), _p(v), _p(out), _p(lse), B, H, Nq, Nk, dh, float(scale), _p(key_bias), _s())


def attn_bwd_ex(q, k, v, out, dout, lse, dq, dk, dv, B, H, Nq, Nk, dh, scale, key_bias=None):
    _call("dl_attn_bwd_ex", _p(q), _p(k), _p(v), _p(out), _p(dout), _p(lse), _p(dq), _p(dk), _p(dv), B, H, Nq, Nk, dh,
          float(scale), _p(key_bias), _s())


def swiglu_fwd(u, h):
    _call("dl_swiglu_fwd", _p(u), _p(h), u.shape[0], h.shape[1], _s())


def swiglu_bwd(dh, u, du):
    _call("dl_swiglu_bwd", _p(dh), _p(u), _p(du), u.shape[0], dh.shape[1], _s())


# ------------------------------------------------------------------ stem / head / conditioning
def patchify(x, tok, p, order):
    B, C, H, W = x.shape
    _call("dl_patchify", _p(x), _p(tok), B, C, H, W, p, tok.stride(0), order, _s())


def unpatchify(tok, img, p):
    B, C, H, W = img.shape
    _call("dl_unpatchify", _p(tok), _p(img), B, C, H, W, p, tok.stride(0), _s())


def patch_embed_dgrad(dtok, w, dimg, p):
    """dimg f32 [B, C, H, W] = gradient of the image behind the patch embedding (patchify, order CPP, then tokens = patches @ w^T)
    from the gradient dtok [M, D] (bf16 or f32 rows, any row stride) of its tokens; w: the f32 parameter [D, C, p, p] (contiguous)"""
    B, C, H, W = dimg.shape
    D = w.shape[0]
    assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() == D * C * p * p and dimg.dtype == torch.float32
    assert dimg.is_contiguous() and dtok.stride(1) == 1 and dtok.shape[1] >= D and dtok.dtype in (torch.bfloat16, torch.float32)
    assert dtok.shape[0] >= B * (H // p) * (W // p)
    _call("dl_patch_embed_dgrad", _p(dtok), BF16 if dtok.dtype == torch.bfloat16 else F32, dtok.stride(0), _p(w), _p(dimg), B, C, H, W,
          p, D, _s())
    return dimg


def timestep_embedding(t, out, max_period=10000.0):
    _call("dl_timestep_embedding", _p(t), _p(out), out.shape[0], out.shape[1], float(max_period), _s())


def cond_combine_fwd(e, table, idx, emb, act):
    _call("dl_cond_combine_fwd", _p(e), _p(table), _p(idx), _p(emb), _p(act), e.shape[0], e.shape[1], _s())


def cond_combine_bwd(dact, emb, idx, demb, demb16, dtable):
    _call("dl_cond_combine_bwd", _p(dact), _p(emb), _p(idx), _p(demb), _p(demb16), _p(dtable), emb.shape[0], emb.shape[1],
          _s())


def cond_combine_dense_fwd(e, pe, emb, act):
    """emb = e + pe (f32 [B, E], contiguous), act = silu(emb) bf16"""
    _call("dl_cond_combine_dense_fwd", _p(e), _p(pe), _p(emb), _p(act), e.shape[0], e.shape[1], _s())


def cond_combine_dense_bwd(dact, emb, demb, demb16):
    _call("dl_cond_combine_dense_bwd", _p(dact), _p(emb), _p(demb), _p(demb16), emb.shape[0], emb.shape[1], _s())


def silu_bwd(dy, pre, dx):
    _call("dl_silu_bwd", _p(dy), _p(pre), _p(dx), dy.numel(), _s())


def gelu_bwd(dy, pre, dx):
    _call("dl_gelu_bwd", _p(dy), _p(pre), _p(dx), dy.numel(), _s())


def heads_split_rope(src, dst, B, H, n_src, n_off, cos=None, sin=None, rot=0):
    """src [B*n_src, ld] -> dst [B, H, n_dst, 64] rows n_off.. (+ RoPE on the first `rot` channels when cos/sin are given)"""
    _call("dl_heads_split_rope", _p(src), src.stride(0), _p(dst), B, H, n_src, dst.shape[2], n_off, _p(cos), _p(sin), rot, _s())


def heads_merge_rope_bwd(dst_grad, src_grad, B, H, n_src, n_off, cos=None, sin=None, rot=0, accumulate=False):
    _call("dl_heads_merge_rope_bwd", _p(dst_grad), _p(src_grad), src_grad.stride(0), B, H, n_src, dst_grad.shape[2], n_off,
          _p(cos), _p(sin), rot, int(accumulate), _s())


def colsum(x, out, R=None, C=None, scratch=None):
    """out[c] += sum_r x[r, c]; scratch (f32): the bit-reproducible form (row-slab partials + fixed-order fold, dl_colsum_det)"""
    R = x.shape[0] if R is None else R
    C = x.shape[1] if C is None else C
    if scratch is not None:
        _call("dl_colsum_det", _p(x), F32 if x.dtype == torch.float32 else BF16, x.stride(0), _p(out), R, C, _p(scratch), scratch.numel(),
              _s())
        return
    _call("dl_colsum", _p(x), F32 if x.dtype == torch.float32 else BF16, x.stride(0), _p(out), R, C, _s())


class _ColsumDesc(ctypes.Structure):
    _fields_ = [("x", ctypes.c_void_p), ("ld", ctypes.c_int64), ("out", ctypes.c_void_p), ("R", ctypes.c_int64), ("C", ctypes.c_int64)]


def colsum_batched(items: list) -> None:
    """items: [(x bf16 [R, ld] rows, out f32 [C], R, C)]: out[c] += sum_r x[r, c] for all of them in one launch per 24"""
    arr = (_ColsumDesc * len(items))()
    for i, (x, out, R, C) in enumerate(items):
        assert x.dtype == torch.bfloat16 and out.dtype == torch.float32
        arr[i] = _ColsumDesc(_p(x), x.stride(0), _p(out), R, C)
    _call("dl_colsum_batched", ctypes.cast(arr, ctypes.c_void_p), len(items), _s())


def reduce_rows_f32(partial, out, G, n, clear=False):
    _call("dl_reduce_rows_f32", _p(partial), _p(out), G, n, int(clear), _s())


def reduce_rows_batched_f32(partial, partial_stride, out, out_stride, K, G, n):
    """K folds in one launch: out[k * out_stride + j] += sum_g partial[k * partial_stride + g * n + j] (deterministic)"""
    _call("dl_reduce_rows_batched_f32", _p(partial), partial_stride, _p(out), out_stride, K, G, n, _s())


def cosine_rows_fwd(p, d, cosv, pn2, dn2, eps=1e-8):
    M, E = p.shape
    _call("dl_cosine_rows_fwd", _p(p), p.stride(0), _p(d), d.stride(0), _p(cosv), _p(pn2), _p(dn2), M, E, float(eps), _s())


def cosine_rows_bwd(p, d, cosv, pn2, dn2, gscale, gscale_dev, dp, eps=1e-8):
    M, E = p.shape
    _call("dl_cosine_rows_bwd", _p(p), p.stride(0), _p(d), d.stride(0), _p(cosv), _p(pn2), _p(dn2), float(gscale),
          _p(gscale_dev), _p(dp), dp.stride(0), M, E, float(eps), _s())


# ------------------------------------------------------------------ optimizer side
def adamw_step(p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0):
    _call("dl_adamw_step", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
          float(wd), float(1.0 - beta1**step), float(1.0 - beta2**step), float(grad_scale), _s())


def adamw_step_dev(p, g, m, v, hyper):
    """AdamW with the scalars read from the device buffer `hyper` f32 [8] (graph-replayable launch)"""
    _call("dl_adamw_step_dev", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _s())


def grad_sumsq_chain(n: int) -> int:
    """terms on the longest serial f32 addition chain of `grad_sumsq` over n elements (host arithmetic): the sum's relative error is
    at most (chain + 2) * 2**-24"""
    return int(lib().call("dl_grad_sumsq_chain", int(n)))


def grad_sumsq_slots(n: int) -> int:
    """slots `grad_sumsq` writes for a buffer of n elements (host arithmetic: size the partials buffer from it)"""
    return int(lib().call("dl_grad_sumsq_slots", int(n)))


def grad_sumsq(x, partials, slot=0) -> int:
    """fixed-order sum of squares of the f32 buffer `x` into partials[slot : slot + k]; returns k, the slots written"""
    if x.dtype != torch.float32 or not x.is_contiguous() or partials.dtype != torch.float32 or not partials.is_contiguous():
        raise RuntimeError("grad_sumsq needs contiguous f32 tensors")
    global _LIB
    if _LIB is None:
        _LIB = lib()
    args = (_p(x), x.numel(), _p(partials), int(slot), partials.numel(), _s())
    k = _LIB.call("dl_grad_sumsq", *args)
    if k <= 0:
        raise RuntimeError(f"dl_grad_sumsq failed ({k}): {_LIB.cdll.dl_last_error().decode()}")
    if _REC is not None:
        _REC.calls.append((_negative_is_failure(_LIB._fns["dl_grad_sumsq"][0]), args))
    return k


def _negative_is_failure(fn):
    """a value-returning entry point as a launch-plan call (LaunchPlan.replay treats a non-zero return as a failure)"""
    return lambda *a: fn(*a) < 0


def clip_coef(partials, n_slots, max_norm, out, grad_scale=1.0, hyper=None):
    """out f32[2] = {grad_scale * sqrt(sum of partials[:n_slots]), min(1, max_norm / (norm + 1e-6))}; with `hyper` (the device
    scalars of `adamw_step_dev`) grad_scale is read from hyper[7]"""
    if n_slots > partials.numel() or out.numel() < 2 or out.dtype != torch.float32 or partials.dtype != torch.float32:
        raise RuntimeError("clip_coef: n_slots exceeds the partials buffer, or out is not f32[2]")
    _call("dl_clip_coef", _p(partials), int(n_slots), float(grad_scale), _p(hyper), float(max_norm), _p(out), _s())
    return out


def adamw_step_clip(p, g, m, v, lr, beta1, beta2, eps, wd, step, coef, grad_scale=1.0):
    """`adamw_step` with the gradient scaled by grad_scale * coef[0], `coef` a device f32 scalar (`clip_coef`'s out[1:2])"""
    _call("dl_adamw_step_clip", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
          float(wd), float(1.0 - beta1**step), float(1.0 - beta2**step), float(grad_scale), _p(coef), _s())


def adamw_step_dev_clip(p, g, m, v, hyper, coef):
    _call("dl_adamw_step_dev_clip", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper), _p(coef), _s())


SGD_NESTEROV, SGD_FIRST, SGD_MAXIMIZE = 1, 2, 4  # DL_SGD_* of include/diffulab_hip.h


def _sgd_check(p, g, buf):
    for t in (p, g, buf):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel()):
            raise RuntimeError("sgd_step needs contiguous f32 tensors of one size")


def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, wd=0.0, grad_scale=1.0, coef=None, nesterov=False, first=False,
             maximize=False):
    """torch.optim.SGD's update of the f32 buffer `p` in one launch; `buf` the momentum buffer (None with momentum == 0; `first`:
    it is written with the gradient, not read), `coef` an optional device f32 scalar the gradient scale is multiplied by
    (`clip_coef`'s out[1:2])"""
    _sgd_check(p, g, buf)
    flags = (SGD_NESTEROV if nesterov else 0) | (SGD_FIRST if first else 0) | (SGD_MAXIMIZE if maximize else 0)
    _call("dl_sgd_step", _p(p), _p(g), _p(buf), p.numel(), float(lr), float(momentum), float(dampening), float(wd),
          float(grad_scale), _p(coef), flags, _s())


def sgd_step_dev(p, g, buf, hyper, coef=None, nesterov=False, maximize=False):
    """SGD with the scalars read from the device buffer `hyper` f32 [8] = {lr, momentum, dampening, weight_decay, grad_scale, 0, 0,
    0} (graph-replayable launch); `buf` None = no momentum"""
    _sgd_check(p, g, buf)
    _call("dl_sgd_step_dev", _p(p), _p(g), _p(buf), p.numel(), _p(hyper), _p(coef),
          (SGD_NESTEROV if nesterov else 0) | (SGD_MAXIMIZE if maximize else 0), _s())


def scale_inplace(g, coef):
    """g *= coef[0] in place (f32, contiguous), `coef` a device f32 scalar"""
    if g.dtype != torch.float32 or not g.is_contiguous():
        raise RuntimeError("scale_inplace needs a contiguous f32 tensor")
    _call("dl_scale_inplace", _p(g), g.numel(), _p(coef), _s())
    return g


# ------------------------------------------------------------------ Muon (csrc/muon.hip)
MUON_MAT_FIELDS, MUON_CHUNK_FIELDS, MUON_CHUNK = 10, 3, 2048  # DL_MUON_* of include/diffulab_hip.h
MUON_TILE = 64


def muon_ratio(rows: int, cols: int, adjust_lr_fn: str | None) -> float:
    """torch.optim._muon._adjust_lr's factor"""
    if adjust_lr_fn is None or adjust_lr_fn == "original":
        return math.sqrt(max(1, rows / cols))
    if adjust_lr_fn == "match_rms_adamw":
        return 0.2 * math.sqrt(max(rows, cols))
    raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")


class MuonPlan:
    """The two tables of `dl_muon_*` for one flat f32 buffer of `n` elements (host copy and device copy of each) and the device
    workspaces they index: X (two bf16 copies of every Muon matrix), A and P (min(rows, cols)^2 bf16 each), one partial sum per
    chunk, one norm per matrix.

    `matrices`: [(offset, rows, cols, ratio)] sorted by offset; everything outside them is auxiliary (AdamW).  `phase`: the
    buffer's address in floats modulo 4 -- chunk boundaries are put on 16-byte boundaries of the buffer where a range allows, so
    that the pre pass can use float4 there."""

    def __init__(self, n: int, matrices: list[tuple[int, int, int, float]], phase: int, device) -> None:
        self.n, self.n_mat = int(n), len(matrices)
        mats = np.zeros((self.n_mat + 1, MUON_MAT_FIELDS), dtype=np.int64)
        chunks: list[np.ndarray] = []
        n_chunks = 0

        def add_range(s: int, e: int, mat: int) -> int:
            nonlocal n_chunks
            if e <= s:
                return 0
            first = min(e - s, MUON_CHUNK - ((s + phase) % 4))
            starts = np.concatenate([[s], np.arange(s + first, e, MUON_CHUNK, dtype=np.int64)]) if s + first < e else np.array([s], dtype=np.int64)
            ends = np.minimum(np.concatenate([starts[1:], [e]]), e)
            chunks.append(np.stack([starts, ends - starts, np.full_like(starts, mat)], axis=1))
            n_chunks += len(starts)
            return len(starts)

        at = x_off = a_off = sq = ap = 0
        for i, (off, rows, cols, ratio) in enumerate(matrices):
            if off < at:
                raise ValueError("MuonPlan: the matrices must be sorted by offset and must not overlap")
            add_range(at, off, -1)
            short = min(rows, cols)
            c0 = n_chunks
            nc = add_range(off, off + rows * cols, i)
            mats[i] = [off, rows, cols, int(np.float32(ratio).view(np.uint32)), x_off, a_off, sq, ap, c0, nc]
            x_off += rows * cols
            a_off += short * short
            sq += (short // MUON_TILE) ** 2
            ap += (rows // MUON_TILE) * (cols // MUON_TILE)
            at = off + rows * cols
        add_range(at, self.n, -1)
        mats[self.n_mat, 6:8] = [sq, ap]
        self.mats_host = torch.from_numpy(mats)
        self.chunks_host = torch.from_numpy(np.ascontiguousarray(np.concatenate(chunks, axis=0)))
        self.n_chunks = n_chunks
        self.has_aux = bool((self.chunks_host[:, 2] < 0).any())
        self.mats_dev, self.chunks_dev = self.mats_host.to(device), self.chunks_host.to(device)
        self.x_cap, self.a_cap = x_off, a_off
        self.xws = self.aws = self.partials = self.norms = None
        if self.n_mat:
            self.xws = torch.zeros(2 * x_off, dtype=torch.bfloat16, device=device)
            self.aws = torch.zeros(2 * a_off, dtype=torch.bfloat16, device=device)
            self.partials = torch.zeros(n_chunks, dtype=torch.float32, device=device)
            self.norms = torch.zeros(self.n_mat, dtype=torch.float32, device=device)

    def result(self, i: int, ns_steps: int) -> Tensor:
        """O of matrix i after `muon_orthogonalize(..., ns_steps)`: a bf16 [rows, cols] view of the X copy that holds it"""
        off, rows, cols = (int(v) for v in self.mats_host[i, [4, 1, 2]])
        lo = (ns_steps & 1) * self.x_cap + off
        return self.xws[lo : lo + rows * cols].view(rows, cols)


def _muon_check(plan: MuonPlan, *bufs) -> None:
    for t in bufs:
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != plan.n):
            raise RuntimeError(f"muon ops need contiguous f32 tensors of the plan's {plan.n} elements")


def muon_pre(plan: MuonPlan, p, g, m, v, lr, beta1, beta2, eps, wd, step, momentum, nesterov=True, grad_scale=1.0, coef=None):
    """one launch over the whole buffer: AdamW (`adamw_step`'s update, bit for bit) outside the plan's matrices; inside them the
    momentum buffer `m`, bf16(U) into the plan's X workspace and the per-chunk sums of squares.  `coef` as in `sgd_step`."""
    _muon_check(plan, p, g, m, v)
    _call("dl_muon_pre", _p(p), _p(g), _p(m), _p(v), plan.n, plan.chunks_host.data_ptr(), _p(plan.chunks_dev), plan.n_chunks,
          plan.mats_host.data_ptr(), _p(plan.mats_dev), plan.n_mat, _p(plan.xws), plan.x_cap, _p(plan.partials), plan.n_chunks,
          float(lr), float(beta1), float(beta2), float(eps), float(wd), float(1.0 - beta1**step), float(1.0 - beta2**step),
          float(momentum), float(grad_scale), _p(coef), int(bool(nesterov)), _s())


def muon_orthogonalize(plan: MuonPlan, eps, ns_coefficients, ns_steps) -> int:
    """every matrix of the plan: X = bf16(U) / max(||bf16(U)||_F, eps), then `ns_steps` quintic Newton-Schulz iterations, in
    2 + 3 * ns_steps launches whatever the number of matrices; returns the launches issued.  The result: `plan.result(i, ns_steps)`."""
    global _LIB
    if _LIB is None:
        _LIB = lib()
    a, b, c = ns_coefficients
    args = (plan.mats_host.data_ptr(), _p(plan.mats_dev), plan.n_mat, _p(plan.partials), _p(plan.norms), _p(plan.xws), plan.x_cap,
            _p(plan.aws), plan.a_cap, float(eps), float(a), float(b), float(c), int(ns_steps), _s())
    k = _LIB.call("dl_muon_orthogonalize", *args)
    if k <= 0:
        raise RuntimeError(f"dl_muon_orthogonalize failed ({k}): {_LIB.cdll.dl_last_error().decode()}")
    if _REC is not None:
        _REC.calls.append((_negative_is_failure(_LIB._fns["dl_muon_orthogonalize"][0]), args))
    return k


def muon_post(plan: MuonPlan, p, lr, wd, ns_steps):
    """one launch: p = p * (1 - lr * wd) - lr * ratio * O on the plan's matrices (O: the result of `muon_orthogonalize`)"""
    _muon_check(plan, p)
    xo = plan.xws[(ns_steps & 1) * plan.x_cap :]
    _call("dl_muon_post", _p(p), plan.n, plan.mats_host.data_ptr(), _p(plan.mats_dev), plan.n_mat, _p(xo), plan.x_cap, float(lr),
          float(wd), _s())


def cast_weight(src, dst, dst_t):
    R, C = src.shape
    _call("dl_cast_weight", _p(src), R, C, _p(dst), dst.stride(0) if dst is not None else 0, _p(dst_t),
          dst_t.stride(0) if dst_t is not None else 0, _s())


class CastTable:
    """device table for dl_cast_weights_batched: every bf16 shadow of a network refreshed by ONE launch.
    entries: (src f32 [R, C], dst | None, dst_t | None, dst_swiglu | None)"""

    def __init__(self, entries: list[tuple[Tensor, Tensor | None, Tensor | None, Tensor | None]]) -> None:
        import ctypes

        class Desc(ctypes.Structure):
            _fields_ = [("src", ctypes.c_void_p), ("R", ctypes.c_int64), ("C", ctypes.c_int64), ("dst", ctypes.c_void_p),
                        ("ld_dst", ctypes.c_int64), ("dst_t", ctypes.c_void_p), ("ld_t", ctypes.c_int64),
                        ("dst_swiglu", ctypes.c_void_p), ("ld_swiglu", ctypes.c_int64), ("tile_begin", ctypes.c_int64),
                        ("tiles_c", ctypes.c_int64)]

        for i, (src, dst, dst_t, dst_g) in enumerate(entries):
            # the kernel's SwiGLU row map works on whole 32-row groups (16 x1 rows, then the 16 x3 rows of the same hidden units): at
            # F = R / 2 not a multiple of 16 it leaves the destination's 2 F rows (dl_cast_weight_swiglu refuses such an F too)
            if dst_g is not None and (src.dim() != 2 or src.shape[0] % 32 != 0):
                raise ValueError(f"CastTable: entry {i} has a SwiGLU destination, its source {tuple(src.shape)} needs rows % 32 == 0")
        arr = (Desc * len(entries))()
        tiles = 0
        self.keep = entries  # the table holds raw pointers: keep the tensors alive
        for i, (src, dst, dst_t, dst_g) in enumerate(entries):
            R, C = src.shape
            assert src.is_contiguous() and src.dtype == torch.float32
            cmax = max(C, dst.stride(0) if dst is not None else 0, dst_g.stride(0) if dst_g is not None else 0)
            rmax = max(R, dst_t.stride(0) if dst_t is not None else 0)
            tc, tr = (cmax + 31) // 32, (rmax + 31) // 32
            arr[i] = Desc(_p(src), R, C, _p(dst), dst.stride(0) if dst is not None else 0, _p(dst_t),
                          dst_t.stride(0) if dst_t is not None else 0, _p(dst_g), dst_g.stride(0) if dst_g is not None else 0,
                          tiles, tc)
            tiles += tc * tr
        self.n, self.tiles = len(entries), tiles
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.dev = host.to(entries[0][0].device)

    def run(self) -> None:
        _call("dl_cast_weights_batched", _p(self.dev), self.n, self.tiles, _s())


class ConvCastTable:
    """device table for dl_cast_conv3x3_weights_batched: the forward / data-gradient shadows of every 3x3 convolution weight of a
    network refreshed by ONE launch.  entries: (w f32 [Co, Ci, 3, 3], wf [Co, 9 Ci], wd [Ci, 9 Co]); `accepts` says which weights fit"""

    @staticmethod
    def accepts(w: Tensor, wf: Tensor, wd: Tensor) -> bool:
        co, ci = w.shape[0], w.shape[1]
        return co % 32 == 0 and ci % 32 == 0 and wf.stride(0) == 9 * ci and wd.stride(0) == 9 * co

    def __init__(self, entries: list[tuple[Tensor, Tensor, Tensor]]) -> None:
        import ctypes

        class Desc(ctypes.Structure):
            _fields_ = [("w", ctypes.c_void_p), ("Co", ctypes.c_int64), ("Ci", ctypes.c_int64), ("wf", ctypes.c_void_p),
                        ("ldf", ctypes.c_int64), ("wd", ctypes.c_void_p), ("ldd", ctypes.c_int64), ("tile_begin", ctypes.c_int64)]

        arr = (Desc * len(entries))()
        tiles = 0
        self.keep = entries  # the table holds raw pointers: keep the tensors alive
        for i, (w, wf, wd) in enumerate(entries):
            assert w.is_contiguous() and w.dtype == torch.float32 and self.accepts(w, wf, wd)
            co, ci = w.shape[0], w.shape[1]
            arr[i] = Desc(_p(w), co, ci, _p(wf), wf.stride(0), _p(wd), wd.stride(0), tiles)
            tiles += (co // 32) * (ci // 32)
        self.n, self.tiles = len(entries), tiles
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.dev = host.to(entries[0][0].device)

    def run(self) -> None:
        _call("dl_cast_conv3x3_weights_batched", _p(self.dev), self.n, self.tiles, _s())


class ConvFoldTable:
    """device table for dl_conv3x3_wgrad_fold_batched: every staged convolution weight gradient (g f32 [9 Ci, ldg], transposed as
    dl_conv3x3_wgrad_tn leaves it, or f32 [n_img, 9 Ci, ldg]: the partial images of dl_conv3x3_wgrad_tn_parts, added in image
    order) folded into its [Co, Ci, 3, 3] gradient by ONE launch.  entries: (g, dw)"""

    TAP_SPLIT_MIN_IMAGES = 8  # DL_FOLD_TAP_SPLIT_MIN_IMAGES of include/diffulab_hip.h

    @staticmethod
    def accepts(co: int, ci: int) -> bool:
        return co % 32 == 0 and ci % 32 == 0

    def __init__(self, entries: list[tuple[Tensor, Tensor]]) -> None:
        import ctypes

        class Desc(ctypes.Structure):
            _fields_ = [("g", ctypes.c_void_p), ("ldg", ctypes.c_int64), ("dw", ctypes.c_void_p), ("Co", ctypes.c_int64),
                        ("Ci", ctypes.c_int64), ("tile_begin", ctypes.c_int64), ("n_img", ctypes.c_int64), ("img_stride", ctypes.c_int64)]

        arr = (Desc * len(entries))()
        tiles = 0
        self.keep = entries  # the table holds raw pointers: keep the tensors alive
        for i, (g, dw) in enumerate(entries):
            co, ci = dw.shape[0], dw.shape[1]
            assert dw.is_contiguous() and dw.dtype == torch.float32 and g.dtype == torch.float32 and self.accepts(co, ci)
            if g.dim() == 3:  # partial images
                assert g.shape[1] >= 9 * ci and g.stride(1) >= co
                arr[i] = Desc(_p(g), g.stride(1), _p(dw), co, ci, tiles, g.shape[0], g.stride(0))
                if g.shape[0] >= self.TAP_SPLIT_MIN_IMAGES:  # one tap of a channel tile per workgroup, 16-byte loads
                    assert g.stride(1) % 4 == 0 and g.stride(0) % 4 == 0 and _p(g) % 16 == 0
                    tiles += 8 * (co // 32) * (ci // 32)
            else:
                assert g.shape[0] >= 9 * ci and g.stride(0) >= co
                arr[i] = Desc(_p(g), g.stride(0), _p(dw), co, ci, tiles, 0, 0)
            tiles += (co // 32) * (ci // 32)
        self.n, self.tiles = len(entries), tiles
        host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.dev = host.to(entries[0][0].device)

    def run(self, clear: bool = True) -> None:
        _call("dl_conv3x3_wgrad_fold_batched", _p(self.dev), self.n, self.tiles, int(clear), _s())


def cast_weight_swiglu(src, dst):
    _call("dl_cast_weight_swiglu", _p(src), src.shape[0] // 2, src.shape[1], _p(dst), dst.stride(0), _s())


def cast_f32_to_bf16(src, dst):
    _call("dl_cast_f32_to_bf16", _p(src), _p(dst), src.numel(), _s())


def cast2d_f32_to_bf16(src, dst):
    """dst[r, c] = bf16(src[r, c]) over 2-D views whose rows may be windows of wider rows"""
    _call("dl_cast2d_f32_to_bf16", _p(src), src.stride(0), _p(dst), dst.stride(0), src.shape[0], src.shape[1], _s())


def cast_bf16_to_f32(src, dst):
    _call("dl_cast_bf16_to_f32", _p(src), _p(dst), src.numel(), _s())


def ema_update(ema, p, beta):
    _call("dl_ema_update", _p(ema), _p(p), float(beta), p.numel(), _s())


EMA_MAX_PROFILES, LINCOMB_MAX_SOURCES, LINCOMB_ACCUMULATE = 4, 256, 1


def ema_update_multi(emas, p, weights):
    """one launch: ema_k = fma(w_k, p - ema_k, ema_k) for up to four f32 buffers `emas` of p's size; `weights` are the w_k = 1 - beta_k
    (formed in fp64 by the caller, rounded to f32 here)"""
    K = len(emas)
    if not 1 <= K <= EMA_MAX_PROFILES or len(weights) != K:
        raise RuntimeError(f"dl_ema_update_multi takes 1 .. {EMA_MAX_PROFILES} profiles and one weight each (got {K} and {len(weights)})")
    for e in emas:
        if e.dtype != torch.float32 or p.dtype != torch.float32 or not e.is_contiguous() or not p.is_contiguous() or e.numel() != p.numel():
            raise RuntimeError("dl_ema_update_multi takes contiguous f32 tensors of one size")
    ptrs = [_p(e) for e in emas] + [None] * (EMA_MAX_PROFILES - K)
    ws = [float(w) for w in weights] + [0.0] * (EMA_MAX_PROFILES - K)
    _call("dl_ema_update_multi", *ptrs, _p(p), K, *ws, p.numel(), _s())


def arena_lincomb(out, srcs, weights, accumulate: bool = False):
    """one launch: out = [out +] sum_k weights[k] * srcs[k], one f32 multiply-add chain per element in the order of `srcs`; f32
    contiguous tensors of out's size, 16-byte aligned.  The two tables (addresses, weights) are built here, host and device copy"""
    K = len(srcs)
    if not 1 <= K <= LINCOMB_MAX_SOURCES or len(weights) != K:
        raise RuntimeError(f"dl_arena_lincomb takes 1 .. {LINCOMB_MAX_SOURCES} sources and one weight each (got {K} and {len(weights)})")
    for s in (out, *srcs):
        if s.dtype != torch.float32 or not s.is_contiguous() or s.numel() != out.numel():
            raise RuntimeError("dl_arena_lincomb takes contiguous f32 tensors of one size")
    ptr_host = torch.tensor([_p(s) for s in srcs], dtype=torch.int64)
    w_host = torch.from_numpy(np.asarray(weights, dtype=np.float64).astype(np.float32))
    ptr_dev, w_dev = keep(ptr_host.to(out.device)), keep(w_host.to(out.device))
    keep(ptr_host), keep(w_host)
    _call("dl_arena_lincomb", _p(out), ptr_host.data_ptr(), _p(ptr_dev), w_host.data_ptr(), _p(w_dev), K, out.numel(),
          LINCOMB_ACCUMULATE if accumulate else 0, _s())
    return out


# ------------------------------------------------------------------ UNet kernels (NHWC bf16 token rows)
def nchw_to_nhwc(x, out, B, C, HW):
    _call("dl_nchw_to_nhwc", _p(x), _p(out), B, C, HW, out.stride(0), _s())


def nhwc_to_nchw(x, out, B, C, HW):
    _call("dl_nhwc_to_nchw", _p(x), _p(out), B, C, HW, x.stride(0), _s())


def gn_stats(x, stats, B, HW, C, G=32, eps=1e-5):
    _call("dl_gn_stats", _p(x), _p(stats), B, HW, C, G, float(eps), _s())


def gn_apply_fwd(x, stats, w, b, film_scale, film_shift, silu, out, B, HW, C, G=32):
    _call("dl_gn_apply_fwd", _p(x), _p(stats), _p(w), _p(b), _p(film_scale), _p(film_shift),
          film_scale.stride(0) if film_scale is not None else 0, int(silu), _p(out), B, HW, C, G, _s())


def gn_fwd(x, stats, w, b, film_scale, film_shift, silu, out, B, HW, C, G=32, eps=1e-5):
    """statistics (written to `stats`) + normalise / FiLM / SiLU in one call"""
    _call("dl_gn_fwd", _p(x), _p(w), _p(b), _p(film_scale), _p(film_shift), film_scale.stride(0) if film_scale is not None else 0,
          int(bool(silu)), _p(out), _p(stats), B, HW, C, G, float(eps), _s())


def gn_bwd(dout, x, stats, w, b, film_scale, film_shift, silu, dres, dx, dw, db, dfilm_scale, dfilm_shift, scratch, B, HW, C,
           G=32):
    _call("dl_gn_bwd", _p(dout), _p(x), _p(stats), _p(w), _p(b), _p(film_scale), _p(film_shift),
          film_scale.stride(0) if film_scale is not None else 0, int(silu), _p(dres), _p(dx), _p(dw), _p(db), _p(dfilm_scale),
          _p(dfilm_shift), dfilm_scale.stride(0) if dfilm_scale is not None else 0, _p(scratch), B, HW, C, G, _s())


def im2col3x3(x, cols, B, H, W, C):
    _call("dl_im2col3x3", _p(x), x.stride(0), _p(cols), B, H, W, C, cols.shape[0], cols.stride(0), _s())


def _maybe(name: str, *args) -> bool:
    """call an entry point that may answer DL_ERR_UNSUPPORTED (-3): False then, True on success"""
    fn = getattr(lib().cdll, name)
    rc = fn(*args)
    if rc == -3:
        return False
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc}): {lib().cdll.dl_last_error().decode()}")
    if _REC is not None:
        _REC.calls.append((fn, args))
    return True


def conv3x3_nt(x, B, H, W, ci, wf, out, co, bias, resid, zero, scratch=None) -> bool:
    """implicit-GEMM 3x3 conv (forward, or data gradient with the rotated shadow); `scratch` (f32; the library splits K into as many
    partial images of B*H*W*co floats as it holds, up to eight) lets the low-resolution levels split K.  False -> use im2col3x3 +
    gemm_nt"""
    assert scratch is None or scratch.dtype == torch.float32
    return _maybe("dl_conv3x3_nt", _p(x), x.stride(0), B, H, W, ci, _p(wf), wf.stride(0), _p(out), out.stride(0), co, _p(bias),
                  _p(resid), resid.stride(0) if resid is not None else 0, _p(zero), _p(scratch),
                  scratch.numel() if scratch is not None else 0, _s())


def conv3x3_wgrad_tn(x, B, H, W, ci, dy, co, g, zero, max_wgs: int = 0) -> bool:
    """implicit-GEMM transposed weight gradient g[(tap, ci), co] +=; max_wgs > 0 caps the persistent workgroups (side-stream
    launches beside the convolution chain); False -> use im2col3x3 + gemm_tn"""
    return _maybe("dl_conv3x3_wgrad_tn", _p(x), x.stride(0), B, H, W, ci, _p(dy), dy.stride(0), dy.shape[0], co, _p(g),
                  g.stride(0), _p(zero), int(max_wgs), _s())


def conv3x3_wgrad_nparts(H: int, W: int, ci: int, co: int, R: int, max_wgs: int = 0) -> int:
    """partial images dl_conv3x3_wgrad_tn_parts writes for this shape and map on this device (0: shape not supported)"""
    return int(lib().cdll.dl_conv3x3_wgrad_tn_nparts(H, W, ci, co, R, int(max_wgs)))


def conv3x3_wgrad_tn_parts(x, B, H, W, ci, dy, co, g, zero, max_wgs: int = 0) -> None:
    """the transposed weight gradient as partial images g[s] f32 [n_parts, 9 ci (padded), co]: plain stores, no atomics; folded in a
    fixed order by ConvFoldTable"""
    _call("dl_conv3x3_wgrad_tn_parts", _p(x), x.stride(0), B, H, W, ci, _p(dy), dy.stride(0), dy.shape[0], co, _p(g), g.stride(1),
          g.stride(0), g.shape[0], _p(zero), int(max_wgs), _s())


def cast_conv3x3_weight(w, wf, wd):
    _call("dl_cast_conv3x3_weight", _p(w), w.shape[0], w.shape[1], _p(wf), wf.stride(0), _p(wd), wd.stride(0), _s())


def conv3x3_wgrad_fold(g, dw):
    _call("dl_conv3x3_wgrad_fold", _p(g), g.stride(0), _p(dw), dw.shape[0], dw.shape[1], _s())


def reduce2x2(x, out, B, Ho, Wo, C, scale):
    _call("dl_reduce2x2", _p(x), _p(out), B, Ho, Wo, C, float(scale), _s())


def expand2x2(x, out, B, Hi, Wi, C, scale):
    _call("dl_expand2x2", _p(x), _p(out), B, Hi, Wi, C, float(scale), _s())


def resample2x2_pair(x0, out0, x1, out1, B, Hs, Ws, C, scale, expand: bool):
    """reduce2x2 / expand2x2 of two tensors of the same geometry (Hs x Ws = the small map) in one launch"""
    _call("dl_resample2x2_pair", _p(x0), _p(out0), _p(x1), _p(out1), B, Hs, Ws, C, float(scale), int(expand), _s())


def pick2x2(x, out, B, Ho, Wo, C):
    _call("dl_pick2x2", _p(x), _p(out), B, Ho, Wo, C, _s())


def stuff2x2(dy, out, B, Hi, Wi, C):
    _call("dl_stuff2x2", _p(dy), _p(out), B, Hi, Wi, C, _s())


def rowbias_add(x, e, out, B, HW, C):
    _call("dl_rowbias_add", _p(x), _p(e), e.stride(0), _p(out), B, HW, C, _s())


def rowbias_bwd(dy, de, B, HW, C):
    _call("dl_rowbias_bwd", _p(dy), _p(de), de.stride(0), B, HW, C, _s())


def attn_small_fwd(q, k, v, out, probs, B, n, H, dh):
    _call("dl_attn_small_fwd", _p(q), _p(k), _p(v), q.stride(0), k.stride(0), _p(out), out.stride(0), _p(probs), B, n, H, dh,
          float(dh) ** -0.5, _s())


def attn_small_bwd(q, k, v, dout, probs, dq, dk, dv, B, n, H, dh):
    assert dq.stride(0) == q.stride(0) and dk.stride(0) == k.stride(0) == dv.stride(0) == v.stride(0)
    _call("dl_attn_small_bwd", _p(q), _p(k), _p(v), q.stride(0), k.stride(0), _p(dout), dout.stride(0), _p(probs), _p(dq),
          _p(dk), _p(dv), B, n, H, dh, float(dh) ** -0.5, _s())


def attn_cross_fwd(q, k, v, key_bias, out, probs, B, Nq, L, H, dh):
    """TransformerBlock cross-attention core (dl_attn_cross_fwd): q [B*Nq, >= H*dh], k / v [B*L, ...] bf16 rows, key_bias f32 [B, L] or None"""
    _call("dl_attn_cross_fwd", _p(q), _p(k), _p(v), q.stride(0), k.stride(0), _p(key_bias), _p(out), out.stride(0), _p(probs), B, Nq,
          L, H, dh, float(dh) ** -0.5, _s())


def attn_cross_bwd(q, k, v, key_bias, dout, probs, ds, dq, dk, dv, B, Nq, L, H, dh):
    """ds: f32 scratch [B, H, Nq, L]"""
    assert dq.stride(0) == q.stride(0) and dk.stride(0) == k.stride(0) == dv.stride(0) == v.stride(0)
    _call("dl_attn_cross_bwd", _p(q), _p(k), _p(v), q.stride(0), k.stride(0), _p(key_bias), _p(dout), dout.stride(0), _p(probs), _p(ds),
          _p(dq), _p(dk), _p(dv), B, Nq, L, H, dh, float(dh) ** -0.5, _s())


def geglu_fwd(u, h):
    """u bf16 [M, 2F] (column windows allowed) -> h [M, F] = u[:, :F] * gelu(u[:, F:])"""
    M, F = h.shape[0], h.shape[1]
    _call("dl_geglu_fwd", _p(u), u.stride(0), _p(h), h.stride(0), M, F, _s())


def geglu_bwd(dh, u, du):
    M, F = dh.shape[0], dh.shape[1]
    _call("dl_geglu_bwd", _p(dh), dh.stride(0), _p(u), u.stride(0), _p(du), du.stride(0), M, F, _s())


def add_bf16(a, b, out):
    _call("dl_add_bf16", _p(a), _p(b), _p(out), a.numel(), _s())


def copy2d_bf16(src, dst, rows, cols):
    _call("dl_copy2d_bf16", _p(src), src.stride(0), _p(dst), dst.stride(0), rows, cols, _s())


def dropout_threshold(p: float) -> int:
    """T of dl_dropout: an element is dropped iff its 16-bit Philox half is below T = floor(p * 65536 + 0.5), so p is quantised to
    1 / 65536.  0 <= p < 1, anything else raises ValueError; T == 0 (p == 0, or below 2^-17) means no launch is needed."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout probability must satisfy 0 <= p < 1 (got {p!r})")
    return min(int(math.floor(p * 65536.0 + 0.5)), 65535)


def dropout_scale(p: float) -> float:
    """scale of dl_dropout: float32(1 / (1 - p)) formed in double, as nn.Dropout does"""
    dropout_threshold(p)
    return float(np.float32(1.0 / (1.0 - float(p))))


def dropout(x, out, rng_state, site: int, T: int, scale: float, resid=None, rows: int | None = None, cols: int | None = None):
    """out[r, c] = x[r, c] * (keep ? scale : 0) + (resid[r, c] if resid is given) over the [rows, cols] window of pitched bf16 or f32
    matrices of one dtype (out may be x); keep = the Philox mask of (rng_state = device int64[2] (seed, step), site, r * cols + c)"""
    rows = x.shape[0] if rows is None else rows
    cols = x.shape[1] if cols is None else cols
    if x.dtype not in (torch.bfloat16, torch.float32) or out.dtype != x.dtype or (resid is not None and resid.dtype != x.dtype):
        raise RuntimeError("dl_dropout takes bf16 or f32 tensors of one dtype")
    if rng_state.dtype != torch.int64 or rng_state.numel() != 2:
        raise RuntimeError("dl_dropout: rng_state is a device int64[2] tensor (seed, step)")
    _call("dl_dropout", _p(x), x.stride(0), _p(resid), 0 if resid is None else resid.stride(0), _p(out), out.stride(0), rows, cols,
          F32 if x.dtype == torch.float32 else BF16, _p(rng_state), site, T, scale, _s())
    return out


# ------------------------------------------------------------------ fp32-class regime (csrc/f32.hip, dl_f32_*)
class _F32Gemm(ctypes.Structure):
    _fields_ = [("A", ctypes.c_void_p), ("B", ctypes.c_void_p), ("C", ctypes.c_void_p), ("lda", ctypes.c_int64),
                ("ldb", ctypes.c_int64), ("ldc", ctypes.c_int64), ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64),
                ("trans_a", ctypes.c_int32), ("trans_b", ctypes.c_int32), ("batch1", ctypes.c_int64), ("batch2", ctypes.c_int64),
                ("stride_a1", ctypes.c_int64), ("stride_a2", ctypes.c_int64), ("stride_b1", ctypes.c_int64),
                ("stride_b2", ctypes.c_int64), ("stride_c1", ctypes.c_int64), ("stride_c2", ctypes.c_int64), ("alpha", ctypes.c_float),
                ("bias", ctypes.c_void_p), ("act", ctypes.c_int32), ("pre_out", ctypes.c_void_p), ("accumulate", ctypes.c_int32),
                ("scratch", ctypes.c_void_p), ("scratch_floats", ctypes.c_int64)]


def _addr(t, off: int = 0) -> int:
    """device address of element `off` of an f32 tensor (or of a raw int address)"""
    if isinstance(t, int):
        return t + 4 * off
    if not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError("dl_f32_* ops take f32 device tensors (no CPU fallback exists)")
    return t.data_ptr() + 4 * off


def f32_gemm(A, B, C, M: int, N: int, K: int, *, lda: int, ldb: int, ldc: int, ta: bool = False, tb: bool = False, a_off: int = 0,
             b_off: int = 0, c_off: int = 0, batch: tuple[int, int] = (1, 1), sa=(0, 0), sb=(0, 0), sc=(0, 0), alpha: float = 1.0,
             bias=None, act: int = ACT_NONE, pre_out=None, accumulate: bool = False, scratch=None) -> None:
    """C[M, N] = act(alpha * op(A) op(B) + bias) (+= with accumulate) on the exact-f32 MFMA; ta: A is [K, M]; tb: B is [K, N]
    (default: A [M, K], B [N, K] = torch Linear weight); *_off: element offsets into the tensors (column windows of token rows);
    batch = (b1, b2) with element strides sa / sb / sc per level"""
    d = _F32Gemm(_addr(A, a_off), _addr(B, b_off), _addr(C, c_off), lda, ldb, ldc, M, N, K, int(ta), int(tb), batch[0], batch[1],
                 sa[0], sa[1], sb[0], sb[1], sc[0], sc[1], float(alpha), _p(bias), act, _p(pre_out), int(accumulate),
                 _p(scratch), scratch.numel() if scratch is not None else 0)
    _call("dl_f32_gemm", ctypes.addressof(d), _s())


def f32_linear(x, w, out, *, bias=None, act: int = ACT_NONE, pre_out=None, M: int | None = None, scratch=None) -> None:
    """out[M, out_f] = act(x[M, in_f] w[out_f, in_f]^T + bias)   (nn.Linear forward); scratch: split-K partial images for products
    with few output tiles and a long contraction (the deep UNet levels' convolutions)"""
    M = x.shape[0] if M is None else M
    f32_gemm(x, w, out, M, w.shape[0], w.shape[1], lda=x.stride(0), ldb=w.stride(0), ldc=out.stride(0), bias=bias, act=act,
             pre_out=pre_out, scratch=scratch)


def f32_linear_dgrad(dy, w, dx, *, M: int | None = None, scratch=None) -> None:
    """dx[M, in_f] = dy[M, out_f] w[out_f, in_f]"""
    M = dy.shape[0] if M is None else M
    f32_gemm(dy, w, dx, M, w.shape[1], w.shape[0], lda=dy.stride(0), ldb=w.stride(0), ldc=dx.stride(0), tb=True, scratch=scratch)


def f32_linear_wgrad(dy, x, g, *, R: int | None = None, scratch=None) -> None:
    """g[out_f, in_f] += dy[R, out_f]^T x[R, in_f]"""
    R = dy.shape[0] if R is None else R
    f32_gemm(dy, x, g, g.shape[0], g.shape[1], R, lda=dy.stride(0), ldb=x.stride(0), ldc=g.stride(0), ta=True, tb=True,
             accumulate=True, scratch=scratch)


def f32_ln_modulate_fwd(x, w, b, scale, shift, rows_per_mod, eps, out, mean, rstd, t=None, gate=None, x_out=None):
    M, D = x.shape
    _call("dl_f32_ln_modulate_fwd", _p(x), _p(w), _p(b), _p(scale), _p(shift), scale.stride(0), rows_per_mod, float(eps), _p(out),
          _p(mean), _p(rstd), _p(t), _p(gate), gate.stride(0) if gate is not None else 0, _p(x_out), M, D, _s())


def f32_ln_modulate_bwd(dout, x, w, b, scale, rows_per_mod, mean, rstd, dres, dx, dscale, dshift, dwb_partial, gate_t=None,
                        gate=None, dt=None, dgate=None):
    M, D = x.shape
    _call("dl_f32_ln_modulate_bwd", _p(dout), _p(x), _p(w), _p(b), _p(scale), scale.stride(0), rows_per_mod, _p(mean), _p(rstd),
          _p(dres), _p(dx), _p(dscale), _p(dshift), dscale.stride(0), _p(dwb_partial), _p(gate_t), _p(gate),
          gate.stride(0) if gate is not None else 0, _p(dt), _p(dgate), M, D, _s())


def f32_qk_norm_rope_fwd(qkv, scale_q, scale_k, cos, sin, qk, rrms, B, N, H, dh, rot, eps=1e-6, pos=None):
    """pos: int32 [B*N] rotary table row of every token (SPRINT's kept tokens) or None"""
    _call("dl_f32_qk_norm_rope_fwd", _p(qkv), qkv.stride(0), _p(scale_q), _p(scale_k), _p(cos), _p(sin), _p(qk), _p(rrms), B, N, H, dh,
          rot, float(eps), _p(pos), _s())


def f32_qk_norm_rope_bwd(dqk, qkv, scale_q, scale_k, cos, sin, rrms, dqkv, partials, B, N, H, dh, rot, pos=None):
    _call("dl_f32_qk_norm_rope_bwd", _p(dqk), _p(qkv), qkv.stride(0), _p(scale_q), _p(scale_k), _p(cos), _p(sin), _p(rrms), _p(dqkv),
          dqkv.stride(0), _p(partials), B, N, H, dh, rot, _p(pos), _s())


def f32_gather_tokens(src, idx, dst, B, N, k, D, keep=None):
    """dst[b, j, :] = src[b, idx[b, j], :] on f32 rows: a bytewise row copy, i.e. dl_gather_tokens over 2 D two-byte columns"""
    _call("dl_gather_tokens", _p(src), 2 * src.stride(0), _p(idx), _p(keep), _p(dst), 2 * dst.stride(0), B, N, k, 2 * D, _s())


def f32_scatter_tokens_add(src, idx, dst, B, N, k, D):
    _call("dl_f32_scatter_tokens_add", _p(src), src.stride(0), _p(idx), _p(dst), dst.stride(0), B, N, k, D, _s())


def f32_restore_tokens(xd, inv, mask, out, B, N, k, D):
    _call("dl_f32_restore_tokens", _p(xd), xd.stride(0), _p(inv), _p(mask), _p(out), out.stride(0), B, N, k, D, _s())


def f32_masked_colsum(x, sel, out, R, C, scratch):
    """out[c] += sum over rows with sel[row] < 0 of x[row, c]: partial images per 256-row slab in `scratch`, fixed-order fold"""
    slabs = min(512, (R + 255) // 256)
    assert scratch.numel() >= slabs * C
    _call("dl_f32_masked_colsum_partials", _p(x), x.stride(0), _p(sel), _p(scratch), slabs, R, C, _s())
    reduce_rows_batched_f32(scratch, 0, out, 0, 1, slabs, C)


def f32_ddt_cond_fwd(enc, temb, B, N, out):
    _call("dl_f32_ddt_cond_fwd", _p(enc), enc.stride(0), _p(temb), temb.stride(0), B, N, enc.shape[1], _p(out), _s())


def f32_ddt_cond_bwd(dsz, enc, temb, B, N, denc, dtemb):
    _call("dl_f32_ddt_cond_bwd", _p(dsz), _p(enc), enc.stride(0), _p(temb), temb.stride(0), B, N, enc.shape[1], _p(denc), _p(dtemb), _s())


def f32_gated_residual_fwd(x, t, gate, rows_per_mod, out):
    M, D = x.shape
    _call("dl_f32_gated_residual_fwd", _p(x), _p(t), _p(gate), gate.stride(0), rows_per_mod, _p(out), out.stride(0), M, D, _s())


def f32_gate_bwd(dout, t, gate, rows_per_mod, dt, dgate):
    M, D = dout.shape
    _call("dl_f32_gate_bwd", _p(dout), _p(t), _p(gate), gate.stride(0), rows_per_mod, _p(dt), _p(dgate), dgate.stride(0), M, D, _s())


def f32_attn_fwd(q, k, v, out, probs, B, n, H, dh):
    """AttentionBlock core (unet.py:311-318) over f32 token rows for ANY token count / head width: heads are dh-wide column blocks of
    the rows (addressed by stride in the batched GEMMs); probs f32 [B, H, n, n] = softmax(scale Q K^T) is kept for the backward"""
    sc = float(dh) ** -0.5
    f32_gemm(q, k, probs, n, n, dh, lda=q.stride(0), ldb=k.stride(0), ldc=n, batch=(B, H), sa=(n * q.stride(0), dh),
             sb=(n * k.stride(0), dh), sc=(H * n * n, n * n), alpha=sc)
    f32_softmax_fwd(probs, B * H * n, n)
    f32_gemm(probs, v, out, n, dh, n, lda=n, ldb=v.stride(0), ldc=out.stride(0), tb=True, batch=(B, H), sa=(H * n * n, n * n),
             sb=(n * v.stride(0), dh), sc=(n * out.stride(0), dh))


def f32_attn_bwd(q, k, v, dout, probs, dP, dq, dk, dv, B, n, H, dh):
    """dP: f32 scratch [B, H, n, n] (overwritten: dP, then dS)"""
    sc = float(dh) ** -0.5
    pb, hb = (H * n * n, n * n), dict(batch=(B, H))
    f32_gemm(dout, v, dP, n, n, dh, lda=dout.stride(0), ldb=v.stride(0), ldc=n, sa=(n * dout.stride(0), dh),
             sb=(n * v.stride(0), dh), sc=pb, **hb)                                                   # dP = dO V^T
    f32_gemm(probs, dout, dv, n, dh, n, lda=n, ldb=dout.stride(0), ldc=dv.stride(0), ta=True, tb=True, sa=pb,
             sb=(n * dout.stride(0), dh), sc=(n * dv.stride(0), dh), **hb)                            # dV = P^T dO
    f32_softmax_bwd(probs, dP, B * H * n, n)                                                          # dS over dP
    f32_gemm(dP, k, dq, n, dh, n, lda=n, ldb=k.stride(0), ldc=dq.stride(0), tb=True, sa=pb, sb=(n * k.stride(0), dh),
             sc=(n * dq.stride(0), dh), alpha=sc, **hb)                                               # dQ = scale dS K
    f32_gemm(dP, q, dk, n, dh, n, lda=n, ldb=q.stride(0), ldc=dk.stride(0), ta=True, tb=True, sa=pb,
             sb=(n * q.stride(0), dh), sc=(n * dk.stride(0), dh), alpha=sc, **hb)                     # dK = scale dS^T Q


def f32_softmax_fwd(s, rows, cols):
    _call("dl_f32_softmax_fwd", _p(s), rows, cols, _s())


def f32_softmax_bwd(p, dp, rows, cols):
    _call("dl_f32_softmax_bwd", _p(p), _p(dp), rows, cols, _s())


def f32_softmax_keymask_fwd(s, key_bias, B, rows_per_sample, cols):
    _call("dl_f32_softmax_keymask_fwd", _p(s), _p(key_bias), B, rows_per_sample, cols, _s())


def f32_xattn_fwd(q, k, v, key_bias, out, probs, B, Nq, L, H, dh):
    """masked cross-attention core (unet.py:306-318 with a context) over f32 token rows: Nq query rows, L context rows per sample, any
    sizes; probs f32 [B, H, Nq, L] kept for the backward (f32_attn_bwd's batched GEMMs with the two token counts)"""
    sc = float(dh) ** -0.5
    f32_gemm(q, k, probs, Nq, L, dh, lda=q.stride(0), ldb=k.stride(0), ldc=L, batch=(B, H), sa=(Nq * q.stride(0), dh),
             sb=(L * k.stride(0), dh), sc=(H * Nq * L, Nq * L), alpha=sc)
    f32_softmax_keymask_fwd(probs, key_bias, B, H * Nq, L)
    f32_gemm(probs, v, out, Nq, dh, L, lda=L, ldb=v.stride(0), ldc=out.stride(0), tb=True, batch=(B, H), sa=(H * Nq * L, Nq * L),
             sb=(L * v.stride(0), dh), sc=(Nq * out.stride(0), dh))


def f32_xattn_bwd(q, k, v, dout, probs, dP, dq, dk, dv, B, Nq, L, H, dh):
    """dP: f32 scratch [B, H, Nq, L] (overwritten: dP, then dS).  Masked keys have P = 0, hence dS = 0 and zero dK / dV rows"""
    sc = float(dh) ** -0.5
    pb, hb = (H * Nq * L, Nq * L), dict(batch=(B, H))
    f32_gemm(dout, v, dP, Nq, L, dh, lda=dout.stride(0), ldb=v.stride(0), ldc=L, sa=(Nq * dout.stride(0), dh),
             sb=(L * v.stride(0), dh), sc=pb, **hb)                                                   # dP = dO V^T
    f32_gemm(probs, dout, dv, L, dh, Nq, lda=L, ldb=dout.stride(0), ldc=dv.stride(0), ta=True, tb=True, sa=pb,
             sb=(Nq * dout.stride(0), dh), sc=(L * dv.stride(0), dh), **hb)                           # dV = P^T dO
    f32_softmax_bwd(probs, dP, B * H * Nq, L)                                                         # dS over dP
    f32_gemm(dP, k, dq, Nq, dh, L, lda=L, ldb=k.stride(0), ldc=dq.stride(0), tb=True, sa=pb, sb=(L * k.stride(0), dh),
             sc=(Nq * dq.stride(0), dh), alpha=sc, **hb)                                              # dQ = scale dS K
    f32_gemm(dP, q, dk, L, dh, Nq, lda=L, ldb=q.stride(0), ldc=dk.stride(0), ta=True, tb=True, sa=pb,
             sb=(Nq * q.stride(0), dh), sc=(L * dk.stride(0), dh), alpha=sc, **hb)                    # dK = scale dS^T Q


def f32_geglu_fwd(u, h):
    _call("dl_f32_geglu_fwd", _p(u), _p(h), u.shape[0], h.shape[1], _s())


def f32_geglu_bwd(dh, u, du):
    _call("dl_f32_geglu_bwd", _p(dh), _p(u), _p(du), u.shape[0], dh.shape[1], _s())


def f32_swiglu_fwd(u, h):
    _call("dl_f32_swiglu_fwd", _p(u), _p(h), u.shape[0], h.shape[1], _s())


def f32_swiglu_bwd(dh, u, du):
    _call("dl_f32_swiglu_bwd", _p(dh), _p(u), _p(du), u.shape[0], dh.shape[1], _s())


def f32_add(a, b, out):
    _call("dl_f32_add", _p(a), _p(b), _p(out), a.numel(), _s())


def f32_silu_bwd(dy, pre, dx):
    _call("dl_f32_silu_bwd", _p(dy), _p(pre), _p(dx), dy.numel(), _s())


def f32_patchify(x, tok, p, order):
    B, C, H, W = x.shape
    _call("dl_f32_patchify", _p(x), _p(tok), B, C, H, W, p, tok.stride(0), order, _s())


def f32_timestep_embedding(t, out, max_period=10000.0):
    _call("dl_f32_timestep_embedding", _p(t), _p(out), out.shape[0], out.shape[1], float(max_period), _s())


def f32_cond_combine_fwd(e, table, idx, emb, act):
    _call("dl_f32_cond_combine_fwd", _p(e), _p(table), _p(idx), _p(emb), _p(act), e.shape[0], e.shape[1], _s())


def f32_cond_combine_bwd(dact, emb, idx, demb, dtable):
    _call("dl_f32_cond_combine_bwd", _p(dact), _p(emb), _p(idx), _p(demb), _p(dtable), dact.shape[0], dact.shape[1], _s())


# ---- fp32-class regime of the UNet: same call shapes as the bf16 wrappers above (unet_engine_f32.py swaps them in by name)
def f32_im2col3x3(x, cols, B, H, W, C):
    _call("dl_f32_im2col3x3", _p(x), x.stride(0), _p(cols), B, H, W, C, _s())


def f32_col2im3x3(dcols, dx, B, H, W, C):
    _call("dl_f32_col2im3x3", _p(dcols), _p(dx), dx.stride(0), B, H, W, C, _s())


def f32_gn_stats(x, stats, B, HW, C, G=32, eps=1e-5):
    _call("dl_f32_gn_stats", _p(x), _p(stats), B, HW, C, G, float(eps), _s())


def f32_gn_apply_fwd(x, stats, w, b, film_scale, film_shift, silu, out, B, HW, C, G=32):
    _call("dl_f32_gn_apply_fwd", _p(x), _p(stats), _p(w), _p(b), _p(film_scale), _p(film_shift),
          film_scale.stride(0) if film_scale is not None else 0, int(silu), _p(out), B, HW, C, G, _s())


def f32_gn_bwd(dout, x, stats, w, b, film_scale, film_shift, silu, dres, dx, dw_partial, db_partial, dfilm_scale, dfilm_shift, B, HW, C,
               G=32):
    assert dfilm_scale is None or dfilm_scale.stride(0) == film_scale.stride(0)
    _call("dl_f32_gn_bwd", _p(dout), _p(x), _p(stats), _p(w), _p(b), _p(film_scale), _p(film_shift),
          film_scale.stride(0) if film_scale is not None else 0, int(silu), _p(dres), _p(dx), _p(dw_partial), _p(db_partial),
          _p(dfilm_scale), _p(dfilm_shift), B, HW, C, G, _s())


def f32_resample2x2(x, out, B, Hs, Ws, C, scale, mode):
    _call("dl_f32_resample2x2", _p(x), _p(out), B, Hs, Ws, C, float(scale), mode, _s())


def f32_nchw_to_nhwc(x, out, B, C, HW):
    _call("dl_f32_nchw_to_nhwc", _p(x), _p(out), B, C, HW, out.stride(0), _s())


def f32_nhwc_to_nchw(x, out, B, C, HW):
    _call("dl_f32_nhwc_to_nchw", _p(x), _p(out), B, C, HW, x.stride(0), _s())


def f32_copy2d(src, dst, rows, cols):
    _call("dl_f32_copy2d", _p(src), src.stride(0), _p(dst), dst.stride(0), rows, cols, _s())


def f32_rowbias_add(x, e, out, B, HW, C):
    _call("dl_f32_rowbias_add", _p(x), _p(e), e.stride(0), _p(out), B, HW, C, _s())


def f32_rowbias_bwd(dy, de, B, HW, C):
    _call("dl_f32_rowbias_bwd", _p(dy), _p(de), de.stride(0), B, HW, C, _s())


def low_priority_stream(device) -> "torch.cuda.Stream":
    """torch stream object over a HIP stream of the device's lowest priority"""
    handle = ctypes.c_void_p()
    rng = (ctypes.c_int * 2)()
    with torch.cuda.device(device):
        lib().call("dl_stream_create_low_priority", ctypes.byref(handle), rng)
    st = torch.cuda.ExternalStream(handle.value, device=device)
    st.priority_range = (rng[0], rng[1])
    return st


def masked_stream(pattern: str, device) -> "torch.cuda.Stream":
    """torch stream object over a CU-masked HIP stream; pattern "i<k>" enables every k-th CU, "b<n>" the first n CUs"""
    import ctypes

    n_cu = torch.cuda.get_device_properties(device).multi_processor_count
    if pattern[0] == "i":
        bits = [i % int(pattern[1:]) == 0 for i in range(n_cu)]
    elif pattern[0] == "b":
        bits = [i < int(pattern[1:]) for i in range(n_cu)]
    else:
        raise ValueError(f"unknown CU mask pattern {pattern!r}")
    words = (n_cu + 31) // 32
    arr = (ctypes.c_uint32 * words)()
    for i, on in enumerate(bits):
        if on:
            arr[i // 32] |= 1 << (i % 32)
    handle = ctypes.c_void_p()
    with torch.cuda.device(device):
        lib().call("dl_stream_create_masked", arr, words, ctypes.byref(handle))
    return torch.cuda.ExternalStream(handle.value, device=device)
