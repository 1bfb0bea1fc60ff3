"""Variable-step Adams-Bashforth 2 for rectified flow (this project's; the reference's flow samplers are first order) on the HIP
`dl_ab2_step` kernel: one forward per step, second order from the second step on.

The ODE dx/dt = v(x, t) is integrated in t itself, not in log-SNR as DPM-Solver++ does for Gaussian diffusion: with alpha = 1 - t,
sigma = t the half-log-SNR log(alpha / sigma) is infinite at both ends of the grid, and first-order DPM-Solver++ on this path is the
Euler step anyway.  AB2 on v has no singular point (Hairer, Norsett & Wanner, "Solving Ordinary Differential Equations I", III.5)."""

from __future__ import annotations

from torch import Tensor

from .... import ops
from ..common import StepResult
from .euler import FlowSampler, flow_refuses_threshold


class AB2(FlowSampler):
    name = "ab2"
    multistep = True

    def __init__(self) -> None:
        super().__init__()
        self._last: tuple[Tensor, float, float] | None = None  # (the kernel's v_out, the t_prev it stepped to, its dt)

    def set_steps(self, timesteps: list[float]) -> None:
        self.reset()

    def reset(self) -> None:
        self._last = None

    def history(self, x_t: Tensor, t_curr: float) -> tuple[Tensor, float] | None:
        """(v_last, dt_last) where the previous call stepped to exactly this t_curr on a tensor of this shape and device, else None:
        the first step of a run, a repeated step of `resample` and a new batch are first order without the loops saying so"""
        if self._last is None:
            return None
        v_last, t_to, dt_last = self._last
        if t_to != t_curr or dt_last == 0.0 or v_last.shape != x_t.shape or v_last.device != x_t.device:
            return None
        return v_last, dt_last

    def step(self, x_t: Tensor, v: Tensor, t_curr: float, t_prev: float, v_uncond: Tensor | None = None,
             guidance_scale: float = 0.0, guidance_rescale: float = 0.0, dynamic_threshold: float | None = None,
             threshold_max: float | None = None) -> StepResult:
        """with dt = t_curr - t_prev, w = dt / (2 dt_last) and vc the CFG-combined (and rescaled) v:
        x_prev = x_t - dt ((1 + w) vc - w v_last) where `history` holds, else the Euler step x_t - dt vc; estimated_x0 = x_t - vc t_curr.
        The history is the kernel's own v_out, never the denoiser's output: the engines reuse their output buffers."""
        flow_refuses_threshold(dynamic_threshold, threshold_max)
        x = x_t.float().contiguous()
        v, vu = v.float().contiguous(), None if v_uncond is None else v_uncond.float().contiguous()
        mul = ops.cfg_rescale_coef(v, vu, guidance_scale, guidance_rescale) if guidance_rescale > 0 and vu is not None else None
        dt = t_curr - t_prev
        hist = self.history(x, t_curr)
        v_last, w = (None, 0.0) if hist is None else (hist[0], dt / (2.0 * hist[1]))
        x_prev, x0, v_out = ops.ab2_step(x, v, vu, guidance_scale, mul, v_last, t_curr, t_prev, w)
        self._last = (v_out, t_prev, dt)
        return StepResult(x_prev=x_prev, estimated_x0=x0)
