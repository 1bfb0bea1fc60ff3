"""DPM-Solver++(2M) (Lu et al., "DPM-Solver++: Fast Solver for Guided Sampling of Diffusion Probabilistic Models", 2022, alg. 2) for
the DDPM chains (this project's; the reference's Gaussian samplers are first order) on the HIP `dl_dpmpp_2m_step` kernel: one forward
per step, deterministic, second order in the half-log-SNR lambda = log(alpha / sigma) wherever the previous step's x0 is at hand.

The steps at index 1 and index 0 are always first order.  Index 0 sits at sigma = 0.01 on the linear 1000-step chain; on its 20-step
respacing the lambda step into index 0 is 2.92 where the steps before it are 0.26-0.66, so the 2M extrapolation weight 1 / (2 r)
would be 2.2, and the solver ends worse than DDIM at 10-40 steps (DESIGN.md has the figures)."""

from __future__ import annotations

import math

from torch import Tensor

from .... import ops
from ..common import StepResult
from .ddim import DDIM
from .ddpm import _MEAN


class DPMSolverPP2M(DDIM):
    name = "dpmpp_2m"
    multistep = True

    def __init__(self, mean_type: str = "epsilon", var_type: str = "fixed_small") -> None:
        if mean_type == "xprev":
            raise ValueError('dpmpp_2m takes mean_type epsilon, xstart or v: a posterior-mean output ("xprev") has no place in an ODE solver')
        super().__init__(mean_type=mean_type, var_type=var_type)
        self._last: tuple[Tensor, int] | None = None  # (the kernel's x0_est, the index of the step that wrote it)

    def set_steps(self, betas: Tensor) -> None:
        super().set_steps(betas)
        self._ab: list[float] = self.alphas_bar.tolist()  # fp64, the respaced chain's where respaced
        self.reset()

    def reset(self) -> None:
        self._last = None

    def history(self, xt: Tensor, step_index: int) -> Tensor | None:
        """x0_last where the previous call was the step at step_index + 1 on a tensor of this shape and device, else None: the first
        step of a run, a repeated step of `resample` and a new batch are first order without the loops saying so"""
        if self._last is None:
            return None
        x0_last, index = self._last
        if index != step_index + 1 or x0_last.shape != xt.shape or x0_last.device != xt.device:
            return None
        return x0_last

    def _lambda(self, i: int) -> float:
        ab = self._ab[i]
        return 0.5 * math.log(ab / (1.0 - ab))

    def coefficients(self, t: int, second_order: bool) -> tuple[float, float, float]:
        """(a, b, c) of x_prev = a x_t + b x0_t + c x0_last for the step at index t, in double.  second_order is honoured for
        2 <= t < T - 1 only (the chain's last index has no step before it); index -1 stands for alphas_bar = 1, so t == 0 returns
        (0, 1, 0) exactly."""
        if t == 0:
            return 0.0, 1.0, 0.0
        ab_t, ab_p = self._ab[t], self._ab[t - 1]
        h = self._lambda(t - 1) - self._lambda(t)
        a = math.sqrt(1.0 - ab_p) / math.sqrt(1.0 - ab_t)
        e = -math.sqrt(ab_p) * math.expm1(-h)
        if not second_order or t < 2 or t + 1 >= len(self._ab):
            return a, e, 0.0
        r = (self._lambda(t) - self._lambda(t + 1)) / h
        return a, e * (1.0 + 1.0 / (2.0 * r)), -e / (2.0 * r)

    def step(self, model_prediction: Tensor, timesteps: Tensor, xt: Tensor, clamp_x: bool = False,
             prediction_uncond: Tensor | None = None, guidance_scale: float = 0.0, guidance_rescale: float = 0.0,
             dynamic_threshold: float | None = None, threshold_max: float | None = None, step_index: int | None = None,
             eta: float = 0.0) -> StepResult:
        """step_index: the host integer every entry of `timesteps` holds (`GaussianDiffusion.one_step_denoise` passes it), so that
        the coefficients and the history rule need no device value.  x0 is formed as DDIM forms it (CFG combine, rescale, the
        mean_type's x0, dynamic threshold, clamp_x); estimated_x0 is that x0 and the next step's history, a tensor the kernel wrote.
        x_prev_mean holds x_prev's values in a tensor of its own (the step is deterministic: no x_prev_std, no logprob, no noise
        drawn), so that the in-place blend of the inpainting loop, which rewrites x_prev, leaves the recorded mean as the step made
        it.  eta: DDIM's keyword, accepted at 0 only -- this solver has no stochastic form here."""
        if eta != 0.0:
            raise ValueError(f"dpmpp_2m is deterministic: eta must be 0, got {eta!r} (the SDE variants of DPM-Solver++ are not built)")
        if step_index is None:
            raise ValueError("dpmpp_2m needs step_index, the host value of `timesteps`: its coefficients are formed on the host")
        t_idx = int(step_index)
        if not 0 <= t_idx < len(self._ab):
            raise ValueError(f"step_index {t_idx} outside the chain of {len(self._ab)} steps")
        self._variance_tables()  # same var_type validation as DDIM.step
        tab, _ = self._ddim_tables(xt.device)
        if self.learned_variance:  # the variance half is discarded, as DDIM discards it; the mean half is read in place
            self._check_halves(model_prediction, xt)
        pred, pu, x, t, mul, thr = self._guided(model_prediction, prediction_uncond, guidance_scale, xt, timesteps, tab, None,
                                                guidance_rescale, dynamic_threshold, threshold_max)
        x0_last = self.history(x, t_idx) if t_idx >= 2 else None
        a, b, c = self.coefficients(t_idx, x0_last is not None)
        xp, x0 = ops.dpmpp_2m_step(pred, pu, guidance_scale, mul, thr, x, x0_last, t, tab, _MEAN.index(self.mean_type),
                                   ops.VAR_MODES.get(self.var_type, ops.VAR_FIXED), clamp_x, a, b, c)
        self._last = (x0, t_idx)
        return StepResult(x_prev=xp, estimated_x0=x0, x_prev_mean=xp.clone())
