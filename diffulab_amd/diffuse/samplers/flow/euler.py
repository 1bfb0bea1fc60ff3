"""Euler ODE step for rectified flow (reference samplers/flow/euler.py:22-41) on the HIP `dl_euler_step` kernel."""

from __future__ import annotations

from torch import Tensor

from .... import ops
from ..common import Sampler, StepResult


class FlowSampler(Sampler):
    name: str


def flow_refuses_threshold(dynamic_threshold, threshold_max) -> None:
    if dynamic_threshold is not None or threshold_max is not None:
        raise ValueError("dynamic_threshold is not available for flow samplers: the flow step has no per-step x0 clamp to replace")


class Euler(FlowSampler):
    name = "euler"

    def set_steps(self, timesteps: list[float]) -> None:
        pass

    def step(self, x_t: Tensor, v: Tensor, t_curr: float, t_prev: float, v_uncond: Tensor | None = None,
             guidance_scale: float = 0.0, guidance_rescale: float = 0.0, dynamic_threshold: float | None = None,
             threshold_max: float | None = None) -> StepResult:
        """x_prev = x_t - v (t_curr - t_prev); estimated_x0 = x_t - v t_curr.  `v_uncond` (extension) fuses the
        classifier-free combine v_u + g (v - v_u) of flow.py:257-259 into the same pass.  guidance_rescale (this project's): the
        combined v is scaled per sample by the CFG-rescale factor (Lin et al. 2023), computed on the device by one more launch."""
        flow_refuses_threshold(dynamic_threshold, threshold_max)
        if guidance_rescale > 0 and v_uncond is not None:
            v, vu = v.float().contiguous(), v_uncond.float().contiguous()
            mul = ops.cfg_rescale_coef(v, vu, guidance_scale, guidance_rescale)
            x_prev, x0 = ops.euler_step_g(x_t.float().contiguous(), v, vu, guidance_scale, mul, t_curr, t_prev)
            return StepResult(x_prev=x_prev, estimated_x0=x0)
        x_prev, x0 = ops.euler_step(x_t.float().contiguous(), v.float().contiguous(),
                                    None if v_uncond is None else v_uncond.float().contiguous(), guidance_scale,
                                    t_curr, t_prev)
        return StepResult(x_prev=x_prev, estimated_x0=x0)
