"""DDIM step (reference samplers/gaussian_diffusion/ddim.py:9-103) on the fused `dl_ddim_step` kernel."""

from __future__ import annotations

import torch
from torch import Tensor

from .... import ops
from ...utils import f32_table
from ..common import StepResult
from .ddpm import _MEAN, DDPM


class DDIM(DDPM):
    name = "ddim"

    def _ddim_tables(self, device: torch.device) -> tuple[Tensor, Tensor]:
        key = ("ddim", device)
        if key not in self._dev_tables:
            self._dev_tables[key] = f32_table(torch.stack([self.sqrt_alphas_bar, self.alphas_bar, self.alphas_bar_prev]), device)
            self._dev_tables[("ddim_c", device)] = f32_table(
                torch.stack([self.posterior_mean_coef1, self.posterior_mean_coef2]), device)
        return self._dev_tables[key], self._dev_tables[("ddim_c", device)]

    def step(self, model_prediction: Tensor, timesteps: Tensor, xt: Tensor, clamp_x: bool = False, eta: float = 0.0,
             prediction_uncond: Tensor | None = None, guidance_scale: float = 0.0, guidance_rescale: float = 0.0,
             dynamic_threshold: float | None = None, threshold_max: float | None = None) -> StepResult:
        self._variance_tables()  # same var_type validation as DDPM._get_p_mean_var (ddim.py:89)
        tab, coefs = self._ddim_tables(xt.device)
        if self.learned_variance:  # the 2C prediction's variance half is discarded (ddim.py:89); the mean half is read in place
            self._check_halves(model_prediction, xt)
        noise = torch.randn_like(xt)  # ddim.py:63
        pred, pu, x, t, mul, thr = self._guided(model_prediction, prediction_uncond, guidance_scale, xt, timesteps, tab, coefs,
                                                guidance_rescale, dynamic_threshold, threshold_max)
        mean_type, var_mode = _MEAN.index(self.mean_type), ops.VAR_MODES.get(self.var_type, ops.VAR_FIXED)
        if guidance_rescale > 0 or dynamic_threshold is not None:  # this project's: see `DDPM._guided`
            xp, x0, mean, std, lp = ops.ddim_step_g(pred, pu, guidance_scale, mul, thr, x, noise, t, tab, coefs, mean_type, var_mode,
                                                    clamp_x, eta)
        elif self.mean_type == "v":
            xp, x0, mean, std, lp = ops.ddim_step_v(pred, pu, guidance_scale, x, noise, t, tab, var_mode, clamp_x, eta)
        else:
            xp, x0, mean, std, lp = ops.ddim_step(pred, pu, guidance_scale, x, noise, t, tab, coefs, mean_type, clamp_x, eta,
                                                  halves=self.learned_variance)
        out = StepResult(x_prev=xp, estimated_x0=x0, x_prev_mean=mean)
        if eta > 0:
            out["x_prev_std"] = std
            out["logprob"] = lp
        return out
