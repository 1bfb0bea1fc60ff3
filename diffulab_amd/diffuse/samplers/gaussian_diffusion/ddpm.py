"""DDPM ancestral step (reference samplers/gaussian_diffusion/ddpm.py:25-363) on the fused `dl_ddpm_step` kernel.

Host side keeps the fp64 schedule tables exactly as the reference builds them (ddpm.py:49-85); the kernel gets
their fp32 casts (what `extract_into_tensor(...).float()` would produce per call)."""

from __future__ import annotations

import torch
from torch import Tensor

from .... import ops
from ...utils import f32_table, quantile_position
from ..common import Sampler, StepResult

_MEAN = ("epsilon", "xstart", "xprev", "v")  # "v" (Salimans & Ho 2022) is this project's; the reference has the first three
_VAR = ("learned", "fixed_small", "fixed_large", "learned_range")


class GaussianSampler(Sampler):
    name: str


class DDPM(GaussianSampler):
    name = "ddpm"

    def __init__(self, mean_type: str = "epsilon", var_type: str = "fixed_small") -> None:
        super().__init__()
        if mean_type not in _MEAN:
            raise ValueError(f"mean_type must be one of {list(_MEAN)}")
        if var_type not in _VAR:
            raise ValueError(f"variance_type must be one of {list(_VAR)}")
        self.mean_type, self.var_type = mean_type, var_type
        self._dev_tables: dict[tuple, Tensor] = {}

    def set_steps(self, betas: Tensor) -> None:
        one = torch.ones_like(betas)
        self.betas = betas
        self.alphas = one - betas
        self.alphas_bar = self.alphas.cumprod(dim=0)
        self.alphas_bar_prev = torch.cat([torch.tensor([1.0], dtype=torch.float64), self.alphas_bar[:-1]])
        self.alphas_bar_next = torch.cat([self.alphas_bar[1:], torch.tensor([0.0], dtype=torch.float64)])
        self.sqrt_alphas_bar = self.alphas_bar.sqrt()
        self.posterior_variance = betas * (one - self.alphas_bar_prev) / (one - self.alphas_bar)
        self.posterior_log_variance_clipped = torch.log(torch.cat([self.posterior_variance[1:2], self.posterior_variance[1:]]))
        self.posterior_mean_coef1 = betas * self.alphas_bar_prev.sqrt() / (one - self.alphas_bar)
        self.posterior_mean_coef2 = (one - self.alphas_bar_prev) * self.alphas.sqrt() / (one - self.alphas_bar)
        self._dev_tables.clear()

    def _variance_tables(self) -> tuple[Tensor, Tensor]:
        if self.var_type == "fixed_small":
            return self.posterior_variance, self.posterior_log_variance_clipped
        if self.var_type == "fixed_large":
            v = torch.cat([self.posterior_variance[1:2], self.betas[1:]])
            return v, torch.log(v)
        # learned / learned_range (ddpm.py:212-222): the variance comes from the prediction's second half; the kernel needs the two
        # ends of the range, rows 4 and 5 of the learned table
        return self.posterior_log_variance_clipped, self.betas

    @property
    def learned_variance(self) -> bool:
        return self.var_type in ops.VAR_MODES

    def _check_halves(self, model_prediction: Tensor, xt: Tensor) -> None:
        assert model_prediction.shape[1] % 2 == 0, "a learned-variance prediction has an even channel count (ddpm.py:271)"
        assert model_prediction.shape[1] == 2 * xt.shape[1] and model_prediction.shape[2:] == xt.shape[2:], (
            f"var_type={self.var_type!r} takes a [B, 2C, ...] prediction for xt {tuple(xt.shape)}, got {tuple(model_prediction.shape)}")

    def _tables(self, device: torch.device) -> Tensor:
        key = ("ddpm", device, self.var_type)
        if key not in self._dev_tables:
            var, lv = self._variance_tables()
            t = torch.stack([self.sqrt_alphas_bar, self.alphas_bar, self.posterior_mean_coef1, self.posterior_mean_coef2, var, lv])
            self._dev_tables[key] = f32_table(t, device)
        return self._dev_tables[key]

    def _guided(self, model_prediction: Tensor, prediction_uncond: Tensor | None, guidance_scale: float, xt: Tensor,
                timesteps: Tensor, tab: Tensor, coefs: Tensor, guidance_rescale: float, dynamic_threshold: float | None,
                threshold_max: float | None):
        """the arguments of a step in the form the kernels read, and the per-sample device scalars of a guided one (None at the
        defaults, which launch nothing), two launches that materialise nothing the size of the image:
        cfg_mul, the CFG-rescale factor (Lin et al. 2023) of the combined prediction's mean half -- only where the step is guided;
        x0_thr, the dynamic threshold (Saharia et al. 2022) of the x0 the step kernel will form from the same arguments.
        -> (pred, pred_uncond, xt, t) in the form the kernels read, cfg_mul or None, x0_thr or None"""
        pred = model_prediction.float().contiguous()
        pu = None if prediction_uncond is None else prediction_uncond.float().contiguous()
        x, t = xt.float().contiguous(), timesteps.to(torch.int32).contiguous()
        halves = self.learned_variance
        mul = ops.cfg_rescale_coef(pred, pu, guidance_scale, guidance_rescale, halves) if guidance_rescale > 0 and pu is not None else None
        thr = None
        if dynamic_threshold is not None:
            k, f = quantile_position(dynamic_threshold, x.numel() // x.shape[0])
            thr = ops.x0_threshold(pred, pu, guidance_scale, mul, x, t, tab, coefs, _MEAN.index(self.mean_type), k, f, threshold_max,
                                   halves)
        return pred, pu, x, t, mul, thr

    def step(self, model_prediction: Tensor, timesteps: Tensor, xt: Tensor, clamp_x: bool = False,
             prediction_uncond: Tensor | None = None, guidance_scale: float = 0.0, guidance_rescale: float = 0.0,
             dynamic_threshold: float | None = None, threshold_max: float | None = None) -> StepResult:
        """guidance_rescale / dynamic_threshold / threshold_max (this project's): see `_guided`.  At their defaults the call below is
        what it was."""
        noise = torch.randn_like(xt)  # ddpm.py:302 (drawn for every t, masked at t == 0)
        if self.learned_variance:  # `_tables` rows 4, 5 are then (posterior_log_variance_clipped, betas)
            self._check_halves(model_prediction, xt)
        tab = self._tables(xt.device)
        pred, pu, x, t, mul, thr = self._guided(model_prediction, prediction_uncond, guidance_scale, xt, timesteps, tab, tab[2:4],
                                                guidance_rescale, dynamic_threshold, threshold_max)
        mean_type, var_mode = _MEAN.index(self.mean_type), ops.VAR_MODES.get(self.var_type, ops.VAR_FIXED)
        if guidance_rescale > 0 or dynamic_threshold is not None:
            out = ops.ddpm_step_g(pred, pu, guidance_scale, mul, thr, x, noise, t, tab, mean_type, var_mode, clamp_x)
        elif self.mean_type == "v":  # one entry point for [B, C] and [B, 2C] predictions; `_tables` follows var_type
            out = ops.ddpm_step_v(pred, pu, guidance_scale, x, noise, t, tab, var_mode, clamp_x)
        elif self.learned_variance:
            out = ops.ddpm_step_lv(pred, pu, guidance_scale, x, noise, t, tab, mean_type, var_mode, clamp_x)
        else:
            out = ops.ddpm_step(pred, pu, guidance_scale, x, noise, t, tab, mean_type, clamp_x)
        xp, x0, mean, std, lp = out
        return StepResult(x_prev=xp, estimated_x0=x0, x_prev_mean=mean, x_prev_std=std, logprob=lp)
