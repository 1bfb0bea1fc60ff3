"""`Diffuser` facade (reference diffuse/diffuser.py:14-239): picks the modelization from `model_registry` and
forwards draw_timesteps / compute_loss / set_steps / generate to it, same signatures."""

from __future__ import annotations

from typing import Any

from torch import Tensor

from .modelizations.diffusion import Diffusion
from .modelizations.flow import Flow
from .modelizations.gaussian_diffusion import GaussianDiffusion
from .utils import SamplingOutput, guidance_kwargs


class Diffuser:
    model_registry: dict[str, type[Diffusion]] = {"rectified_flow": Flow, "gaussian_diffusion": GaussianDiffusion}

    def __init__(self, denoiser, sampling_method: str, model_type: str = "rectified_flow", n_steps: int = 1000,
                 vision_tower=None, extra_args: dict[str, Any] = {}, extra_losses: list = []) -> None:
        self.model_type = model_type
        self.denoiser = denoiser
        self.n_steps = n_steps
        self.vision_tower = vision_tower
        self.extra_losses = extra_losses
        if self.vision_tower:
            self.latent_scale = self.vision_tower.latent_scale
            self.latent_bias = self.vision_tower.latent_bias
        if self.model_type not in self.model_registry:
            raise NotImplementedError(f"Model type {self.model_type} is not implemented")
        self.diffusion = self.model_registry[self.model_type](
            n_steps=n_steps, sampling_method=sampling_method, latent_diffusion=self.vision_tower is not None, **extra_args)

    def eval(self) -> None:
        self.denoiser.eval()

    def train(self) -> None:
        self.denoiser.train()

    def draw_timesteps(self, batch_size: int) -> Tensor:
        if getattr(self.diffusion, "timestep_sampler_state", None) is not None:  # a loss-aware sampler draws on the denoiser's device
            return self.diffusion.draw_timesteps(batch_size=batch_size, device=next(self.denoiser.parameters()).device)
        return self.diffusion.draw_timesteps(batch_size=batch_size)

    def compute_loss(self, model_inputs, timesteps: Tensor | None = None, noise: Tensor | None = None,
                     extra_args: dict[str, Any] = {}, grpo: bool = False, grpo_args: dict[str, Any] = {}) -> dict[str, Tensor]:
        if grpo:
            assert isinstance(self.diffusion, Flow), "GRPO loss computation is only available for Flow-based models"
            return self.diffusion.compute_loss_grpo(self.denoiser, model_inputs, **grpo_args)
        assert timesteps is not None, "timesteps must be provided for loss computation"
        return self.diffusion.compute_loss(self.denoiser, model_inputs, timesteps, noise, self.extra_losses, extra_args)

    def evaluate_bpd(self, model_inputs, **kwargs: Any) -> dict[str, Tensor]:
        """the variational bound on the negative log-likelihood of the clean data model_inputs["x"] in bits per dimension (this
        project's; the reference has no likelihood evaluation): `GaussianDiffusion.calc_bpd_loop` on this denoiser, same keywords
        (clip_denoised, t_chunk, noise, timesteps, use_tqdm) and same result dict.  Refused for rectified flow (no variational
        bound) and for latent diffusion (the t = 0 term's 8-bit bins are pixel bins)."""
        return self.diffusion.calc_bpd_loop(self.denoiser, model_inputs, **kwargs)

    def evaluate_nll(self, model_inputs, **kwargs: Any) -> dict[str, Tensor]:
        """the negative log-likelihood of the clean data model_inputs["x"] under a rectified-flow model's probability-flow ODE, in nats
        per dimension (and, in pixel space, bits per dimension of the 8-bit data), with Hutchinson's divergence estimate (this
        project's; the reference has no likelihood evaluation): `Flow.calc_nll_loop` on this denoiser, same keywords (method,
        n_probes, probe, probes, dequantize, dequant_noise, use_tqdm) and same result dict.  Refused for Gaussian diffusion, whose
        likelihood measure is the variational bound (`evaluate_bpd`)."""
        return self.diffusion.calc_nll_loop(self.denoiser, model_inputs, **kwargs)

    def set_steps(self, n_steps: int, schedule: str = "linear", *args: Any, **kwargs: Any) -> None:
        self.diffusion.set_steps(n_steps, schedule=schedule, *args, **kwargs)

    def generate(self, model_inputs, data_shape: tuple[int, ...] | None = None, use_tqdm: bool = True,
                 clamp_x: bool = False, guidance_scale: float = 0, sampler_args: dict[str, Any] = {},
                 guidance_rescale: float = 0.0, guidance_interval: tuple[float, float] | None = None,
                 dynamic_threshold: float | None = None, threshold_max: float | None = None,
                 return_intermediates: bool = False, return_latents: bool = False, init_image: Tensor | None = None,
                 strength: float = 1.0, mask: Tensor | None = None, resample: int = 1) -> SamplingOutput:
        """init_image, strength, mask, resample (this project's; the reference starts from pure noise only): image-to-image (SDEdit)
        and inpainting (RePaint) with every sampler.  init_image [B, C, *spatial] lives in the space the denoiser works in (with a
        vision tower: scaled latents, no encoder is run); strength in (0, 1] is the fraction of the sampler's steps that is run, from
        init_image noised to the level where they start; mask [B, 1, *spatial] or [B, C, *spatial], bool or float in [0, 1], is 1
        where the image is generated and 0 where init_image is kept; resample >= 1 repeats every step but the last that many times
        (RePaint's U).  model_inputs["x"] stays the initial noise.  A bad argument raises a ValueError that names it before any device
        work; with all four at their defaults the call is what it was.  Details: `Flow._denoise_from_image`,
        `GaussianDiffusion._denoise_from_image`.

        guidance_rescale, guidance_interval, dynamic_threshold, threshold_max (this project's): guided sampling at a high
        guidance_scale.  guidance_rescale = phi in [0, 1] scales the guided prediction back to the conditional prediction's per-sample
        standard deviation, mixed by phi (CFG rescale, Lin et al. 2023); guidance_interval = (lo, hi), 0 <= lo <= hi <= 1, guides only
        the steps whose noise level lies inside it (flow: t; Gaussian diffusion: (training index + 1) / training steps) and runs one
        forward elsewhere (Kynkaanniemi et al. 2024); dynamic_threshold = p in (0, 1] clamps every step's x0 to its own p-quantile
        of |x0| (at least 1, at most threshold_max) and divides by it (Saharia et al. 2022; Gaussian diffusion only).  Same rule: a
        ValueError before any device work, and the call is what it was with all four at their defaults."""
        extra = guidance_kwargs(guidance_rescale, guidance_interval, dynamic_threshold, threshold_max)
        if init_image is not None or strength != 1.0 or mask is not None or resample != 1:
            extra.update(init_image=init_image, strength=strength, mask=mask, resample=resample)
        out = self.diffusion.denoise(self.denoiser, model_inputs=model_inputs, data_shape=data_shape, use_tqdm=use_tqdm,
                                     clamp_x=clamp_x, guidance_scale=guidance_scale, sampler_args=sampler_args,
                                     return_intermediates=return_intermediates, **extra)
        if self.vision_tower and not return_latents:  # decode latents with the (external) VAE, diffuser.py:220-227
            scale, bias = self.latent_scale, self.latent_bias
            if isinstance(scale, Tensor):
                scale = scale.to(out["x"].device)
            if isinstance(bias, Tensor):
                bias = bias.to(out["x"].device)
            out["x"] = self.vision_tower.decode(out["x"] / scale + bias)
        return out
