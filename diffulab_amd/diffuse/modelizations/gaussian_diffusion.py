"""DDPM / IDDPM modelization (reference diffuse/modelizations/gaussian_diffusion.py:18-447) over the HIP kernels.

Schedules are built on the host in fp64 with the same torch ops as the reference (bit-identical tables and
`timestep_map`); the device kernels read their fp32 casts.  Timesteps are int32 indices drawn on the CPU global
generator and are fed to the denoiser unscaled (after the `timestep_map` remap when the chain is respaced).
"""

from __future__ import annotations

import math
from typing import Any, Callable

import torch
from torch import Tensor

from ... import ops
from ..samplers.common import StepResult
from ..samplers.gaussian_diffusion import DDIM, DDPM, DPMSolverPP2M
from ..utils import (SamplingOutput, check_guidance, f32_table, guidance_kwargs, in_guidance_interval, strength_to_steps,
                     to_device)
from .diffusion import Diffusion, gd_head, gd_rows_head, hybrid_head, mse_head
from .timestep_sampler import TIMESTEP_SAMPLERS, LossSecondMomentState
from .utils import space_timesteps

try:
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    def tqdm(it, **kw):
        return it


LOSS_TARGETS = ("epsilon", "mean_type")
LOSS_WEIGHTINGS = (None, "min_snr")
LOSS_TYPES = ("mse", "vlb")


def min_snr_weights(alphas_bar: Tensor, target: str, gamma: float = 5.0) -> Tensor:
    """Min-SNR-gamma loss weights (Hang et al., "Efficient Diffusion Training via Min-SNR Weighting Strategy", 2023) of one chain,
    fp64 [T]: with snr_t = ab_t / (1 - ab_t), the weight min(snr, gamma) of the x0 loss expressed for the target that is regressed."""
    ab = alphas_bar.double()
    snr = ab / (1.0 - ab)
    clipped = snr.clamp(max=gamma)
    if target == "epsilon":
        return clipped / snr
    if target == "xstart":
        return clipped
    if target == "v":
        return clipped / (snr + 1.0)
    raise ValueError(f"loss_weighting='min_snr' is defined for the targets epsilon, xstart and v, not for {target!r}")


BPD_ROWS = 256  # rows (sample, timestep pairs) of one pass of calc_bpd_loop when t_chunk is left to it


def plan_bpd_chunks(n_steps: int, batch: int, t_chunk: int | None = None, timesteps=None) -> list[list[int]]:
    """the passes of `calc_bpd_loop` as lists of chain indices: the indices (all n_steps of the chain, or the subset `timesteps`)
    from high to low, t_chunk per pass; t_chunk None takes the largest K with K * batch <= BPD_ROWS rows, at least 1.  Host
    arithmetic only; a bad argument raises a ValueError that names it."""
    if t_chunk is not None and (isinstance(t_chunk, bool) or int(t_chunk) != t_chunk or t_chunk < 1):
        raise ValueError(f"t_chunk must be an integer >= 1 or None, got {t_chunk!r}")
    if timesteps is None:
        idx = list(range(n_steps))
    else:
        idx = [int(v) for v in (timesteps.tolist() if isinstance(timesteps, Tensor) else timesteps)]
        if not idx:
            raise ValueError("timesteps must name at least one index of the chain")
        if min(idx) < 0 or max(idx) >= n_steps:
            raise ValueError(f"timesteps must lie in [0, {n_steps}) on this chain, got {min(idx)} .. {max(idx)}")
        if len(set(idx)) != len(idx):
            raise ValueError("timesteps must not repeat an index")
    idx = sorted(idx, reverse=True)
    k = max(1, BPD_ROWS // max(1, int(batch))) if t_chunk is None else int(t_chunk)
    return [idx[i:i + k] for i in range(0, len(idx), k)]


NO_ODE_LIKELIHOOD = ("the ODE likelihood (calc_nll_loop, evaluate_nll, val_nll_batches) is evaluated for model_type='rectified_flow' "
                     "only; the likelihood measure of Gaussian diffusion is the variational bound: evaluate_bpd / calc_bpd_loop "
                     "(train(val_bpd_batches=...))")


class GaussianDiffusion(Diffusion):
    sampler_registry = {"ddpm": DDPM, "ddim": DDIM, "dpmpp_2m": DPMSolverPP2M}  # "dpmpp_2m" (second order, multistep) is this project's

    def __init__(self, n_steps: int = 1000, sampling_method: str = "ddpm", schedule: str = "linear",
                 latent_diffusion: bool = False, sampler_parameters: dict[str, Any] = {}, vlb_weight: float | None = None,
                 loss_target: str = "epsilon", loss_weighting: str | None = None, min_snr_gamma: float = 5.0,
                 loss_type: str = "mse", timestep_sampler: str = "uniform", sampler_history: int = 10,
                 sampler_uniform_prob: float = 0.001) -> None:
        if sampling_method not in self.sampler_registry:
            raise ValueError(f"sampling method must be one of {list(self.sampler_registry)}")
        if loss_target not in LOSS_TARGETS:
            raise ValueError(f"loss_target must be one of {list(LOSS_TARGETS)}")
        if loss_weighting not in LOSS_WEIGHTINGS:
            raise ValueError(f"loss_weighting must be one of {list(LOSS_WEIGHTINGS)}")
        # what compute_loss regresses the mean output on: the noise (the reference's loss, whatever the sampler's mean_type), or the
        # parameterisation the sampler reads the output as
        mean_type = sampler_parameters.get("mean_type", "epsilon")
        if loss_target == "epsilon" and mean_type == "v":
            raise ValueError('a sampler with mean_type="v" takes loss_target="mean_type": loss_target="epsilon" would train a noise '
                             "predictor and sample it as a v predictor")
        self.loss_target, self.loss_weighting, self.min_snr_gamma = loss_target, loss_weighting, float(min_snr_gamma)
        self._target = mean_type if loss_target == "mean_type" else "epsilon"
        if (loss_weighting is not None and loss_target == "epsilon" and mean_type != "epsilon"
                and sampler_parameters.get("var_type", "fixed_small") in ops.VAR_MODES):
            # the weighted head derives the bound's frozen mean from the regression target; the unweighted default derives it from
            # mean_type.  A weight documented to touch "loss" alone must not move "vb", so the mixed form is not offered.
            raise ValueError(f'loss_weighting with learned variances and mean_type={mean_type!r} takes loss_target="mean_type": with '
                             'loss_target="epsilon" the variational bound would read the output as epsilon')
        if loss_weighting == "min_snr" and self._target == "xprev":
            raise ValueError('loss_weighting="min_snr" is defined for the targets epsilon, xstart and v, not for xprev')
        self._check_loss_type(loss_type, timestep_sampler, sampler_history, sampler_uniform_prob, loss_target, loss_weighting, mean_type,
                              sampler_parameters.get("var_type", "fixed_small"), latent_diffusion)
        self.loss_type, self.timestep_sampler = loss_type, timestep_sampler
        # compute_loss goes through the row head (per-sample losses) instead of the batch-scalar heads
        self._rows_head = loss_type == "vlb" or timestep_sampler != "uniform"
        self.timestep_sampler_state: LossSecondMomentState | None = None  # built below, once the chain is
        self.last_terms: dict[str, Tensor] = {}
        self.loss_weight: Tensor | None = None  # fp64 [T], rebuilt with the chain
        self._dev_weight: dict[torch.device, Tensor] = {}
        self.training_steps = n_steps
        # weight of the variational-bound term of a learned-variance model's loss: Improved DDPM rescales it by T / 1000
        self.vlb_weight = n_steps / 1000 if vlb_weight is None else float(vlb_weight)
        self._dev: dict[torch.device, tuple[Tensor, Tensor]] = {}
        super().__init__(n_steps=self.training_steps, sampling_method=sampling_method, schedule=schedule,
                         latent_diffusion=latent_diffusion, sampler_parameters=sampler_parameters)
        if timestep_sampler == "loss_second_moment":
            self.timestep_sampler_state = LossSecondMomentState(self.steps, sampler_history, sampler_uniform_prob)

    @staticmethod
    def _check_loss_type(loss_type, timestep_sampler, sampler_history, sampler_uniform_prob, loss_target, loss_weighting, mean_type,
                         var_type, latent_diffusion) -> None:
        """the host checks of loss_type / timestep_sampler and their two parameters: a ValueError that names the argument"""
        if loss_type not in LOSS_TYPES:
            raise ValueError(f"loss_type must be one of {list(LOSS_TYPES)}, got {loss_type!r}")
        if timestep_sampler not in TIMESTEP_SAMPLERS:
            raise ValueError(f"timestep_sampler must be one of {list(TIMESTEP_SAMPLERS)}, got {timestep_sampler!r}")
        if isinstance(sampler_history, bool) or not isinstance(sampler_history, int) or sampler_history < 1:
            raise ValueError(f"sampler_history must be an integer >= 1, got {sampler_history!r}")
        if isinstance(sampler_uniform_prob, bool) or not isinstance(sampler_uniform_prob, (int, float)) or not 0.0 <= sampler_uniform_prob <= 1.0:
            raise ValueError(f"sampler_uniform_prob must lie in [0, 1], got {sampler_uniform_prob!r}")
        learned = var_type in ops.VAR_MODES
        if loss_type == "vlb":
            if not learned:
                raise ValueError(f'loss_type="vlb" needs learned variances (var_type "learned" or "learned_range"), got var_type={var_type!r}: '
                                 "with a fixed variance the variance is not trained and L_vlb is a reweighted MSE")
            if loss_weighting is not None:
                raise ValueError(f'loss_weighting={loss_weighting!r} weights the MSE, which loss_type="vlb" does not form')
            if latent_diffusion:
                raise ValueError('latent_diffusion=True: the t = 0 term of loss_type="vlb" is the likelihood of 8-bit pixel bins on [-1, 1], '
                                 "which means nothing for latents")
        if (loss_type == "vlb" or timestep_sampler != "uniform") and learned and loss_target == "epsilon" and mean_type != "epsilon":
            # one parameterisation per call of the row head: the regression target is also what the bound reads the mean output as
            raise ValueError(f'loss_type="vlb" / a loss-aware timestep_sampler with learned variances and mean_type={mean_type!r} take '
                             'loss_target="mean_type": with loss_target="epsilon" the bound would read the output as epsilon')

    def set_diffusion_parameters(self, betas: Tensor) -> None:
        self.betas = betas
        self.alphas = torch.ones_like(betas) - betas
        self.alphas_bar = self.alphas.cumprod(dim=0)
        self.sqrt_alphas_bar = self.alphas_bar.sqrt()
        self._dev.clear()
        self._dev_weight.clear()
        if self.loss_weighting == "min_snr":  # a respaced chain has its own alphas_bar
            self.loss_weight = min_snr_weights(self.alphas_bar, self._target, self.min_snr_gamma)
        self.sampler.set_steps(betas)

    def set_steps(self, n_steps: int, schedule: str = "linear", section_counts: int | str | None = None) -> None:
        """n_steps below the training chain respaces it.  Only "ddim" asks `space_timesteps` for the reference's ddim=True spacing,
        which only ever accepts stride 1; "dpmpp_2m" (like "ddpm") gets ddim=False, so `set_steps(20)` on a 1000-step chain yields
        the IDDPM-respaced 20-step chain, and the sampler's lambda table is that chain's."""
        if n_steps != self.training_steps:
            section_counts = section_counts or n_steps
        self.steps = n_steps
        self.set_diffusion_parameters(self._get_variance_schedule(self.training_steps, schedule))
        self.timestep_map: list[int] = []
        if section_counts:
            keep = space_timesteps(num_timesteps=self.training_steps, section_counts=section_counts,
                                   ddim=self.sampling_method == "ddim")
            prev_bar = torch.tensor(1.0)
            respaced: list[Tensor] = []
            for i, bar in enumerate(self.alphas_bar):
                if i in keep:
                    respaced.append(torch.ones_like(bar) - bar / prev_bar)
                    prev_bar = bar
                    self.timestep_map.append(i)
            self.set_diffusion_parameters(torch.tensor(respaced))
        state = getattr(self, "timestep_sampler_state", None)
        if state is not None and state.n_steps != self.steps:  # the history is per index of the chain being trained
            state.reset(self.steps)

    def _get_variance_schedule(self, n_steps: int, variance_schedule: str = "linear") -> Tensor:
        if variance_schedule == "linear":  # Ho et al., rescaled to any chain length
            k = 1000 / n_steps
            return torch.linspace(k * 0.0001, k * 0.02, n_steps, dtype=torch.float64, requires_grad=False)
        if variance_schedule == "cosine":
            return self._betas_for_alpha_bar(n_steps, lambda u: math.cos((u + 0.008) / 1.008 * math.pi / 2) ** 2)
        raise NotImplementedError(f"unknown beta schedule: {variance_schedule}")

    def _betas_for_alpha_bar(self, n_steps: int, alpha_bar: Callable[[float], float], max_beta: float = 0.999) -> Tensor:
        vals = [min(1 - alpha_bar((i + 1) / n_steps) / alpha_bar(i / n_steps), max_beta) for i in range(n_steps)]
        return torch.tensor(vals, dtype=torch.float64, requires_grad=False)

    def draw_timesteps(self, batch_size: int, device: torch.device | str | None = None) -> Tensor:
        """timestep_sampler "uniform": the reference's CPU draw (`device` is ignored).  "loss_second_moment": a device int32 tensor
        drawn from the state's distribution -- one uniform per sample from the CPU global generator (the reference's site for
        timestep randomness), searched in the device's cumulative table by `dl_draw_timesteps`; nothing is read back."""
        if self.timestep_sampler_state is None:
            return torch.randint(0, self.steps, (batch_size,), dtype=torch.int32)
        if device is None:
            raise ValueError('device: timestep_sampler="loss_second_moment" draws on the device that holds its state; pass the '
                             "denoiser's (Diffuser.draw_timesteps does)")
        u = torch.rand(batch_size)
        return self.timestep_sampler_state.draw(to_device(u, device, torch.float32))

    def _remap(self, timesteps: Tensor) -> Tensor:
        if self.timestep_map:
            table = torch.tensor(self.timestep_map, device=timesteps.device, dtype=timesteps.dtype)
            return table[timesteps]
        return timesteps

    def guidance_level(self, t: int) -> float:
        """the noise level of the step at index t, as `guidance_interval` reads it: (tau + 1) / training_steps, tau the index the
        denoiser is given (timestep_map[t] on a respaced chain, else t)"""
        tau = self.timestep_map[t] if self.timestep_map else t
        return (tau + 1) / self.training_steps

    def one_step_denoise(self, model, model_inputs, t: int, clamp_x: bool = False, guidance_scale: float = 0.0,
                         sampler_args: dict[str, Any] = {}, guidance_rescale: float = 0.0,
                         guidance_interval: tuple[float, float] | None = None, dynamic_threshold: float | None = None,
                         threshold_max: float | None = None) -> StepResult:
        """guidance_rescale / guidance_interval / dynamic_threshold / threshold_max (this project's): CFG rescale and the dynamic
        threshold reach the sampler as keywords; a step whose `guidance_level` lies outside the interval makes the one conditional
        forward (no combine, no rescale; the threshold still applies)."""
        if guidance_rescale or guidance_interval is not None or dynamic_threshold is not None or threshold_max is not None:
            check_guidance(guidance_scale, guidance_rescale, guidance_interval, dynamic_threshold, threshold_max)
            extra_args = {"guidance_rescale": guidance_rescale} if guidance_rescale else {}
            if dynamic_threshold is not None:
                extra_args.update(dynamic_threshold=dynamic_threshold, threshold_max=threshold_max)
            sampler_args = {**sampler_args, **extra_args}
            if not in_guidance_interval(guidance_interval, self.guidance_level(t)):
                guidance_scale = 0.0
        device = next(model.parameters()).device
        timesteps = torch.full((model_inputs["x"].shape[0],), t, device=device, dtype=torch.int32)
        t_model = self._remap(timesteps)
        extra = {}
        pair = None
        if guidance_scale > 0:  # CFG combine fused into the step kernel; the two forwards as one where the denoiser can (see Flow)
            fn = getattr(model, "forward_cfg_pair", None)
            pair = fn(t_model, **model_inputs) if fn is not None else None
        if pair is not None:
            prediction, extra = pair[0], {"prediction_uncond": pair[1], "guidance_scale": guidance_scale}
        else:
            prediction = model(**{**model_inputs, "p": 0}, timesteps=t_model)["x"]
            if guidance_scale > 0:
                extra = {"prediction_uncond": model(**{**model_inputs, "p": 1}, timesteps=t_model)["x"],
                         "guidance_scale": guidance_scale}
        if self.sampler.multistep:  # its coefficients and its history rule are host arithmetic on the index: no device value is read
            extra = {**extra, "step_index": t}
        return self.sampler.step(model_prediction=prediction, timesteps=timesteps, xt=model_inputs["x"], clamp_x=clamp_x,
                                 **extra, **sampler_args)

    def _weight(self, device: torch.device) -> Tensor | None:
        if self.loss_weight is None:
            return None
        if device not in self._dev_weight:
            self._dev_weight[device] = f32_table(self.loss_weight, device)
        return self._dev_weight[device]

    def compute_loss(self, model, model_inputs, timesteps: Tensor, noise: Tensor | None = None, extra_losses=[],
                     extra_args: dict[str, Any] = {}) -> dict[str, Tensor]:
        """One of four heads, with the same keys from each: "loss", and "vb" for a learned-variance model.
        - the row head (`_rows_losses`): loss_type="vlb" and / or a loss-aware timestep sampler;
        - `gd_head`: the loss of the parameterisation the sampler reads (loss_target="mean_type": x0, the posterior mean or v as the
          regression target, formed inside the kernel) and / or a per-timestep weight on it.  The bound of a learned-variance model
          derives its frozen mean from the same parameterisation and carries no weight.  (The constructor refuses the one form in
          which that parameterisation would differ from the sampler's mean_type.)
        - `hybrid_head`: L_hybrid of Nichol & Dhariwal (2021), eq. 16, for a [B, 2C, ...] denoiser (the reference leaves it as a TODO,
          gaussian_diffusion.py:267): "loss" = the usual MSE on the mean half, "vb" = vlb_weight * the variational bound in bits per
          dimension, which trains the variance half only.  The trainer sums the dict and logs each entry.
        - `mse_head`: the reference's loss, which reads neither x0 nor xt, so no copy of x0 is kept."""
        learned = self.sampler.learned_variance
        gd = self._target != "epsilon" or self.loss_weight is not None
        plain = not (self._rows_head or gd or learned)
        x0 = model_inputs["x"]
        if not plain:
            x0 = x0.float().contiguous()  # kept: add_noise's result replaces model_inputs["x"]
        model_inputs["x"], noise = self.add_noise(x0, timesteps, noise)
        xt = model_inputs["x"]
        prediction = model(**model_inputs, timesteps=self._remap(timesteps))["x"]
        if not plain:
            t = to_device(timesteps, xt.device, torch.int32)
        if learned:
            self.sampler._check_halves(prediction, xt)
        if self._rows_head:
            loss_dict = self._rows_losses(prediction, noise, x0, xt, t)
        elif gd:
            out = gd_head(prediction, noise, x0, xt, t, self.sampler._tables(xt.device), ops.MEAN_TYPES[self._target],
                          self._weight(xt.device), ops.VAR_MODES[self.sampler.var_type] if learned else ops.VAR_FIXED)
            loss_dict = {"loss": out[0], "vb": self.vlb_weight * out[1]} if learned else {"loss": out}
        elif learned:
            mse, vb = hybrid_head(prediction, noise, x0, xt, t, self.sampler._tables(xt.device), ops.MEAN_TYPES[self.sampler.mean_type],
                                  ops.VAR_MODES[self.sampler.var_type])
            loss_dict = {"loss": mse, "vb": self.vlb_weight * vb}
        else:
            loss_dict = {"loss": mse_head(prediction, noise, None, ops.LOSS_EPS)}
        for extra_loss in extra_losses:
            loss_dict[extra_loss.name] = extra_loss(**extra_args)
        return loss_dict

    def _rows_losses(self, prediction: Tensor, noise: Tensor, x0: Tensor, xt: Tensor, t: Tensor) -> dict[str, Tensor]:
        """the losses of `gd_head` through the row head (loss_type="vlb" and / or a loss-aware timestep sampler; Nichol &
        Dhariwal 2021, sec. 3.3): every sample's loss is multiplied by imp[t_b] = 1 / (T p[t_b]) -- "loss" and "vb" alike, as IDDPM
        weights the whole per-sample loss -- and, when the prediction requires grad, the step's (t_b, total_b) pairs enter the
        sampler's history with one launch (all ranks' pairs under data parallel).  total_b is the sample's loss before that weight:
        w[t_b] mse_b + vlb_weight vb_b, or vb_b alone for loss_type="vlb", which returns {"loss": the bound} with its gradient
        flowing into the mean output too.  Under no_grad the history is not touched: a validation batch drawn from the current
        distribution with the same weights is an unbiased estimate of the uniform loss.  The step's detached per-sample tensors stay
        on the device as `last_terms`; no device value is read back."""
        learned = self.sampler.learned_variance
        state = self.timestep_sampler_state
        imp = None
        if state is not None:
            imp = state.on(xt.device)["imp"]
            if prediction.requires_grad:  # the backward reads the weights of this step, the update below rewrites the table
                imp = imp.clone()
        out = gd_rows_head(prediction, noise, x0, xt, t, self.sampler._tables(xt.device), ops.MEAN_TYPES[self._target],
                           self._weight(xt.device), imp, ops.VAR_MODES[self.sampler.var_type] if learned else ops.VAR_FIXED,
                           ops.LOSS_TYPES[self.loss_type], self.vlb_weight)
        if self.loss_type == "vlb":
            loss_dict = {"loss": out["loss_vb"]}
        elif learned:
            loss_dict = {"loss": out["loss_mse"], "vb": self.vlb_weight * out["loss_vb"]}
        else:
            loss_dict = {"loss": out["loss_mse"]}
        self.last_terms = {"t": t, **{k: out[k].detach() for k in ("mse", "vb", "total") if k in out}}
        if state is not None and prediction.requires_grad:
            state.update(t, self.last_terms["total"])
        return loss_dict

    def add_noise(self, x: Tensor, timesteps: Tensor, noise: Tensor | None = None) -> tuple[Tensor, Tensor]:
        x = x.float().contiguous()
        if noise is None:
            noise = torch.randn_like(x)
        noise = noise.to(device=x.device, dtype=torch.float32).contiguous()
        assert noise.shape == x.shape
        assert timesteps.shape[0] == x.shape[0]
        if x.device not in self._dev:
            self._dev[x.device] = (f32_table(self.sqrt_alphas_bar, x.device), f32_table(self.alphas_bar, x.device))
        sab, ab = self._dev[x.device]
        return ops.ddpm_add_noise(x, noise, to_device(timesteps, x.device, torch.int32), sab, ab), noise

    # ---- likelihood evaluation (this project's; the reference has none): the variational bound in bits per dimension, the headline
    # number of Nichol & Dhariwal, "Improved Denoising Diffusion Probabilistic Models" (2021), `calc_bpd_loop` of their code base
    def _bpd_check_halves(self, pred_shape: tuple[int, ...], x: Tensor) -> None:
        try:  # (shapes only: a meta tensor stands in for a prediction that does not exist yet)
            self.sampler._check_halves(torch.empty(pred_shape, device="meta"), x)
        except AssertionError as e:
            raise ValueError(f"model: {e}") from None

    def _bpd_plan(self, model, model_inputs, t_chunk, noise, timesteps) -> list[list[int]]:
        """every host check of `calc_bpd_loop`, before any device work; -> the passes as lists of chain indices"""
        if self.latent_diffusion:
            raise ValueError("latent_diffusion=True: the bound's t = 0 term is the likelihood of 8-bit bins on [-1, 1], which only mean "
                             "something for pixel data; bits per dimension of a latent chain are not offered")
        x = model_inputs["x"]
        if x.dim() < 2:
            raise ValueError(f"model_inputs['x'] must be [B, C, *spatial], got {tuple(x.shape)}")
        chunks = plan_bpd_chunks(self.steps, x.shape[0], t_chunk, timesteps)
        if noise is not None and tuple(noise.shape) != (x.shape[0], self.steps, *x.shape[1:]):
            raise ValueError(f"noise must be [B, T, C, *spatial] = {(x.shape[0], self.steps, *x.shape[1:])} (one draw per sample and "
                             f"chain index), got {tuple(noise.shape)}")
        out_ch = getattr(model, "out_channels", None) or getattr(model, "output_channels", None)
        if self.sampler.learned_variance and isinstance(out_ch, int):
            self._bpd_check_halves((x.shape[0], out_ch, *x.shape[2:]), x)
        return chunks

    def calc_nll_loop(self, *a: Any, **k: Any):
        raise NotImplementedError(NO_ODE_LIKELIHOOD)

    @torch.no_grad()
    def calc_bpd_loop(self, model, model_inputs, clip_denoised: bool = True, t_chunk: int | None = None, noise: Tensor | None = None,
                      timesteps=None, use_tqdm: bool = False) -> dict[str, Tensor]:
        """The variational bound on the negative log-likelihood of the clean data model_inputs["x"] [B, C, *spatial], in bits per
        dimension, term by term.  The chain's indices (all `self.steps` of them, or the subset `timesteps`) are walked from high to
        low, t_chunk of them per pass: a pass noises the data to its K indices (K * B rows, a fresh draw per row, or noise[:, j] of
        `noise` [B, T, C, *spatial] for index j), makes one conditional forward (p = 0, indices through the respacing map, every
        other entry of model_inputs repeated K times along the batch) and one `dl_vb_terms` launch.  t_chunk None: the largest K
        with K * B <= 256, at least 1.  Runs under no_grad (the denoiser takes its inference path); nothing is read back to the host
        inside the loop.  Unlike `compute_loss`, model_inputs is not mutated.
        -> "vb", "xstart_mse", "mse": f32 [B, n_t], columns in ascending index order (vb: KL(q(x_{t-1} | x_t, x_0) || p) for t > 0,
        the discretised-Gaussian NLL for t == 0; the squared errors of the predicted x0 and of the eps derived from it);
        "prior_bpd" f32 [B] = KL(q(x_T | x_0) || N(0, I)); "total_bpd" f32 [B] = vb.sum(1) + prior_bpd, only when every index was
        evaluated.  clip_denoised (IDDPM's default for this loop) clamps the predicted x0 to [-1, 1] before the model mean is formed.
        A bad argument raises a ValueError that names it before any device work."""
        chunks = self._bpd_plan(model, model_inputs, t_chunk, noise, timesteps)
        x0 = model_inputs["x"].float().contiguous()
        dev, B, tail = x0.device, x0.shape[0], tuple(x0.shape[1:])
        order = [j for c in chunks for j in c]
        n_t = len(order)
        t_rows = to_device(torch.tensor(order, dtype=torch.int32).repeat_interleave(B), dev, torch.int32)  # row k B + b: index k
        t_model = self._remap(t_rows)
        if noise is not None:
            noise = noise.to(device=dev, dtype=torch.float32)
            cols = torch.tensor(order, dtype=torch.int64).to(dev)
        tab = self.sampler._tables(dev)
        key = ("lv_q", dev)
        if key not in self.sampler._dev_tables:
            self.sampler._dev_tables[key] = f32_table(self.sampler.posterior_log_variance_clipped, dev)
        lv_q = self.sampler._dev_tables[key]
        mean_type = ops.MEAN_TYPES[self.sampler.mean_type]
        var_mode = ops.VAR_MODES.get(self.sampler.var_type, ops.VAR_FIXED)
        rest = {k: v for k, v in model_inputs.items() if k not in ("x", "p")}

        def repeated(v, K: int):
            if isinstance(v, Tensor) and v.dim() >= 1 and v.shape[0] == B:
                return v.repeat(K, *([1] * (v.dim() - 1)))
            if isinstance(v, dict):
                return {k: repeated(u, K) for k, u in v.items()}
            return v

        per_k: dict[int, tuple[Tensor, dict[str, Any]]] = {}  # x0 and the conditioning repeated K times (two values of K at most)
        flat = [torch.empty(n_t * B, device=dev, dtype=torch.float32) for _ in range(3)]
        off = 0
        for chunk in tqdm(chunks, desc="evaluating the bound", total=len(chunks), disable=not use_tqdm, leave=False):
            K = len(chunk)
            if K not in per_k:
                per_k[K] = (x0.repeat(K, *([1] * len(tail))), {k: repeated(v, K) for k, v in rest.items()})
            x0r, cond = per_k[K]
            rows = slice(off * B, (off + K) * B)
            eps = None if noise is None else noise.index_select(1, cols[off:off + K]).transpose(0, 1).reshape(K * B, *tail)
            xt, eps = self.add_noise(x0r, t_rows[rows], eps)
            prediction = model(**cond, x=xt, p=0, timesteps=t_model[rows])["x"]
            if self.sampler.learned_variance:
                self._bpd_check_halves(tuple(prediction.shape), xt)
            ops.vb_terms(prediction.float().contiguous(), eps, x0r, xt, t_rows[rows], tab, lv_q, mean_type, var_mode, clip_denoised,
                         out=tuple(a[rows] for a in flat))
            off += K
        out = {k: a.view(n_t, B).flip(0).t().contiguous() for k, a in zip(("vb", "xstart_mse", "mse"), flat)}
        ab = float(self.alphas_bar[-1])
        out["prior_bpd"] = ops.prior_bpd(x0, ab, math.log(1.0 - ab))
        if n_t == self.steps:
            out["total_bpd"] = out["vb"].sum(1) + out["prior_bpd"]
        return out

    # The reference leaves autograd on in this loop (gaussian_diffusion.py:344-447 carries no inference_mode / no_grad, unlike
    # Flow.denoise): outside the trainer's @no_grad image logging it would record a graph through all 1000 steps.  Here the
    # loop runs under no_grad: same values, and the denoiser takes its inference path (hipGraph replay, no activation keeping).
    @torch.no_grad()
    def denoise(self, model, model_inputs, data_shape: tuple[int, ...] | None = None, use_tqdm: bool = True,
                clamp_x: bool = False, guidance_scale: float = 0, sampler_args: dict[str, Any] = {},
                guidance_rescale: float = 0.0, guidance_interval: tuple[float, float] | None = None,
                dynamic_threshold: float | None = None, threshold_max: float | None = None,
                return_intermediates: bool = False, init_image: Tensor | None = None, strength: float = 1.0,
                mask: Tensor | None = None, resample: int = 1) -> SamplingOutput:
        """init_image / strength / mask / resample (this project's; the reference has neither): see `_denoise_from_image`.
        guidance_rescale / guidance_interval / dynamic_threshold / threshold_max (this project's): see `one_step_denoise`; validated
        here, before any device work.  At their defaults this is the reference's loop, call for call."""
        check_guidance(guidance_scale, guidance_rescale, guidance_interval, dynamic_threshold, threshold_max)
        guided = guidance_kwargs(guidance_rescale, guidance_interval, dynamic_threshold, threshold_max)
        cond = self._image_conditioning(model, model_inputs, data_shape, init_image, strength, mask, resample)
        if cond is not None:
            return self._denoise_from_image(model, model_inputs, cond, strength, resample, use_tqdm, clamp_x, guidance_scale,
                                            sampler_args, return_intermediates, guided)
        if "x" not in model_inputs:
            assert data_shape is not None, "'data_shape' must be provided if 'x' is not in model_inputs"
            p0 = next(model.parameters())
            model_inputs["x"] = torch.randn(data_shape, device=p0.device, dtype=p0.dtype)
        keep = return_intermediates
        xt = [model_inputs["x"]] if keep else None
        x0s: list[Tensor] = []
        means: list[Tensor] = []
        stds: list[Tensor] = []
        lps: list[Tensor] = []
        self.sampler.reset()
        for t in tqdm(list(range(self.steps))[::-1], desc="generating image", total=self.steps, disable=not use_tqdm,
                      leave=False):
            out = self.one_step_denoise(model=model, model_inputs=model_inputs, t=t, clamp_x=clamp_x,
                                        guidance_scale=guidance_scale, sampler_args=sampler_args, **guided)
            model_inputs["x"] = out["x_prev"]
            if keep:
                xt.append(out["x_prev"])
                x0s.append(out["estimated_x0"])
                if "x_prev_mean" in out:
                    means.append(out["x_prev_mean"])
                if "x_prev_std" in out:
                    stds.append(out["x_prev_std"])
                if "logprob" in out:
                    lps.append(out["logprob"])
        self.sampler.reset()  # (a multistep sampler lets go of its image-sized history tensor)
        return self._pack(model_inputs["x"], xt, x0s, means, stds, lps, std_dim=1)

    def _denoise_from_image(self, model, model_inputs, cond, strength: float, resample: int, use_tqdm: bool, clamp_x: bool,
                            guidance_scale: float, sampler_args: dict[str, Any], return_intermediates: bool,
                            guided: dict[str, Any] = {}) -> SamplingOutput:
        """Image-to-image (SDEdit, Meng et al. 2022) and inpainting (RePaint, Lugmayr et al. 2022) on the (respaced) chain.

        Start: k = strength_to_steps(steps, strength) steps are run, t = k - 1 .. 0, from x = q(x_t | init_image) at t = k - 1 with
        the noise eps0 = model_inputs["x"] (the initial noise, as in the plain call) or a fresh draw.  strength 1 therefore starts
        from q(x_{T-1} | init_image), not from pure noise: the chain's last level still carries sqrt(alphas_bar[T-1]) of the image
        (6.4e-3 on the linear 1000-step chain).
        Known region (mask 0): after the step at index t, whose x_prev lives at t - 1, it is set to
        sqrt_alphas_bar[t-1] init_image + sqrt(1 - alphas_bar[t-1]) randn with a fresh draw per step, as RePaint does, and to init_image
        itself after the step at t == 0.  The coefficients are the chain's fp64 tables, cast to f32 once per step.
        resample (RePaint's U, jump length 1): every step but the last runs `resample` times; between two repeats x_prev goes back one
        level by x_t = sqrt(1 - betas[t]) x_prev + sqrt(betas[t]) randn.  The denoiser runs resample (k - 1) + 1 times (twice that
        where CFG makes two forwards).
        Intermediates: `xt` holds the starting x and each step's x_prev after the blend (of the last repeat); estimated_x0, xt_mean,
        xt_std and logprob are what the sampler returned, before the blend.  guided: the guided-sampling keywords of
        `one_step_denoise`."""
        init, eps0, m = cond
        k = strength_to_steps(self.steps, strength)
        B = init.shape[0]
        model_inputs["x"], _ = self.add_noise(init, torch.full((B,), k - 1, dtype=torch.int32), eps0)
        keep = return_intermediates
        xt = [model_inputs["x"]] if keep else None
        x0s: list[Tensor] = []
        means: list[Tensor] = []
        stds: list[Tensor] = []
        lps: list[Tensor] = []
        self.sampler.reset()
        for t in tqdm(list(range(k))[::-1], desc="generating image", total=k, disable=not use_tqdm, leave=False):
            repeats = resample if t > 0 else 1
            for r in range(repeats):
                out = self.one_step_denoise(model=model, model_inputs=model_inputs, t=t, clamp_x=clamp_x,
                                            guidance_scale=guidance_scale, sampler_args=sampler_args, **guided)
                if m is not None:  # in place: the sampler's x_prev is a fresh tensor
                    xp = out["x_prev"]
                    if t > 0:
                        a, b = float(self.sqrt_alphas_bar[t - 1]), float((1.0 - self.alphas_bar[t - 1]).sqrt())
                        out["x_prev"] = ops.inpaint_blend(xp, init, torch.randn_like(xp), m, a, b, out=xp)
                    else:
                        out["x_prev"] = ops.inpaint_blend(xp, init, None, m, 1.0, 0.0, out=xp)
                model_inputs["x"] = out["x_prev"]
                if r + 1 < repeats:
                    beta = float(self.betas[t])
                    model_inputs["x"] = ops.inpaint_blend(None, out["x_prev"], torch.randn_like(out["x_prev"]), None,
                                                          (1.0 - beta) ** 0.5, beta**0.5)
            if keep:
                self._record(out, xt, x0s, means, stds, lps)
        self.sampler.reset()  # (a multistep sampler lets go of its image-sized history tensor)
        return self._pack(model_inputs["x"], xt, x0s, means, stds, lps, std_dim=1)
