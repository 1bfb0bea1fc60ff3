"""Rectified-flow modelization (reference diffuse/modelizations/flow.py:16-524) over the HIP kernels.

Host logic (timestep grids, draws, CFG bookkeeping, the sampler loop) stays Python and follows the reference
statement by statement, including its quirks: timesteps are drawn on the CPU global
generator; `t` enters the network unscaled; a constructor `shift` only affects `draw_timesteps` because the
base class builds the grid before `Flow.__init__` stores it; `model_inputs` is mutated in place.
Device arithmetic (noising, loss, x->v, Euler / Euler-Maruyama updates) is `libdiffulab_hip.so`.
GRPO (flow.py:317-380) is out of scope (needs the VLM reward stack).
"""

from __future__ import annotations

import contextlib
import math
from typing import Any

import torch
from torch import Tensor

from ... import ops
from ..samplers.common import StepResult
from ..samplers.flow import AB2, Euler, EulerMaruyama
from ..utils import (SamplingOutput, check_guidance, flow_renoise_coefs, guidance_kwargs, in_guidance_interval, strength_to_steps,
                     to_device)
from .diffusion import Diffusion, mse_head

try:
    from tqdm import tqdm
except ImportError:  # pragma: no cover
    def tqdm(it, **kw):
        return it


class _XToV(torch.autograd.Function):
    """v = (z - xhat) / t  (flow.py:300-303)"""

    @staticmethod
    def forward(ctx, xhat: Tensor, z: Tensor, t: Tensor) -> Tensor:
        ctx.save_for_backward(t)
        return ops.flow_x_to_v(z, xhat.float().contiguous(), t)

    @staticmethod
    def backward(ctx, dv: Tensor):
        (t,) = ctx.saved_tensors
        return ops.flow_x_to_v_bwd(dv.float().contiguous(), t), None, None


NO_VARIATIONAL_BOUND = ("rectified flow has no variational bound: bits per dimension (calc_bpd_loop, evaluate_bpd, val_bpd_batches) "
                        "are evaluated for model_type='gaussian_diffusion' only; the exact likelihood of a flow model is the ODE "
                        "likelihood: Diffuser.evaluate_nll / Flow.calc_nll_loop (train(val_nll_batches=...))")


def _repeat_rows(v: Any, B: int, K: int) -> Any:
    """a per-sample entry of model_inputs (leading dimension B; dicts of such) repeated K times along the batch"""
    if K == 1:
        return v
    if isinstance(v, Tensor) and v.dim() >= 1 and v.shape[0] == B:
        return v.repeat(K, *([1] * (v.dim() - 1)))
    if isinstance(v, dict):
        return {k: _repeat_rows(u, B, K) for k, u in v.items()}
    return v


class Flow(Diffusion):
    sampler_registry = {"euler": Euler, "euler_maruyama": EulerMaruyama, "ab2": AB2}  # "ab2" (second order, multistep) is this project's

    def __init__(self, n_steps: int = 50, sampling_method: str = "euler", schedule: str = "linear",
                 latent_diffusion: bool = False, logits_normal: bool = False, shift: float | None = None,
                 sampler_parameters: dict[str, Any] = {}, prediction_type: str = "v") -> None:
        assert prediction_type in ["v", "x"], (
            "prediction_type must be either 'v' or 'x', noise prediction not supported yet for flow models")
        super().__init__(n_steps=n_steps, sampling_method=sampling_method, schedule=schedule,
                         latent_diffusion=latent_diffusion, sampler_parameters=sampler_parameters)
        self.logits_normal = logits_normal
        self.shift = shift  # after the base class already built the (unshifted) grid -- reference behaviour
        self.x_prediction = prediction_type == "x"

    @staticmethod
    def _shift_timestep(t, alpha: float):
        return alpha * t / (1 + (alpha - 1) * t)

    def set_steps(self, n_steps: int, schedule: str = "linear", shift: float | None = None) -> None:
        self.shift = shift
        if schedule != "linear":
            raise NotImplementedError("Only linear schedule is supported for the moment")
        self.schedule = schedule
        grid: list[float] = torch.linspace(1, 0, n_steps + 1).tolist()
        if self.shift is not None:
            grid = [self._shift_timestep(t, self.shift) for t in grid]
        self.timesteps = grid
        self.steps = n_steps
        self.sampler.set_steps(self.timesteps)

    def at(self, timesteps: Tensor) -> Tensor:
        return 1 - timesteps

    def bt(self, timesteps: Tensor) -> Tensor:
        return timesteps

    def draw_timesteps(self, batch_size: int) -> Tensor:
        if self.logits_normal:
            t = torch.sigmoid(torch.randn((batch_size), dtype=torch.float32))
        else:
            t = torch.rand((batch_size), dtype=torch.float32)
        if self.shift is not None:
            t = self._shift_timestep(t, self.shift)
        if self.x_prediction:
            t = t.clamp(min=0.05)
        return t

    def get_v(self, model, model_inputs, t_curr: float) -> Tensor:
        p0 = next(model.parameters())
        timesteps = torch.full((model_inputs["x"].shape[0],), t_curr, device=p0.device, dtype=p0.dtype)
        prediction = model(**model_inputs, timesteps=timesteps)["x"]
        if self.x_prediction:
            return (model_inputs["x"] - prediction) / max(t_curr, 0.05)
        return prediction

    def _get_v_pair(self, model, model_inputs, t_curr: float):
        fn = getattr(model, "forward_cfg_pair", None)
        if fn is None:
            return None
        p0 = next(model.parameters())
        timesteps = torch.full((model_inputs["x"].shape[0],), t_curr, device=p0.device, dtype=p0.dtype)
        pair = fn(timesteps, **model_inputs)
        if pair is None or not self.x_prediction:
            return pair
        return tuple((model_inputs["x"] - pred) / max(t_curr, 0.05) for pred in pair)

    def one_step_denoise(self, model, model_inputs, t_prev: float, t_curr: float, guidance_scale: float,
                         sampler_args: dict[str, Any] = {}, guidance_rescale: float = 0.0,
                         guidance_interval: tuple[float, float] | None = None, dynamic_threshold: float | None = None,
                         threshold_max: float | None = None) -> StepResult:
        """guidance_rescale / guidance_interval (this project's): CFG rescale reaches the sampler as a keyword; a step whose t_curr lies
        outside the interval makes the one conditional forward.  dynamic_threshold is refused: the flow step has no x0 clamp."""
        if guidance_rescale or guidance_interval is not None or dynamic_threshold is not None or threshold_max is not None:
            check_guidance(guidance_scale, guidance_rescale, guidance_interval, dynamic_threshold, threshold_max, flow=True)
            if guidance_rescale:
                sampler_args = {**sampler_args, "guidance_rescale": guidance_rescale}
            if not in_guidance_interval(guidance_interval, t_curr):
                guidance_scale = 0
        if guidance_scale > 0:
            # flow.py:256-259 makes two forwards (p = 0, then p = 1: every label dropped).  A denoiser whose `p` only reaches the
            # label drop runs them as ONE forward over [x ; x] (FlatArenaDenoiser.forward_cfg_pair: same values per row, half the
            # weight streaming); the combine v_u + g (v - v_u) is fused into the step kernel either way.
            pair = self._get_v_pair(model, model_inputs, t_curr)
            if pair is None:
                pair = (self.get_v(model, {**model_inputs, "p": 0}, t_curr), self.get_v(model, {**model_inputs, "p": 1}, t_curr))
            return self.sampler.step(model_inputs["x"], pair[0], t_curr, t_prev, v_uncond=pair[1],
                                     guidance_scale=guidance_scale, **sampler_args)
        v = self.get_v(model, {**model_inputs, "p": 0}, t_curr)
        return self.sampler.step(model_inputs["x"], v, t_curr, t_prev, **sampler_args)

    def compute_loss(self, model, model_inputs, timesteps: Tensor, noise: Tensor | None = None, extra_losses=[],
                     extra_args: dict[str, Any] = {}) -> dict[str, Tensor]:
        x_0 = model_inputs["x"]  # add_noise writes a fresh tensor, so no clone is needed to keep x_0
        model_inputs["x"], noise = self.add_noise(x_0, timesteps, noise)
        prediction = model(**model_inputs, timesteps=timesteps)
        pred = prediction["x"]
        if self.x_prediction:
            t_dev = to_device(timesteps, pred.device, torch.float32)
            pred = _XToV.apply(pred, model_inputs["x"], t_dev) if pred.requires_grad else ops.flow_x_to_v(
                model_inputs["x"], pred.float().contiguous(), t_dev)
            prediction["x"] = pred
        # mean_b(mean_chw(((eps - x0) - v)^2)) == global mean for equal-size samples (flow.py:306-309)
        loss_dict = {"loss": mse_head(pred, noise, x_0, ops.LOSS_FLOW)}
        for extra_loss in extra_losses:
            loss_dict[extra_loss.name] = extra_loss(**extra_args)
        return loss_dict

    def compute_loss_grpo(self, *a: Any, **k: Any):
        raise NotImplementedError("GRPO fine-tuning (flow.py:317-380) is outside the MI355X hot-path scope (DESIGN.md)")

    def calc_bpd_loop(self, *a: Any, **k: Any):
        raise NotImplementedError(NO_VARIATIONAL_BOUND)

    # ------------------------------------------------------------------ ODE likelihood (this project's; the reference has none)
    def _nll_plan(self, model, model_inputs, method: str, n_probes: int, probe: str, probes: Tensor | None, dequantize: bool | None,
                  dequant_noise: Tensor | None) -> tuple[int, bool]:
        """every check of calc_nll_loop, before any device work -> (number of probes per sample, dequantize)"""
        from ...networks.denoisers.common import FlatArenaDenoiser

        if torch.is_inference_mode_enabled():
            raise RuntimeError("calc_nll_loop differentiates the denoiser with respect to its input: it cannot run under "
                               "torch.inference_mode() (torch.no_grad() is fine)")
        if self.x_prediction:
            raise NotImplementedError("calc_nll_loop: prediction_type='x' is not evaluated: v = (z - xhat) / t is singular at the data "
                                      "end t = 0 of the ODE")
        if isinstance(model, FlatArenaDenoiser) and not model.input_grad_capable:
            raise NotImplementedError(f"calc_nll_loop: diffulab_amd.{type(model).__name__} returns no gradient with respect to its input "
                                      "(input_grad_capable is False): the divergence estimate needs one; built for MMDiT(simple_dit=True)")
        if method not in ("euler", "heun"):
            raise ValueError(f"method must be 'euler' or 'heun' (got {method!r})")
        if probe not in ("rademacher", "gaussian"):
            raise ValueError(f"probe must be 'rademacher' or 'gaussian' (got {probe!r})")
        if isinstance(n_probes, bool) or not isinstance(n_probes, int) or n_probes < 1:
            raise ValueError(f"n_probes must be a positive integer (got {n_probes!r})")
        x = model_inputs["x"]
        shape = tuple(x.shape)
        if probes is not None:
            if not isinstance(probes, Tensor) or probes.dim() != x.dim() + 1 or tuple(probes.shape[1:]) != shape or probes.shape[0] < 1:
                raise ValueError(f"probes must be [K, {', '.join(map(str, shape))}] (got "
                                 f"{tuple(probes.shape) if isinstance(probes, Tensor) else type(probes).__name__})")
            n_probes = probes.shape[0]
        dequantize = (not self.latent_diffusion) if dequantize is None else bool(dequantize)
        if dequant_noise is not None:
            if not isinstance(dequant_noise, Tensor) or tuple(dequant_noise.shape) != shape:
                raise ValueError(f"dequant_noise must be {list(shape)} (got "
                                 f"{list(dequant_noise.shape) if isinstance(dequant_noise, Tensor) else type(dequant_noise).__name__})")
            if not dequantize:
                raise ValueError("dequant_noise given with dequantize=False")
            if bool((dequant_noise < 0).any()) or bool((dequant_noise >= 1).any()):
                raise ValueError("dequant_noise must lie in [0, 1)")
        return n_probes, dequantize

    def calc_nll_loop(self, model, model_inputs, method: str = "heun", n_probes: int = 1, probe: str = "rademacher",
                      probes: Tensor | None = None, dequantize: bool | None = None, dequant_noise: Tensor | None = None,
                      use_tqdm: bool = False) -> dict[str, Tensor]:
        """The negative log-likelihood of the clean data model_inputs["x"] [B, C, *spatial] under the model's probability-flow ODE,
        by the instantaneous change of variables (Chen et al. 2018) with Hutchinson's divergence estimate (Grathwohl et al. 2019,
        FFJORD).  With z_t = (1 - t) x0 + t eps data sits at t = 0 and noise at t = 1: dx/dt = v(x, t) is integrated upward over this
        object's own grid (`self.timesteps` ascending, so `set_steps` and `shift` apply) and
            log p0(x) = log N(x1; 0, I) + integral_0^1 div v dt.
        div v is estimated per sample as sum(eps * J^T eps), J^T eps from `torch.autograd.grad(pred, x, eps)` through the conditional
        forward (p = 0; every other entry of model_inputs is passed through; a FlatArenaDenoiser runs inside `input_grad_only()`, so no
        `p.grad` is touched).  method "euler": one evaluation per step; "heun": two (x_mid = x + h v1, x_new = x + h/2 (v1 + v2)), the
        divergence with the same trapezoid weights.  One probe per row, drawn once and held along the trajectory: `probe` "rademacher"
        or "gaussian"; n_probes = K repeats the rows K times along the batch and averages per sample; `probes` [K, B, C, *spatial]
        supplies them.  dequantize (default: not latent_diffusion) adds (u - 0.5) * 2 / 255, u ~ U[0, 1) or `dequant_noise`
        [B, C, *spatial]: uniform noise over the 8-bit bins of width 2/255 that `evaluate_bpd`'s t = 0 term uses.
        Behind each backward the loop makes one `dl_hutchinson_step` launch (state update and row sums); nothing is read back to the
        host inside it, and model_inputs is not mutated.
        -> f32, D_el = C * prod(spatial): "nll" [B] = -(log p0) / D_el, nats per dimension; "prior" [B] = 0.5 mean(x1^2) + 0.5 log(2 pi);
        "div" [B] = the integrated divergence / D_el; "div_terms" [B, n_evals] = every evaluation's estimate / D_el, unweighted, averaged
        over the probes, in evaluation order; "x1" [B, C, *spatial] = the latent at t = 1; and, unless latent_diffusion, "total_bpd" [B]
        = nll / ln 2 + log2(127.5), bits per dimension of the 8-bit data.  A bad argument raises before any device work."""
        from ...networks.denoisers.common import FlatArenaDenoiser

        K, dequantize = self._nll_plan(model, model_inputs, method, n_probes, probe, probes, dequantize, dequant_noise)
        with torch.no_grad():
            x0 = model_inputs["x"].detach().float().contiguous()
            dev, B, tail = x0.device, x0.shape[0], tuple(x0.shape[1:])
            n_el = x0.numel() // B
            if dequantize:
                u = torch.rand_like(x0) if dequant_noise is None else dequant_noise.to(device=dev, dtype=torch.float32)
                x0 = x0 + (u - 0.5) * (2.0 / 255.0)
            R = K * B
            x = x0.repeat(K, *([1] * len(tail))).contiguous()
            if probes is not None:
                eps = probes.to(device=dev, dtype=torch.float32).reshape(R, *tail).contiguous()
            elif probe == "rademacher":
                eps = torch.randint(0, 2, (R, *tail), device=dev).float().mul_(2.0).sub_(1.0)
            else:
                eps = torch.randn(R, *tail, device=dev, dtype=torch.float32)
            rest = {k: _repeat_rows(v, B, K) for k, v in model_inputs.items() if k not in ("x", "p")}
            grid = sorted(float(t) for t in self.timesteps)
            heun = method == "heun"
            n_evals = (2 if heun else 1) * (len(grid) - 1)
            table = torch.empty(R, n_evals, device=dev, dtype=torch.float32)
            nshare = ops.lib().call("dl_mse_loss_partials", n_el)
            partial = torch.empty(R * nshare, device=dev, dtype=torch.float32) if nshare > 1 else None
            x_mid = torch.empty_like(x) if heun else None
            p0 = next(model.parameters(), None)
            t_dev, t_dtype = (p0.device, p0.dtype) if p0 is not None else (dev, torch.float32)
        only = model.input_grad_only if isinstance(model, FlatArenaDenoiser) else contextlib.nullcontext

        def evaluate(xin: Tensor, t: float) -> tuple[Tensor, Tensor]:
            """(v, J^T eps) at (xin, t)"""
            with torch.enable_grad(), only():
                xin = xin.detach().requires_grad_(True)
                pred = model(**rest, x=xin, p=0, timesteps=torch.full((R,), t, device=t_dev, dtype=t_dtype))["x"]
                (g,) = torch.autograd.grad(pred, xin, eps.to(pred.dtype))
            return pred.detach().float().contiguous(), g.detach().float().contiguous()

        weights: list[float] = []
        scale = 1.0 / n_el
        steps = list(zip(grid[:-1], grid[1:]))
        for i, (t0, t1) in enumerate(tqdm(steps, desc="evaluating the likelihood", total=len(steps), disable=not use_tqdm, leave=False)):
            h = t1 - t0
            v1, g1 = evaluate(x, t0)
            if not heun:
                ops.hutchinson_step(g1, eps, table, i, scale, x=x, v=v1, a=h, x_out=x, partial=partial)
                weights.append(h)
                continue
            ops.hutchinson_step(g1, eps, table, 2 * i, scale, x=x, v=v1, a=h, x_out=x_mid, partial=partial)
            v2, g2 = evaluate(x_mid, t1)
            ops.hutchinson_step(g2, eps, table, 2 * i + 1, scale, x=x, v=v2, a=0.5 * h, v0=v1, b=0.5 * h, x_out=x, partial=partial)
            weights += [0.5 * h, 0.5 * h]
        with torch.no_grad():
            terms = table.view(K, B, n_evals).mean(0)
            div = (terms * torch.tensor(weights, dtype=torch.float32).to(dev)).sum(1)
            x1 = x[:B].clone()  # (the trajectory does not depend on the probe: every repeat of a sample ends at the same latent)
            prior = ops.normal_nll_rows(x1)
            out = {"nll": prior - div, "prior": prior, "div": div, "div_terms": terms, "x1": x1}
            if not self.latent_diffusion:
                out["total_bpd"] = out["nll"] / math.log(2.0) + math.log2(127.5)
        return out

    def add_noise(self, x: Tensor, timesteps: Tensor, noise: Tensor | None = None) -> tuple[Tensor, Tensor]:
        x = x.float().contiguous()
        if noise is None:
            noise = torch.randn_like(x)
        noise = noise.to(device=x.device, dtype=torch.float32).contiguous()
        assert noise.shape == x.shape
        assert timesteps.shape[0] == x.shape[0]
        t = to_device(timesteps, x.device, torch.float32)
        return ops.flow_add_noise(x, noise, t), noise

    @torch.inference_mode()
    def denoise(self, model, model_inputs, data_shape: tuple[int, ...] | None = None, use_tqdm: bool = True,
                clamp_x: bool = False, guidance_scale: float = 0, sampler_args: dict[str, Any] = {},
                guidance_rescale: float = 0.0, guidance_interval: tuple[float, float] | None = None,
                dynamic_threshold: float | None = None, threshold_max: float | None = None,
                return_intermediates: bool = False, init_image: Tensor | None = None, strength: float = 1.0,
                mask: Tensor | None = None, resample: int = 1) -> SamplingOutput:
        """init_image / strength / mask / resample (this project's; the reference has neither): see `_denoise_from_image`.
        guidance_rescale / guidance_interval (this project's): see `one_step_denoise`; validated here, before any device work.  At
        their defaults this is the reference's loop, call for call."""
        check_guidance(guidance_scale, guidance_rescale, guidance_interval, dynamic_threshold, threshold_max, flow=True)
        guided = guidance_kwargs(guidance_rescale, guidance_interval, dynamic_threshold, threshold_max)
        cond = self._image_conditioning(model, model_inputs, data_shape, init_image, strength, mask, resample)
        if cond is not None:
            return self._denoise_from_image(model, model_inputs, cond, strength, resample, use_tqdm, clamp_x, guidance_scale,
                                            sampler_args, return_intermediates, guided)
        p0 = next(model.parameters())
        if "x" not in model_inputs:
            assert data_shape is not None, "'data_shape' must be provided if 'x' is not in model_inputs"
            model_inputs["x"] = torch.randn(data_shape, device=p0.device, dtype=p0.dtype)
        keep = return_intermediates
        xt = [model_inputs["x"]] if keep else None
        x0s: list[Tensor] = []
        means: list[Tensor] = []
        stds: list[Tensor] = []
        lps: list[Tensor] = []
        pairs = zip(self.timesteps[:-1], self.timesteps[1:])
        self.sampler.reset()
        for t_curr, t_prev in tqdm(pairs, desc="generating image", total=self.steps, disable=not use_tqdm, leave=False):
            out = self.one_step_denoise(model, model_inputs, t_curr=t_curr, t_prev=t_prev, guidance_scale=guidance_scale,
                                        sampler_args=sampler_args, **guided)
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
        if clamp_x:
            model_inputs["x"] = model_inputs["x"].clamp(-1, 1)
        return self._pack(model_inputs["x"], xt, x0s, means, stds, lps, std_dim=0)  # std stacked on dim 0 (flow.py:520)

    def _denoise_from_image(self, model, model_inputs, cond, strength: float, resample: int, use_tqdm: bool, clamp_x: bool,
                            guidance_scale: float, sampler_args: dict[str, Any], return_intermediates: bool,
                            guided: dict[str, Any] = {}) -> SamplingOutput:
        """Image-to-image (SDEdit, Meng et al. 2022) and inpainting (RePaint, Lugmayr et al. 2022) on the grid of `self.timesteps`.

        Start: k = strength_to_steps(steps, strength) steps are run, from index i0 = steps - k: x = (1 - t) init_image + t eps0 at
        t = timesteps[i0], eps0 = model_inputs["x"] (the initial noise, as in the plain call) or a fresh draw.  strength 1 starts at
        t = 1, i.e. from eps0 itself.
        Known region (mask 0): after every step to t_prev it is set to (1 - t_prev) init_image + t_prev eps0 -- always the same eps0,
        so it follows one trajectory and ends at init_image exactly.
        resample (RePaint's U, jump length 1): every step but the last runs `resample` times; between two repeats x_prev goes back to
        t_curr by x_t = a x_prev + s randn, a = (1 - t_curr) / (1 - t_prev), s = sqrt(t_curr^2 - a^2 t_prev^2), which keeps the
        marginal (1 - t_curr) x0 + t_curr eps.  The denoiser runs resample (k - 1) + 1 times (twice that where CFG makes two forwards).
        Intermediates: `xt` holds the starting x and each step's x_prev after the blend (of the last repeat); estimated_x0, xt_mean,
        xt_std and logprob are what the sampler returned, before the blend.  clamp_x clamps the final sample, as in the plain loop (the
        known region too, where init_image leaves [-1, 1]).  guided: the guided-sampling keywords of `one_step_denoise`."""
        init, eps0, m = cond
        k = strength_to_steps(self.steps, strength)
        i0 = self.steps - k
        B = init.shape[0]
        model_inputs["x"], _ = self.add_noise(init, torch.full((B,), self.timesteps[i0], dtype=torch.float32), eps0)
        keep = return_intermediates
        xt = [model_inputs["x"]] if keep else None
        x0s: list[Tensor] = []
        means: list[Tensor] = []
        stds: list[Tensor] = []
        lps: list[Tensor] = []
        pairs = list(zip(self.timesteps[i0:-1], self.timesteps[i0 + 1:]))
        self.sampler.reset()
        for j, (t_curr, t_prev) in enumerate(tqdm(pairs, desc="generating image", total=k, disable=not use_tqdm, leave=False)):
            repeats = resample if j + 1 < k else 1
            for r in range(repeats):
                out = self.one_step_denoise(model, model_inputs, t_curr=t_curr, t_prev=t_prev, guidance_scale=guidance_scale,
                                            sampler_args=sampler_args, **guided)
                if m is not None:  # in place: the sampler's x_prev is a fresh tensor
                    out["x_prev"] = ops.inpaint_blend(out["x_prev"], init, eps0, m, 1.0 - t_prev, t_prev, out=out["x_prev"])
                model_inputs["x"] = out["x_prev"]
                if r + 1 < repeats:
                    a, s = flow_renoise_coefs(t_curr, t_prev)
                    model_inputs["x"] = ops.inpaint_blend(None, out["x_prev"], torch.randn_like(out["x_prev"]), None, a, s)
            if keep:
                self._record(out, xt, x0s, means, stds, lps)
        self.sampler.reset()  # (a multistep sampler lets go of its image-sized history tensor)
        if clamp_x:
            model_inputs["x"] = model_inputs["x"].clamp(-1, 1)
        return self._pack(model_inputs["x"], xt, x0s, means, stds, lps, std_dim=0)
