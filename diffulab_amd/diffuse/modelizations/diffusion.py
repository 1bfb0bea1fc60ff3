"""`Diffusion` plugin base (reference diffuse/modelizations/diffusion.py:13-244): owns the sampler built from
`sampler_registry`, the step grid, and declares the six methods a modelization implements."""

from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Any

import torch
from torch import Tensor

from ... import ops
from ..samplers.common import Sampler, StepResult
from ..utils import SamplingOutput, check_image_conditioning


class _MSEHead(torch.autograd.Function):
    """loss = mean((target - pred)^2) with target = a - b (flow) or a (eps) -- dl_mse_loss_fwd / _bwd"""

    @staticmethod
    def forward(ctx, pred: Tensor, a: Tensor, b: Tensor | None, mode: int) -> Tensor:
        pred = pred.float().contiguous()
        ctx.save_for_backward(pred, a, b)
        ctx.mode = mode
        return ops.mse_loss_fwd(pred, a, b, mode)

    @staticmethod
    def backward(ctx, gout: Tensor):
        pred, a, b = ctx.saved_tensors
        # the upstream gradient stays on the device (no .item() sync): the kernel multiplies by *gscale_dev
        gdev = gout.float().contiguous() if gout is not None else None
        return ops.mse_loss_bwd(pred, a, b, 1.0, ctx.mode, gscale_dev=gdev), None, None, None


def mse_head(pred: Tensor, a: Tensor, b: Tensor | None, mode: int) -> Tensor:
    a = a.float().contiguous()
    b = None if b is None else b.float().contiguous()
    if pred.requires_grad:
        return _MSEHead.apply(pred, a, b, mode)
    return ops.mse_loss_fwd(pred.float().contiguous(), a, b, mode)


class _HybridHead(torch.autograd.Function):
    """(mse, vb) of a learned-variance [B, 2C, ...] prediction -- dl_vlb_loss_fwd / _bwd.  mse = mean((eps - mean half)^2); vb = the
    variational bound in bits per dimension with the predicted mean frozen, so it trains the variance half only (Nichol & Dhariwal
    2021, eq. 16; the reference leaves this loss as a TODO, gaussian_diffusion.py:267)."""

    @staticmethod
    def forward(ctx, pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, tables: Tensor, mean_type: int, var_mode: int):
        pred = pred.float().contiguous()
        ctx.save_for_backward(pred, eps, x0, xt, t, tables)
        ctx.modes = (mean_type, var_mode)
        both = ops.vlb_loss_fwd(pred, eps, x0, xt, t, tables, mean_type, var_mode)
        return both[0], both[1]

    @staticmethod
    def backward(ctx, g_mse: Tensor, g_vb: Tensor):
        # both upstream gradients stay on the device (an unused output arrives as zeros); one kernel writes the whole dpred
        dpred = ops.vlb_loss_bwd(*ctx.saved_tensors, *ctx.modes, g_mse.float().contiguous(), g_vb.float().contiguous())
        return dpred, None, None, None, None, None, None, None


def hybrid_head(pred: Tensor, eps: Tensor, x0: Tensor, xt: Tensor, t: Tensor, tables: Tensor, mean_type: int,
                var_mode: int) -> tuple[Tensor, Tensor]:
    eps, x0, xt = (v.float().contiguous() for v in (eps, x0, xt))
    if pred.requires_grad:
        return _HybridHead.apply(pred, eps, x0, xt, t, tables, mean_type, var_mode)
    both = ops.vlb_loss_fwd(pred.float().contiguous(), eps, x0, xt, t, tables, mean_type, var_mode)
    return both[0], both[1]


class _GDHead(torch.autograd.Function):
    """the loss of any parameterisation of the mean output -- dl_gd_loss_fwd / _bwd.  The regression target (epsilon, x0, the posterior
    mean or v) is formed inside the kernels from eps, x0, xt; `weight` is a per-timestep table or None.  Fixed variances: one scalar,
    the weighted mse.  Learned variances: (weighted mse of the mean half, variational bound in bits per dimension), the bound as
    `_HybridHead` has it, with the predicted mean derived from the same parameterisation and frozen."""

    @staticmethod
    def forward(ctx, pred: Tensor, eps, x0, xt, t: Tensor, tables: Tensor, weight, target: int, var_mode: int):
        pred = pred.float().contiguous()
        ctx.save_for_backward(pred, eps, x0, xt, t, tables, weight)
        ctx.modes = (target, var_mode)
        out = ops.gd_loss_fwd(pred, eps, x0, xt, t, tables, target, weight, var_mode)
        return out if var_mode == ops.VAR_FIXED else (out[0], out[1])

    @staticmethod
    def backward(ctx, g_mse: Tensor, g_vb: Tensor | None = None):
        # the upstream gradients stay on the device (an unused output arrives as zeros); one kernel writes the whole dpred
        pred, eps, x0, xt, t, tables, weight = ctx.saved_tensors
        target, var_mode = ctx.modes
        dpred = ops.gd_loss_bwd(pred, eps, x0, xt, t, tables, target, weight, var_mode, g_mse.float().contiguous(),
                                None if g_vb is None else g_vb.float().contiguous())
        return dpred, None, None, None, None, None, None, None, None


def gd_head(pred: Tensor, eps: Tensor | None, x0: Tensor | None, xt: Tensor | None, t: Tensor, tables: Tensor, target: int,
            weight: Tensor | None = None, var_mode: int = ops.VAR_FIXED):
    """-> the scalar loss (var_mode VAR_FIXED) or (mse, vb) (learned variances); eps / x0 / xt may be None where the mode does not
    read them (the epsilon target with fixed variances reads eps only)"""
    eps, x0, xt = (None if v is None else v.float().contiguous() for v in (eps, x0, xt))
    if pred.requires_grad:
        return _GDHead.apply(pred, eps, x0, xt, t, tables, weight, target, var_mode)
    out = ops.gd_loss_fwd(pred.float().contiguous(), eps, x0, xt, t, tables, target, weight, var_mode)
    return out if var_mode == ops.VAR_FIXED else (out[0], out[1])


class _GDRowsHead(torch.autograd.Function):
    """`_GDHead` with every sample's loss kept -- dl_gd_loss_rows_fwd / _bwd: for a per-sample importance weight `imp` (loss-aware
    timestep sampling) and for loss_type "vlb", the variational bound trained without the stop-gradient on the predicted mean.
    -> (loss f32 [2] = the two batch scalars, rows): only `loss` is differentiable; rows = the detached per-sample tensors."""

    @staticmethod
    def forward(ctx, pred: Tensor, eps, x0, xt, t: Tensor, tables: Tensor, weight, imp, target: int, var_mode: int, loss_type: int,
                vb_scale: float):
        pred = pred.float().contiguous()
        ctx.save_for_backward(pred, eps, x0, xt, t, tables, weight, imp)
        ctx.modes = (target, var_mode, loss_type)
        mse_row, vb_row, total_row, loss = ops.gd_loss_rows_fwd(pred, eps, x0, xt, t, tables, target, weight, imp, var_mode, loss_type,
                                                                vb_scale)
        ctx.mark_non_differentiable(mse_row, total_row, *(() if vb_row is None else (vb_row,)))
        if vb_row is None:
            return loss[0], mse_row, total_row
        return loss[0], loss[1], mse_row, vb_row, total_row

    @staticmethod
    def backward(ctx, g_mse: Tensor, *rest):
        # the upstream gradients stay on the device (an unused output arrives as zeros); one kernel writes the whole dpred
        pred, eps, x0, xt, t, tables, weight, imp = ctx.saved_tensors
        target, var_mode, loss_type = ctx.modes
        g_vb = None if var_mode == ops.VAR_FIXED else rest[0].float().contiguous()
        dpred = ops.gd_loss_rows_bwd(pred, eps, x0, xt, t, tables, target, weight, imp, var_mode, loss_type,
                                     g_mse.float().contiguous(), g_vb)
        return (dpred,) + (None,) * 11


def gd_rows_head(pred: Tensor, eps: Tensor | None, x0: Tensor | None, xt: Tensor | None, t: Tensor, tables: Tensor, target: int,
                 weight: Tensor | None, imp: Tensor | None, var_mode: int, loss_type: int, vb_scale: float) -> dict[str, Tensor]:
    """-> {"loss_mse", "loss_vb" (learned variances), "mse", "vb" (learned variances), "total"}: the two batch scalars, carrying the
    importance weights and differentiable in pred, and the per-sample f32 [B] tensors before those weights, detached"""
    eps, x0, xt = (None if v is None else v.float().contiguous() for v in (eps, x0, xt))
    fixed = var_mode == ops.VAR_FIXED
    if pred.requires_grad:
        out = _GDRowsHead.apply(pred, eps, x0, xt, t, tables, weight, imp, target, var_mode, loss_type, vb_scale)
    else:
        mse_row, vb_row, total_row, loss = ops.gd_loss_rows_fwd(pred.float().contiguous(), eps, x0, xt, t, tables, target, weight, imp,
                                                                var_mode, loss_type, vb_scale)
        out = (loss[0], mse_row, total_row) if fixed else (loss[0], loss[1], mse_row, vb_row, total_row)
    return dict(zip(("loss_mse", "mse", "total") if fixed else ("loss_mse", "loss_vb", "mse", "vb", "total"), out))


class Diffusion(ABC):
    sampler_registry: dict[str, type[Sampler]]

    def __init__(self, n_steps: int, sampling_method: str = "euler", schedule: str = "linear",
                 latent_diffusion: bool = False, sampler_parameters: dict[str, Any] = {}) -> None:
        assert sampling_method in self.sampler_registry, (
            f"Unknown sampling method '{sampling_method}'. Available methods: {list(self.sampler_registry.keys())}")
        self.sampler = self.sampler_registry[sampling_method](**sampler_parameters)
        self.timesteps: list[float] = []
        self.steps: int = n_steps
        self.sampling_method = sampling_method
        self.schedule = schedule
        self.latent_diffusion = latent_diffusion
        self.set_steps(n_steps, schedule=schedule)

    @abstractmethod
    def set_steps(self, n_steps: int, schedule: str) -> None: ...

    @abstractmethod
    def one_step_denoise(self, model, model_inputs, guidance_scale: float, *args: Any, **kwargs: Any) -> StepResult: ...

    @abstractmethod
    def compute_loss(self, model, model_inputs, timesteps: Tensor, noise: Tensor | None = None, extra_losses=[],
                     extra_args: dict[str, Any] = {}) -> dict[str, Tensor]: ...

    @abstractmethod
    def add_noise(self, x: Tensor, timesteps: Tensor, noise: Tensor | None = None) -> tuple[Tensor, Tensor]: ...

    @abstractmethod
    def denoise(self, model, model_inputs, data_shape=None, use_tqdm: bool = True, clamp_x: bool = False,
                guidance_scale: float = 0, sampler_args: dict[str, Any] = {}, guidance_rescale: float = 0.0,
                guidance_interval: tuple[float, float] | None = None, dynamic_threshold: float | None = None,
                threshold_max: float | None = None,
                return_intermediates: bool = False, init_image: Tensor | None = None, strength: float = 1.0,
                mask: Tensor | None = None, resample: int = 1) -> SamplingOutput: ...

    @abstractmethod
    def draw_timesteps(self, batch_size: int) -> Tensor: ...

    # Image-to-image (SDEdit, Meng et al. 2022) and inpainting (RePaint, Lugmayr et al. 2022), which the reference does not have.
    # Shared by both heads: the arguments are validated on the host before anything touches the device, then brought to the f32
    # contiguous form `ops.inpaint_blend` reads.
    @staticmethod
    def _image_conditioning(model, model_inputs, data_shape, init_image: Tensor | None, strength: float, mask: Tensor | None,
                            resample: int) -> tuple[Tensor, Tensor, Tensor | None] | None:
        """-> None with all four arguments at their defaults (the caller then takes the plain sampling path untouched), else
        (init_image, eps0, mask or None) as f32 contiguous tensors on the model's device; eps0 is the run's initial noise"""
        shape = tuple(model_inputs["x"].shape) if "x" in model_inputs else (None if data_shape is None else tuple(data_shape))
        if not check_image_conditioning(shape, init_image, strength, mask, resample):
            return None
        p0 = next(model.parameters())
        init = init_image.to(device=p0.device, dtype=torch.float32).contiguous()
        # model_inputs["x"] keeps its meaning: the initial noise
        eps0 = model_inputs["x"] if "x" in model_inputs else torch.randn(tuple(init.shape), device=p0.device, dtype=p0.dtype)
        eps0 = eps0.to(device=p0.device, dtype=torch.float32).contiguous()
        m = None if mask is None else mask.to(device=p0.device, dtype=torch.float32).contiguous()
        return init, eps0, m

    @staticmethod
    def _record(out: StepResult, xt, x0s, means, stds, lps) -> None:
        xt.append(out["x_prev"])
        x0s.append(out["estimated_x0"])
        if "x_prev_mean" in out:
            means.append(out["x_prev_mean"])
        if "x_prev_std" in out:
            stds.append(out["x_prev_std"])
        if "logprob" in out:
            lps.append(out["logprob"])

    # shared by both heads: stack what the sampler loop collected (flow.py:510-522 / gaussian_diffusion.py:436-445)
    @staticmethod
    def _pack(x: Tensor, xt, x0, mean, std, lp, std_dim: int) -> SamplingOutput:
        out: SamplingOutput = {"x": x}
        if xt is not None:
            out["xt"] = torch.stack(xt, dim=1)
            out["estimated_x0"] = torch.stack(x0, dim=1)
            if mean:
                out["xt_mean"] = torch.stack(mean, dim=1)
            if std:
                out["xt_std"] = torch.stack(std, dim=std_dim)
            if lp:
                out["logprob"] = torch.stack(lp, dim=1)
        return out
