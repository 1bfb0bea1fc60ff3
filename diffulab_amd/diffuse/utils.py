"""Carriers shared by the diffusion heads (reference diffuse/utils.py:6-28, samplers/common.py:7-32)."""

from __future__ import annotations

import math
from typing import TypedDict

import torch
from torch import Tensor

try:
    from typing import NotRequired, Required
except ImportError:
    from typing_extensions import NotRequired, Required


class SamplingOutput(TypedDict, total=False):
    x: Required[Tensor]
    estimated_x0: NotRequired[Tensor]
    xt: NotRequired[Tensor]
    xt_mean: NotRequired[Tensor]
    xt_std: NotRequired[Tensor]
    logprob: NotRequired[Tensor]


def f32_table(table_fp64: Tensor, device: torch.device) -> Tensor:
    """fp64 schedule table -> fp32 device table: the same rounding `extract_into_tensor` applies per gather
    (diffuse/utils.py:16 `.float()`), hoisted out of the loop."""
    return table_fp64.to(torch.float32).to(device).contiguous()


def strength_to_steps(steps: int, strength: float) -> int:
    """the number of sampler steps an image-to-image run makes: k = clamp(floor(strength * steps + 0.5), 1, steps).  strength 1 runs
    the whole chain; a strength too small for one step still runs the last one."""
    return max(1, min(int(steps), int(math.floor(float(strength) * steps + 0.5))))


def flow_renoise_coefs(t_curr: float, t_prev: float) -> tuple[float, float]:
    """(a, s) of x_t = a x_prev + s randn, which takes the rectified-flow marginal (1 - t_prev) x0 + t_prev eps back to
    (1 - t_curr) x0 + t_curr eps: a = (1 - t_curr) / (1 - t_prev), s^2 = t_curr^2 - a^2 t_prev^2 (t_prev < t_curr, t_prev < 1)"""
    a = (1.0 - t_curr) / (1.0 - t_prev)
    return a, max(t_curr * t_curr - a * a * t_prev * t_prev, 0.0) ** 0.5


def check_image_conditioning(shape: tuple[int, ...] | None, init_image: Tensor | None, strength: float, mask: Tensor | None,
                             resample: int) -> bool:
    """validate the image-to-image / inpainting arguments of `Diffuser.generate` / `Diffusion.denoise` against `shape`, the shape of the
    generated tensor (None: it follows init_image).  Host checks only, apart from one min / max over the mask.  -> False when all four
    are at their defaults (the plain sampling path), else True; a ValueError names the offending argument."""
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 < strength <= 1.0:
        raise ValueError(f"strength must be a number in (0, 1], got {strength!r}")
    if isinstance(resample, bool) or not isinstance(resample, int) or resample < 1:
        raise ValueError(f"resample must be an integer >= 1, got {resample!r}")
    if init_image is None:
        if strength < 1.0:
            raise ValueError(f"strength={strength} < 1 needs init_image: without one the sampler starts from pure noise")
        if mask is not None:
            raise ValueError("mask needs init_image: the region it keeps is taken from there")
        if resample > 1:
            raise ValueError(f"resample={resample} > 1 needs mask (and init_image): it is RePaint's resampling of an inpainting run")
        return False
    if resample > 1 and mask is None:
        raise ValueError(f"resample={resample} > 1 needs mask: it is RePaint's resampling of an inpainting run")
    if not isinstance(init_image, Tensor) or init_image.dim() < 3:
        raise ValueError("init_image must be a [B, C, *spatial] tensor")
    if shape is not None and tuple(init_image.shape) != tuple(shape):
        raise ValueError(f"init_image has shape {tuple(init_image.shape)}, the generated tensor {tuple(shape)}")
    if mask is not None:
        B, C, spatial = init_image.shape[0], init_image.shape[1], tuple(init_image.shape[2:])
        if not isinstance(mask, Tensor) or tuple(mask.shape) not in ((B, 1) + spatial, (B, C) + spatial):
            got = tuple(mask.shape) if isinstance(mask, Tensor) else type(mask).__name__
            raise ValueError(f"mask must have shape {(B, 1) + spatial} or {(B, C) + spatial}, got {got}")
        if mask.dtype != torch.bool:
            if not mask.dtype.is_floating_point:
                raise ValueError(f"mask must be bool or floating point, got {mask.dtype}")
            lo, hi = torch.aminmax(mask.detach().float())
            if not (float(lo) >= 0.0 and float(hi) <= 1.0):  # (a NaN fails both comparisons)
                raise ValueError(f"mask values must lie in [0, 1], got min {float(lo)}, max {float(hi)}")
    return True


GUIDANCE_DEFAULTS = dict(guidance_rescale=0.0, guidance_interval=None, dynamic_threshold=None, threshold_max=None)


def _number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and v == v


def check_guidance(guidance_scale: float, guidance_rescale: float = 0.0, guidance_interval=None, dynamic_threshold=None,
                   threshold_max=None, flow: bool = False) -> bool:
    """validate the guided-sampling arguments of `Diffuser.generate` / `Diffusion.denoise`: guidance_rescale (phi of CFG rescale, Lin et
    al. 2023) in [0, 1]; guidance_interval (lo, hi) with 0 <= lo <= hi <= 1 (Kynkaanniemi et al. 2024); dynamic_threshold p in (0, 1]
    (Saharia et al. 2022); threshold_max >= 1, the cap on the threshold.  Host checks only.  -> False when all four are at their
    defaults (the plain sampling path), else True; a ValueError names the offending argument."""
    if not _number(guidance_rescale) or not 0.0 <= guidance_rescale <= 1.0:
        raise ValueError(f"guidance_rescale must be a number in [0, 1], got {guidance_rescale!r}")
    if guidance_interval is not None:
        ok = isinstance(guidance_interval, (tuple, list)) and len(guidance_interval) == 2 and all(_number(v) for v in guidance_interval)
        if not ok or not 0.0 <= guidance_interval[0] <= guidance_interval[1] <= 1.0:
            raise ValueError(f"guidance_interval must be (lo, hi) with 0 <= lo <= hi <= 1, got {guidance_interval!r}")
    if dynamic_threshold is not None and (not _number(dynamic_threshold) or not 0.0 < dynamic_threshold <= 1.0):
        raise ValueError(f"dynamic_threshold must be a number in (0, 1], got {dynamic_threshold!r}")
    if threshold_max is not None:
        if not _number(threshold_max) or not threshold_max >= 1.0:
            raise ValueError(f"threshold_max must be a number >= 1, got {threshold_max!r}")
        if dynamic_threshold is None:
            raise ValueError("threshold_max needs dynamic_threshold: it caps the threshold that one computes")
    if not guidance_scale > 0:
        if guidance_rescale > 0:
            raise ValueError(f"guidance_rescale={guidance_rescale} needs guidance_scale > 0: it rescales the guided prediction")
        if guidance_interval is not None:
            raise ValueError(f"guidance_interval={guidance_interval!r} needs guidance_scale > 0: it limits where guidance is applied")
    if flow and dynamic_threshold is not None:
        raise ValueError("dynamic_threshold is not available for flow samplers: the flow step has no per-step x0 clamp to replace "
                         "(use a Gaussian-diffusion sampler, ddpm or ddim)")
    return guidance_rescale > 0 or guidance_interval is not None or dynamic_threshold is not None


def guidance_kwargs(guidance_rescale: float = 0.0, guidance_interval=None, dynamic_threshold=None, threshold_max=None) -> dict:
    """the guided-sampling arguments that are not at their default, as keywords to pass on: a call with all four at their defaults
    passes nothing and stays what it was"""
    given = dict(guidance_rescale=guidance_rescale, guidance_interval=guidance_interval, dynamic_threshold=dynamic_threshold,
                 threshold_max=threshold_max)
    return {k: v for k, v in given.items() if v is not None and v != GUIDANCE_DEFAULTS[k]}


def in_guidance_interval(guidance_interval, level: float) -> bool:
    """is a step at noise level `level` (flow: t_curr; Gaussian diffusion: (training index + 1) / training steps) guided?  Both ends
    are inclusive; None guides every step"""
    return guidance_interval is None or guidance_interval[0] <= level <= guidance_interval[1]


def quantile_position(p: float, n: int) -> tuple[int, float]:
    """torch.quantile's `linear` position of the p-quantile among n sorted values, split for the kernels: pos = p (n - 1) in double,
    k = floor(pos), f = float32(pos - k); the quantile is v[k] + f (v[min(k + 1, n - 1)] - v[k]).  Where the fraction rounds up to 1
    in float32 the position moves to k + 1 with f = 0, which is the same value."""
    pos = float(p) * (n - 1)
    k = min(int(math.floor(pos)), n - 1)
    f = float(torch.tensor(pos - k, dtype=torch.float64).float())
    if f >= 1.0:
        k, f = min(k + 1, n - 1), 0.0
    return k, f


class _PinnedRing:
    """pinned staging slots for small host -> device transfers (per-step timestep vectors): a pageable `.to(device)` blocks the host
    until the stream has drained everything queued before it, i.e. once per training step the host loses its whole lead over the GPU
    -- and a step of short kernels (the UNet: 800 launches of 10-90 us) then runs its forward at the host's launch rate.  A slot is
    reused only after the copy that last read it has completed (an event per slot), so the host may run several steps ahead."""

    SLOTS = 8
    CAP_BYTES = 512 << 20  # pinned host memory the ring may hold; least-recently-used size classes are dropped beyond it

    def __init__(self) -> None:
        import collections
        import threading

        # size class (bytes rounded up to a power of two, device) -> [next slot, [(pinned byte buffer, event)], [used]]: multi-aspect-
        # ratio buckets and short last batches share a class instead of pinning a ring per shape
        self.slots: "collections.OrderedDict[tuple, list]" = collections.OrderedDict()
        self.bytes = 0
        self.lock = threading.Lock()  # (a prefetch thread and the training loop may both stage transfers)

    def put(self, t: Tensor, device: torch.device, dtype: torch.dtype) -> Tensor:
        nbytes = t.numel() * torch.empty((), dtype=dtype).element_size()
        cls = 1 << max(6, (nbytes - 1).bit_length())
        key = (cls, device)
        with self.lock:
            ring = self.slots.get(key)
            if ring is None:
                n = self.SLOTS if cls <= (1 << 18) else 3  # (batch-sized tensors: three slots are enough)
                while self.slots and self.bytes + n * cls > self.CAP_BYTES:
                    _, old = self.slots.popitem(last=False)
                    for (buf, ev), used in zip(old[1], old[2]):
                        if used:
                            ev.synchronize()  # (its last copy must have read the buffer before the memory is unpinned)
                        self.bytes -= buf.numel()
                ring = self.slots[key] = [0, [(torch.empty(cls, dtype=torch.uint8).pin_memory(), torch.cuda.Event()) for _ in range(n)], [False] * n]
                self.bytes += n * cls
            else:
                self.slots.move_to_end(key)
            i = ring[0]
            raw, ev = ring[1][i]
            if ring[2][i]:
                ev.synchronize()  # (eight transfers ago: completed long since unless the host is that far ahead)
            buf = raw[:nbytes].view(dtype).view(t.shape)
            buf.copy_(t)  # host-side conversion + copy into the pinned slot
            out = buf.to(device, non_blocking=True)
            ev.record(torch.cuda.current_stream(device))
            ring[2][i] = True
            ring[0] = (i + 1) % len(ring[1])
        return out


_RING = _PinnedRing()


def to_device(t: Tensor, device: torch.device | str, dtype: torch.dtype) -> Tensor:
    """`t.to(device=device, dtype=dtype).contiguous()` without the host-side synchronisation of a pageable copy (small CPU tensors go
    through a ring of pinned slots -- timestep vectors, batches of up to 32 MB --, everything else is the plain call): same values,
    same dtype conversion"""
    device = torch.device(device)
    if t.device.type == "cpu" and device.type == "cuda" and t.numel() * t.element_size() <= (32 << 20) and not t.requires_grad and t.numel() > 0:
        return _RING.put(t.detach(), device, dtype)
    return t.to(device=device, dtype=dtype).contiguous()

