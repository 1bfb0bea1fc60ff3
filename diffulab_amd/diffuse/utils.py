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

