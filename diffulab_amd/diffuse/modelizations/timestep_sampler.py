"""Loss-aware timestep sampling for Gaussian diffusion: the state of the loss-second-moment resampler of Nichol & Dhariwal,
"Improved Denoising Diffusion Probabilistic Models" (2021), sec. 3.3 (`LossSecondMomentResampler` of their code base), kept on the
device.  The reference draws timesteps uniformly and has none of this.

The state is five small device tensors: the last `history` per-sample losses of every chain index, how many of them are filled, and
the tables formed from them -- the sampling distribution p, the importance weights 1 / (T p) and the cumulative distribution the
draw searches.  `dl_loss_history_update` advances all of them in one launch and `dl_draw_timesteps` draws from them; no value of the
state is read back to the host by either, nor by `compute_loss`.
"""

from __future__ import annotations

from typing import Any

import torch
from torch import Tensor

from ... import ops

TIMESTEP_SAMPLERS = ("uniform", "loss_second_moment")
MAX_STEPS = 4096  # dl_loss_history_update keeps the whole distribution in one workgroup's shared memory


def gather_pairs(t: Tensor, total: Tensor) -> tuple[Tensor, Tensor]:
    """the (t, loss) pairs of all data-parallel ranks, concatenated in rank order, so that every rank applies the same pairs in the
    same order and holds the same history (IDDPM's `update_with_local_losses`; every rank brings the same batch size).  Without an
    initialised process group of more than one rank: the arguments themselves."""
    dist = torch.distributed
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return t, total
    world = dist.get_world_size()
    ts = [torch.empty_like(t) for _ in range(world)]
    ls = [torch.empty_like(total) for _ in range(world)]
    dist.all_gather(ts, t.contiguous())
    dist.all_gather(ls, total.contiguous())
    return torch.cat(ts), torch.cat(ls)


class LossSecondMomentState:
    """history f32 [T, H], counts int32 [T], p / imp / cdf f32 [T] on one device (created on the first use that names one).  Before
    every index has `history` losses p is uniform, exactly as IDDPM warms up."""

    KEYS = ("history", "counts", "p", "imp", "cdf")

    def __init__(self, n_steps: int, history: int = 10, uniform_prob: float = 0.001) -> None:
        if n_steps > MAX_STEPS:
            raise ValueError(f'timestep_sampler="loss_second_moment" keeps chains of up to {MAX_STEPS} steps, got {n_steps}')
        self.n_steps, self.history_per_term, self.uniform_prob = int(n_steps), int(history), float(uniform_prob)
        self.device: torch.device | None = None
        self.tensors: dict[str, Tensor] = {}

    def reset(self, n_steps: int | None = None) -> None:
        if n_steps is not None:
            if n_steps > MAX_STEPS:
                raise ValueError(f'timestep_sampler="loss_second_moment" keeps chains of up to {MAX_STEPS} steps, got {n_steps}')
            self.n_steps = int(n_steps)
        self.device, self.tensors = None, {}

    def on(self, device: torch.device | str) -> dict[str, Tensor]:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.device is None:
            T, H = self.n_steps, self.history_per_term
            cdf = (torch.arange(1, T + 1, dtype=torch.float64) / T).float()
            cdf[-1] = 1.0
            host = {"history": torch.zeros(T, H), "counts": torch.zeros(T, dtype=torch.int32),
                    "p": torch.full((T,), 1.0 / T, dtype=torch.float64).float(), "imp": torch.ones(T), "cdf": cdf}
            self.tensors = {k: v.to(device).contiguous() for k, v in host.items()}
            self.device = device
        elif device != self.device:  # (a host copy of a few KB, outside the training step)
            self.tensors = {k: v.to(device).contiguous() for k, v in self.tensors.items()}
            self.device = device
        return self.tensors

    def update(self, t: Tensor, total: Tensor) -> None:
        """one training step's pairs (device int32 [n], f32 [n]; all ranks' under data parallel), one launch"""
        s = self.on(t.device)
        t, total = gather_pairs(t, total)
        ops.loss_history_update(t, total, s["history"], s["counts"], s["p"], s["imp"], s["cdf"], self.uniform_prob)

    def draw(self, u: Tensor) -> Tensor:
        """u f32 [B] on the device, uniform in [0, 1) -> int32 [B] drawn from p"""
        return ops.draw_timesteps(u, self.on(u.device)["cdf"])

    def state_dict(self) -> dict[str, Any]:
        out: dict[str, Any] = {"n_steps": self.n_steps, "history_per_term": self.history_per_term, "uniform_prob": self.uniform_prob}
        out.update({k: v.detach().clone() for k, v in self.tensors.items()})
        return out

    def load_state_dict(self, state: dict[str, Any]) -> None:
        T, H = int(state["n_steps"]), int(state["history_per_term"])
        if T != self.n_steps:
            raise ValueError(f"the state is that of a {T}-step chain; this one has {self.n_steps} steps")
        given = [k for k in self.KEYS if k in state]
        if given and len(given) != len(self.KEYS):
            raise ValueError(f"the state holds {given}; all of {list(self.KEYS)} or none are expected")
        for k in given:
            want = (T, H) if k == "history" else (T,)
            if tuple(state[k].shape) != want:
                raise ValueError(f"state[{k!r}] has shape {tuple(state[k].shape)}, expected {want}")
        self.history_per_term, self.uniform_prob = H, float(state["uniform_prob"])
        device = self.device
        self.device, self.tensors = None, {}
        if given:
            self.tensors = {k: state[k].detach().to(dtype=torch.int32 if k == "counts" else torch.float32).clone().contiguous()
                            for k in self.KEYS}
            self.device = self.tensors["p"].device
            if device is not None:
                self.on(device)
