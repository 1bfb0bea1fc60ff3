"""Exponential moving average of the denoiser, one fused launch over the flat parameter arena.

Replaces ``ema_pytorch.EMA`` (third-party, pinned 0.7.7 in the reference's uv.lock, not vendored under /root/reference) as the
reference uses it in base_trainer.py:247-256 (``EMA(denoiser, beta, update_after_step, update_every)``, ``.update()``,
``.ema_model``).  Published update rule restated (ema_pytorch/ema_pytorch.py, ``update`` / ``get_current_decay`` /
``update_moving_average`` with its defaults inv_gamma=1, power=2/3, min_value=0):

    step = self.step ; self.step += 1
    if step % update_every: return
    if step <= update_after_step: ema <- model ; return            (plain copy)
    if not initted: ema <- model ; initted = True
    epoch = max(step - update_after_step - 1, 0)
    decay = 0 if epoch <= 0 else clamp(1 - (1 + epoch / inv_gamma) ** -power, min_value, beta)
    ema <- ema + (1 - decay) * (model - ema)                        (Tensor.lerp_)

``ema_model`` is a deep copy of the denoiser (its own flat arena), so the lerp over ALL parameters is one ``dl_ema_update``
launch instead of one ATen kernel per tensor.
"""

from __future__ import annotations

import copy
import json
import os

import torch

from .. import ops
from ..engine import bump_param_epoch
from . import posthoc_ema


class EMA(torch.nn.Module):
    def __init__(self, model: torch.nn.Module, beta: float = 0.9999, update_after_step: int = 100, update_every: int = 10,
                 inv_gamma: float = 1.0, power: float = 2 / 3, min_value: float = 0.0) -> None:
        super().__init__()
        self.beta, self.update_after_step, self.update_every = beta, update_after_step, update_every
        self.inv_gamma, self.power, self.min_value = inv_gamma, power, min_value
        object.__setattr__(self, "online_model", model)  # not registered: the online model is not part of the EMA state
        self.ema_model = copy.deepcopy(model)
        self.ema_model.requires_grad_(False)
        self.step = 0
        self.initted = False

    @property
    def model(self) -> torch.nn.Module:
        return self.online_model

    def get_current_decay(self) -> float:
        epoch = max(self.step - self.update_after_step - 1, 0)
        if epoch <= 0:
            return 0.0
        value = 1 - (1 + epoch / self.inv_gamma) ** -self.power
        return min(max(value, self.min_value), self.beta)

    def _arenas(self):
        src, dst = self.online_model, self.ema_model
        if hasattr(src, "engine") and hasattr(dst, "engine"):
            src.engine, dst.engine  # noqa: B018 -- (re)flatten both if needed
            if src._flat is not None and dst._flat is not None and src._flat.numel() == dst._flat.numel():
                return src._flat, dst._flat
        return None

    @torch.no_grad()
    def _lerp(self, weight: float) -> None:
        """ema <- ema + weight * (model - ema); weight = 1 is the plain copy"""
        flat = self._arenas()
        if flat is not None:
            ops.ema_update(flat[1], flat[0], 1.0 - weight)
        else:
            for pe, pm in zip(self.ema_model.parameters(), self.online_model.parameters()):
                ops.ema_update(pe.data, pm.data, 1.0 - weight)
        bump_param_epoch()

    def copy_params_from_model_to_ema(self) -> None:
        self._lerp(1.0)

    def update(self) -> None:
        step = self.step
        self.step += 1
        if step % self.update_every != 0:
            return
        if step <= self.update_after_step:
            self.copy_params_from_model_to_ema()
            return
        if not self.initted:
            self.copy_params_from_model_to_ema()
            self.initted = True
        self._lerp(1.0 - self.get_current_decay())  # reads the already incremented step counter, like ema_pytorch

    def forward(self, *args, **kwargs):
        return self.ema_model(*args, **kwargs)


class PowerEMA(torch.nn.Module):
    """Power-function EMA profiles for post-hoc EMA (training/posthoc_ema.py; this project's, the reference has none).

    One deep copy of the denoiser per tracked ``sigma_rel`` (``ema_models``, each with its own flat arena).  ``update()`` counts calls;
    every ``update_every``-th call is update number t = 1, 2, ...: ema_k <- ema_k + w_k (model - ema_k) with
    w_k = posthoc_ema.ema_weight(t, gamma_k), all profiles in ONE ``dl_ema_update_multi`` launch that reads the online arena once.
    t = 1 has w = 1: the first update is a copy, there is no warm-up.  ``ema_model`` (what validation and ``forward`` use) is the
    profile of ``eval_sigma_rel`` (default: the first).  ``snapshot(dir)`` writes every profile as a checkpoint with the denoiser's own
    key names plus one index line each; ``posthoc_ema.synthesize`` combines them afterwards."""

    MAX_PROFILES = ops.EMA_MAX_PROFILES

    @staticmethod
    def check_arguments(sigma_rels, eval_sigma_rel) -> tuple[tuple[float, ...], float]:
        """-> (sigma_rels as floats, the evaluation profile's sigma_rel); a ValueError names the argument at fault"""
        sigma_rels = tuple(float(s) for s in sigma_rels)
        if not 1 <= len(sigma_rels) <= PowerEMA.MAX_PROFILES:
            raise ValueError(f"sigma_rels: 1 to {PowerEMA.MAX_PROFILES} profiles can be tracked, got {len(sigma_rels)}")
        if len({f"{s:.3f}" for s in sigma_rels}) != len(sigma_rels):
            raise ValueError(f"sigma_rels: duplicate sigma_rel in {sigma_rels!r} (snapshots are told apart to 3 decimals)")
        for s in sigma_rels:
            if not 0.0 < s < posthoc_ema.SIGMA_REL_MAX:
                raise ValueError(f"sigma_rels: every sigma_rel must lie in (0, {posthoc_ema.SIGMA_REL_MAX}), got {s!r}")
        if eval_sigma_rel is None:
            eval_sigma_rel = sigma_rels[0]
        if float(eval_sigma_rel) not in sigma_rels:
            raise ValueError(f"eval_sigma_rel = {eval_sigma_rel!r} is not one of the tracked sigma_rels {sigma_rels!r}")
        return sigma_rels, float(eval_sigma_rel)

    def __init__(self, model: torch.nn.Module, sigma_rels=(0.05, 0.10), update_every: int = 1, eval_sigma_rel: float | None = None) -> None:
        super().__init__()
        sigma_rels, eval_sigma_rel = self.check_arguments(sigma_rels, eval_sigma_rel)
        if int(update_every) < 1:
            raise ValueError(f"update_every must be >= 1, got {update_every!r}")
        self.sigma_rels, self.update_every = sigma_rels, int(update_every)
        self.eval_sigma_rel = eval_sigma_rel
        self.gammas = tuple(posthoc_ema.sigma_rel_to_gamma(s) for s in sigma_rels)
        object.__setattr__(self, "online_model", model)  # not registered: the online model is not part of the EMA state
        self.ema_models = torch.nn.ModuleList(copy.deepcopy(model) for _ in sigma_rels)
        self.ema_models.requires_grad_(False)
        self.t = 0      # profile updates made
        self.calls = 0  # update() calls seen

    @property
    def model(self) -> torch.nn.Module:
        return self.online_model

    @property
    def ema_model(self) -> torch.nn.Module:
        return self.ema_models[self.sigma_rels.index(self.eval_sigma_rel)]

    def weights(self, t: int) -> list[float]:
        return [posthoc_ema.ema_weight(t, g) for g in self.gammas]

    def _arenas(self):
        src = self.online_model
        if not hasattr(src, "engine") or not all(hasattr(m, "engine") for m in self.ema_models):
            return None
        src.engine  # noqa: B018 -- (re)flatten if needed
        for m in self.ema_models:
            m.engine  # noqa: B018
        flats = [m._flat for m in self.ema_models]
        if src._flat is None or any(f is None or f.numel() != src._flat.numel() for f in flats):
            return None
        return src._flat, flats

    @torch.no_grad()
    def _lerp(self, weights: list[float]) -> None:
        flat = self._arenas()
        if flat is not None:
            ops.ema_update_multi(flat[1], flat[0], weights)
        else:
            for pm, *pes in zip(self.online_model.parameters(), *(m.parameters() for m in self.ema_models)):
                ops.ema_update_multi([pe.data for pe in pes], pm.data, weights)
        bump_param_epoch()

    def update(self) -> None:
        calls = self.calls
        self.calls += 1
        if calls % self.update_every != 0:
            return
        self.t += 1
        self._lerp(self.weights(self.t))

    def forward(self, *args, **kwargs):
        return self.ema_model(*args, **kwargs)

    # ---- state: t, the call counter, the tracked widths and every profile's weights
    def state_dict(self, *args, **kwargs):
        return {"t": self.t, "calls": self.calls, "sigma_rels": list(self.sigma_rels), "eval_sigma_rel": self.eval_sigma_rel,
                "profiles": [m.state_dict() for m in self.ema_models]}

    def load_state_dict(self, state, strict: bool = True, assign: bool = False):
        got = tuple(float(s) for s in state["sigma_rels"])
        if got != self.sigma_rels:
            raise ValueError(f"sigma_rels: the state tracks {got!r}, this PowerEMA {self.sigma_rels!r}")
        for m, sd in zip(self.ema_models, state["profiles"]):
            m.load_state_dict(sd, strict=strict)
        self.t, self.calls = int(state["t"]), int(state["calls"])
        bump_param_epoch()

    def snapshot(self, directory) -> list[str]:
        """every profile's `state_dict()` as phema_{t:09d}_{sigma_rel:.3f}.pt (the denoiser's own keys: loads wherever ema.pt does)
        and one line {"t", "sigma_rel", "file"} each appended to phema_index.jsonl; -> the file names"""
        if self.t < 1:
            raise ValueError("snapshot: no profile update has been made yet (t = 0)")
        os.makedirs(directory, exist_ok=True)
        names = []
        for s, m in zip(self.sigma_rels, self.ema_models):
            name = posthoc_ema.snapshot_name(self.t, s)
            torch.save({k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in m.state_dict().items()},
                       os.path.join(directory, name))
            names.append(name)
        with open(os.path.join(directory, posthoc_ema.INDEX_NAME), "a") as f:
            for s, name in zip(self.sigma_rels, names):
                f.write(json.dumps({"t": self.t, "sigma_rel": s, "file": name}) + "\n")
        return names
