"""Fused AdamW over the flat parameter arena: ONE `dl_adamw_step` launch per optimizer step (with ``max_grad_norm``: one sum of
squares over the gradient arena and a one-workgroup fold in front of it, then `dl_adamw_step_clip`).

Drop-in `torch.optim.Optimizer` (same hyper-parameters / update rule as `torch.optim.AdamW`, which
`configs/optimizer/adamw.yaml` of the reference instantiates).  When the parameters are views of one flat f32
arena (what `MMDiT.flatten_parameters` sets up) the whole model is updated by a single kernel; otherwise it
launches the same HIP kernel once per tensor.

`FusedSGD` is the same for `torch.optim.SGD` (`configs/optimizer/sgd.yaml`): ONE `dl_sgd_step` launch.  `FusedMuon` is
`torch.optim.Muon` (`configs/optimizer/muon.yaml`) on the hidden matrices and AdamW on the rest: 19 launches, whatever the number of
matrices.  All derive from `FusedArenaOptimizer`, which owns what is not the update rule: finding the arena, `zero_grad` as one memset, the clipping pass,
`grad_scale` and the device scalars of a captured step.
"""

from __future__ import annotations

import torch
from torch import Tensor

from .. import ops
from ..engine import bump_param_epoch


def _arena_of(params: list[Tensor], use_grad: bool) -> Tensor | None:
    """flat f32 tensor spanning the storage all `params` (or their grads) are views of, else None.
    (`p.data` is not a view object, so `_base` cannot be used: compare the underlying storages.)"""
    store = None
    for p in params:
        t = p.grad if use_grad else p.data
        if t is None or t.dtype != torch.float32 or not t.is_contiguous():
            return None
        s = t.untyped_storage()
        if store is None:
            store = s
        elif s.data_ptr() != store.data_ptr():
            return None
    if store is None:
        return None
    t0 = params[0].grad if use_grad else params[0].data
    return torch.empty(0, dtype=torch.float32, device=t0.device).set_(store, 0, (store.nbytes() // 4,))


class FusedArenaOptimizer(torch.optim.Optimizer):
    """What the fused optimizers share; a subclass adds the update rule (``step``), its state and ``_graph_scalars``.

    ``max_grad_norm``: clip by the global 2-norm of all gradients of all parameter groups (``torch.nn.utils.clip_grad_norm_``'s
    rule: every gradient times ``min(1, max_grad_norm / (norm + 1e-6))``, the norm being that of ``grad_scale * grad``) INSIDE the
    update: ``step()`` reads the gradients once more for the sum of squares, leaves ``{norm, coef}`` in device memory and hands the
    update kernels the coefficient's address.  ``p.grad`` is left UNSCALED -- the fused path never rewrites the gradient arena --
    and nothing synchronises with the host; ``last_grad_norm`` is the norm of the latest step as a 0-d device tensor (a view of the
    optimizer's own scalar: clone it to keep a value across steps).  ``None`` (the default): exactly the launches of the plain
    update."""

    def __init__(self, params, defaults: dict, max_grad_norm: float | None = None) -> None:
        super().__init__(params, defaults)
        self.grad_scale = 1.0  # data parallel: 1/world (gradients are SUM-reduced), folded into the update kernel
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm: Tensor | None = None
        # sum-of-squares slots and the {norm, coef} pair: allocated ONCE (captured graphs hold their addresses, like _graph_buffers)
        self._clip_partials: Tensor | None = None
        self._clip_out: Tensor | None = None
        self._graph_hyper: list[tuple[Tensor, Tensor]] | None = None  # per group: (device f32[8], pinned host mirror)
        self._graph_buffers: list[tuple[Tensor, Tensor]] | None = None

    # ---- hipGraph support (dl_adamw_step_dev / dl_sgd_step_dev; the captured-step experiment lives in scripts/lab/graph_step.py):
    #      inside a captured step the update kernels read their scalars from a device buffer; the host advances the step count and
    #      refreshes that buffer BEFORE each replay.  The buffers are allocated ONCE: graphs captured earlier hold their addresses,
    #      so a second begin_graph_mode (another input shape being captured) must not replace them.
    def begin_graph_mode(self) -> None:
        if self._graph_hyper is None:
            if self._graph_buffers is None:
                dev = next(p for g in self.param_groups for p in g["params"]).device
                self._graph_buffers = [(torch.zeros(8, device=dev), torch.zeros(8).pin_memory()) for _ in self.param_groups]
            self._graph_hyper = self._graph_buffers
        self._graph_step = max([int(st["step"]) for st in self.state.values() if "step" in st] or [0])

    def in_graph_mode(self) -> bool:
        return self._graph_hyper is not None

    def end_graph_mode(self) -> None:
        self._graph_hyper = None  # (the buffers stay allocated: a graph that is still alive keeps reading them)

    def advance(self) -> None:
        """one optimizer step is about to be replayed: bump the step count everywhere and upload the hyper-parameters"""
        assert self._graph_hyper is not None
        self._graph_step += 1
        for st in self.state.values():
            if "step" in st:
                st["step"] = self._graph_step
        for group, (dev, host) in zip(self.param_groups, self._graph_hyper):
            host.copy_(torch.tensor(self._graph_scalars(group, self._graph_step), dtype=torch.float32))
            dev.copy_(host, non_blocking=True)
        bump_param_epoch()

    def _graph_scalars(self, group: dict, step: int) -> list[float]:
        """the eight f32 the update kernel of a captured step reads from device memory; [7] is grad_scale (dl_clip_coef reads it)"""
        raise NotImplementedError

    @staticmethod
    def _arena_key(group, rest: list) -> Tensor:
        skip = {id(p) for p in rest}
        return next(p for p in group["params"] if id(p) not in skip and p.requires_grad)

    def _flat(self, group) -> tuple[Tensor, Tensor, list] | None:
        """`_flat_scan(group)`, remembered per group: a hit is re-validated by pointer compares only (every arena parameter's data and
        gradient still sit at the recorded addresses, the group's parameter list is the same objects) -- the full scan costs 1.7 ms
        on the UNet's ~500 tensors and ran twice per training step (zero_grad, step)"""
        cache = self.__dict__.setdefault("_flat_cache", {})
        hit = cache.get(id(group))
        if hit is not None:
            plist, n, pins, res = hit
            if plist is group["params"] and len(plist) == n:
                for p, dp, gp in pins:
                    g = p.grad
                    if g is None or g.data_ptr() != gp or p.data_ptr() != dp or not p.requires_grad:
                        break
                else:
                    if all(p.grad is None or not p.requires_grad or id(p) in res[3] for p in res[2]):  # (nobody outside joined the arena)
                        return res[:3]
        res = self._flat_scan(group)
        if res is None:
            cache.pop(id(group), None)
            return None
        ids = {id(p) for p in group["params"]} - {id(p) for p in res[2]}
        inside = [p for p in group["params"] if id(p) in ids]
        # (outside tensors are re-scanned when one of them gains a gradient: it might be an arena view that had none yet)
        outside_with_grad = {id(p) for p in res[2] if p.grad is not None and p.requires_grad}
        cache[id(group)] = (group["params"], len(group["params"]), [(p, p.data_ptr(), p.grad.data_ptr()) for p in inside],
                            (res[0], res[1], res[2], outside_with_grad))
        return res

    def _flat_scan(self, group) -> tuple[Tensor, Tensor, list] | None:
        """(param arena, grad arena, parameters NOT in it) when (most of) the group lives in one flat arena -- e.g. a denoiser's
        arena plus the few tensors of an auxiliary loss head (REPA projector) in the same param group -- else None"""
        ps = [p for p in group["params"] if p.requires_grad]
        by_store: dict[int, list] = {}
        for p in ps:
            if p.grad is None or p.data.dtype != torch.float32:
                continue
            by_store.setdefault(p.data.untyped_storage().data_ptr(), []).append(p)
        if not by_store:
            return None
        inside = max(by_store.values(), key=lambda v: sum(q.numel() for q in v))
        pb, gb = _arena_of(inside, False), _arena_of(inside, True)
        if pb is None or gb is None or pb.numel() != gb.numel():
            return None
        if any(p.data.storage_offset() != p.grad.storage_offset() for p in inside):
            return None
        if sum(p.numel() for p in inside) < 0.9 * pb.numel():  # the group must own (almost) the whole arena
            return None
        ids = {id(p) for p in inside}
        return pb, gb, [p for p in group["params"] if id(p) not in ids]

    def zero_grad(self, set_to_none: bool = True) -> None:
        for group in self.param_groups:
            flat = self._flat(group)
            rest = group["params"]
            if flat is not None:
                flat[1].zero_()  # one memset; .grad views stay attached
                rest = flat[2]
            for p in rest:
                if p.grad is not None:
                    if set_to_none:
                        p.grad = None
                    else:
                        p.grad.zero_()

    def _clip_pass(self) -> Tensor:
        """sum of squares over every group's gradient arena and loose gradients (ONE global norm, as torch's function takes it over a
        parameter list), then the fold: -> the device coefficient the update launches of this step take"""
        bufs: list[Tensor] = []
        for group in self.param_groups:
            flat = self._flat(group)
            rest = group["params"]
            if flat is not None:
                bufs.append(flat[1])
                rest = flat[2]
            bufs.extend(p.grad for p in rest if p.grad is not None)
        if not bufs:
            raise RuntimeError("max_grad_norm is set but no parameter has a gradient")
        need = sum(ops.grad_sumsq_slots(b.numel()) for b in bufs)
        if self._clip_partials is None or need > self._clip_partials.numel():
            if self._clip_partials is not None and self._graph_buffers is not None:
                raise RuntimeError("the gradient buffers grew after a graph was captured: captured graphs hold the partials' address")
            self._clip_partials = torch.zeros(max(need, 1024), device=bufs[0].device)
        if self._clip_out is None:
            self._clip_out = torch.zeros(2, device=bufs[0].device)
            self.last_grad_norm = self._clip_out[0]
        slot = 0
        for b in bufs:
            slot += ops.grad_sumsq(b, self._clip_partials, slot)
        hyper = self._graph_hyper[0][0] if self._graph_hyper is not None else None  # (grad_scale is one value for every group)
        ops.clip_coef(self._clip_partials, slot, self.max_grad_norm, self._clip_out, self.grad_scale, hyper)
        return self._clip_out[1:2]


class FusedAdamW(FusedArenaOptimizer):
    """``torch.optim.AdamW``'s update in one launch per arena; ``max_grad_norm`` as in `FusedArenaOptimizer`."""

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: float | None = None) -> None:
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), max_grad_norm)
        self._legacy_arena_states: list[dict] = []

    def _graph_scalars(self, group: dict, step: int) -> list[float]:
        b1, b2 = group["betas"]
        bc1, bc2 = 1.0 - b1**step, 1.0 - b2**step
        return [group["lr"], b1, b2, group["eps"], group["weight_decay"], group["lr"] / bc1, bc2**-0.5, self.grad_scale]

    def load_state_dict(self, state_dict) -> None:
        """accepts three optimizer.pt layouts: this class's own (arena-sized ``m`` / ``v`` / ``step`` under the first arena
        parameter of a group, per-parameter ``m`` / ``v`` / ``step`` for tensors outside the arena), the reference's
        ``torch.optim.AdamW`` checkpoint (per-parameter ``exp_avg`` / ``exp_avg_sq`` / ``step``: packed into the arena moments at
        the first step, see _adopt_reference_state) and the address-keyed ``arena*`` entries round 1 wrote (matched by size)"""
        super().load_state_dict(state_dict)
        for k in [k for k in self.state if isinstance(k, str) and k.startswith("arena")]:
            self._legacy_arena_states.append(self.state.pop(k))

    def _adopt_reference_state(self, pb: Tensor, inside: list, key: Tensor) -> None:
        """torch.optim.AdamW state (the reference's optimizer.pt, base_trainer.py:246-251) -> arena moments: every arena
        parameter's exp_avg / exp_avg_sq is copied to its offset, the step count is the parameters' common one"""
        m, v = torch.zeros_like(pb), torch.zeros_like(pb)
        steps = set()
        base = pb.storage_offset()
        for p in inside:
            st = self.state.get(p)
            if not st:
                continue
            if "exp_avg" not in st or "exp_avg_sq" not in st:
                raise RuntimeError(f"optimizer state of an arena parameter has keys {sorted(st)}: expected FusedAdamW's "
                                   "('m', 'v', 'step') or torch.optim.AdamW's ('exp_avg', 'exp_avg_sq', 'step')")
            o = p.data.storage_offset() - base
            m[o : o + p.numel()].copy_(st["exp_avg"].reshape(-1).to(pb.device, torch.float32))
            v[o : o + p.numel()].copy_(st["exp_avg_sq"].reshape(-1).to(pb.device, torch.float32))
            steps.add(int(st["step"]))
            if p is not key:
                del self.state[p]
        if len(steps) > 1:
            raise RuntimeError(f"torch.optim.AdamW checkpoint with different step counts per parameter ({sorted(steps)}): the arena "
                               "update has one")
        st = self.state[key]
        st.clear()
        st["step"], st["m"], st["v"] = (steps.pop() if steps else 0), m, v

    @staticmethod
    def _adopt_reference_param_state(st: dict, p: Tensor) -> None:
        """a parameter OUTSIDE the arena (REPA projector / resampler tensors that share the denoiser's param group,
        examples/train_repa.py) resumed from a torch.optim.AdamW checkpoint: rename exp_avg / exp_avg_sq to this class's m / v"""
        if "m" not in st and "exp_avg" in st and "exp_avg_sq" in st:
            st["m"] = st.pop("exp_avg").to(device=p.device, dtype=torch.float32).contiguous()
            st["v"] = st.pop("exp_avg_sq").to(device=p.device, dtype=torch.float32).contiguous()
            st.pop("max_exp_avg_sq", None)
            st["step"] = int(st.get("step", 0))

    def _update(self, p: Tensor, g: Tensor, st: dict, group: dict, coef: Tensor | None) -> None:
        b1, b2 = group["betas"]
        if coef is None:
            ops.adamw_step(p, g, st["m"], st["v"], group["lr"], b1, b2, group["eps"], group["weight_decay"], st["step"],
                           self.grad_scale)
        else:
            ops.adamw_step_clip(p, g, st["m"], st["v"], group["lr"], b1, b2, group["eps"], group["weight_decay"], st["step"],
                                coef, self.grad_scale)

    @staticmethod
    def _update_dev(p: Tensor, g: Tensor, st: dict, hyper: Tensor, coef: Tensor | None) -> None:
        if coef is None:
            ops.adamw_step_dev(p, g, st["m"], st["v"], hyper)
        else:
            ops.adamw_step_dev_clip(p, g, st["m"], st["v"], hyper, coef)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        coef = self._clip_pass() if self.max_grad_norm is not None else None
        for gi, group in enumerate(self.param_groups):
            if self._graph_hyper is not None:  # captured step: scalars come from the device buffer, state must already exist
                hyper = self._graph_hyper[gi][0]
                flat = self._flat(group)
                rest = group["params"]
                if flat is not None:
                    pb, gb, rest = flat
                    st = self.state[self._arena_key(group, rest)]
                    if "m" not in st:
                        raise RuntimeError("graph mode needs the arena moments: run one eager step() after loading a checkpoint")
                    self._update_dev(pb, gb, st, hyper, coef)
                for p in rest:
                    if p.grad is not None:
                        st = self.state[p]
                        self._adopt_reference_param_state(st, p)
                        self._update_dev(p.data, p.grad, st, hyper, coef)
                continue
            flat = self._flat(group)
            rest = group["params"]
            if flat is not None:
                pb, gb, rest = flat
                # The arena's moments are keyed on the group's first arena parameter: Optimizer.state_dict() maps parameter keys
                # to stable indices, so a checkpoint resumes in a new process (a key derived from the arena's address would not)
                key = self._arena_key(group, rest)
                st = self.state[key]
                if not st:
                    for i, old in enumerate(self._legacy_arena_states):  # address-keyed entries of round-1 checkpoints
                        if old["m"].numel() == pb.numel():
                            st.update(self._legacy_arena_states.pop(i))
                            break
                if st and "m" not in st:  # a torch.optim.AdamW checkpoint (per-parameter exp_avg / exp_avg_sq)
                    skip = {id(p) for p in rest}
                    self._adopt_reference_state(pb, [p for p in group["params"] if id(p) not in skip and p.requires_grad], key)
                if not st:
                    st["step"], st["m"], st["v"] = 0, torch.zeros_like(pb), torch.zeros_like(pb)
                if st["m"].device != pb.device or st["m"].numel() != pb.numel():  # state loaded before the model moved
                    assert st["m"].numel() == pb.numel(), "optimizer state does not match the parameter arena"
                    st["m"], st["v"] = st["m"].to(pb.device), st["v"].to(pb.device)
                st["step"] = int(st["step"]) + 1
                self._update(pb, gb, st, group, coef)
                bump_param_epoch()  # raw-pointer writes bump no torch version counter: tell the engines
            if rest:
                for p in rest:
                    if p.grad is None:
                        continue
                    st = self.state[p]
                    self._adopt_reference_param_state(st, p)
                    if not st:
                        st["step"], st["m"], st["v"] = 0, torch.zeros_like(p.data), torch.zeros_like(p.data)
                    if st["m"].device != p.device:
                        st["m"], st["v"] = st["m"].to(p.device), st["v"].to(p.device)
                    st["step"] = int(st["step"]) + 1
                    self._update(p.data, p.grad, st, group, coef)
            bump_param_epoch()
        return loss


class FusedSGD(FusedArenaOptimizer):
    """``torch.optim.SGD``'s update (``configs/optimizer/sgd.yaml``: momentum, dampening, weight decay, Nesterov, maximize) in ONE
    `dl_sgd_step` launch per arena and one per tensor outside it; ``max_grad_norm``, ``grad_scale`` and graph mode as in
    `FusedArenaOptimizer`.  State: one arena-sized ``buf`` plus ``step`` under the group's first arena parameter, ``buf`` / ``step``
    per tensor outside the arena, and no buffer at all with ``momentum == 0``.  As in torch, a tensor's first step with momentum
    copies the gradient into the buffer (no dampening).  ``foreach`` / ``fused`` / ``differentiable`` are accepted, as a config may
    pass them, and ignored."""

    def __init__(self, params, lr: float = 1e-3, momentum: float = 0, dampening: float = 0, weight_decay: float = 0,
                 nesterov: bool = False, maximize: bool = False, max_grad_norm: float | None = None, foreach=None, fused=None,
                 differentiable: bool = False) -> None:
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      maximize=maximize), max_grad_norm)

    def _graph_scalars(self, group: dict, step: int) -> list[float]:
        # ([5], [6] are unused; dl_sgd_step_dev reads grad_scale at [4], dl_clip_coef at [7])
        return [group["lr"], group["momentum"], group["dampening"], group["weight_decay"], self.grad_scale, 0.0, 0.0, self.grad_scale]

    def _adopt_reference_state(self, pb: Tensor, group: dict, inside: list, key: Tensor) -> None:
        """torch.optim.SGD state (the reference's optimizer.pt: per-parameter ``momentum_buffer``) -> the arena buffer: every arena
        parameter's buffer is copied to its offset.  Buffers that are all None (or no state at all): the first step.  Both kinds
        side by side cannot be one launch's state (torch would dampen the one and not the other): refused"""
        have = [p for p in inside if (self.state.get(p) or {}).get("momentum_buffer") is not None]
        if have and len(have) != len(inside):
            index = {id(p): i for i, p in enumerate(group["params"])}
            ids = {id(p) for p in have}
            without = [index[id(p)] for p in inside if id(p) not in ids]
            raise RuntimeError(f"torch.optim.SGD checkpoint: {len(have)} arena parameters have a 'momentum_buffer' and {len(without)} "
                               f"have none (positions {without[:8]}{' ...' if len(without) > 8 else ''} of the group; state keys "
                               f"{[sorted(self.state.get(group['params'][i]) or {}) for i in without[:8]]}): the arena update has one "
                               "buffer for all of them")
        buf = torch.zeros_like(pb) if have else None
        base = pb.storage_offset()
        for p in inside:
            st = self.state.get(p)
            if st is None:
                continue
            mb = st.pop("momentum_buffer", None)
            if mb is not None:
                o = p.data.storage_offset() - base
                buf[o : o + p.numel()].copy_(mb.reshape(-1).to(pb.device, torch.float32))
            if p is not key and not st:
                del self.state[p]
        if buf is not None:
            self.state[key]["buf"] = buf

    def _update(self, p: Tensor, g: Tensor, st: dict, group: dict, hyper: Tensor | None, coef: Tensor | None) -> None:
        mom = group["momentum"]
        buf = st.get("buf") if mom != 0 else None
        first = mom != 0 and buf is None
        if buf is not None and buf.numel() != p.numel():
            raise RuntimeError(f"optimizer state does not match its parameter: a momentum buffer of {buf.numel()} elements for "
                               f"{p.numel()} parameters")
        if hyper is not None:  # captured step: the scalars come from the device buffer, advance() counts the step
            if first:
                raise RuntimeError("graph mode needs the momentum buffer: run one eager step() first (also after loading a checkpoint)")
            ops.sgd_step_dev(p, g, buf, hyper, coef, group["nesterov"], group["maximize"])
            return
        if first:
            buf = st["buf"] = torch.empty_like(p)  # (written, not read, by the first step)
        elif buf is not None and buf.device != p.device:  # state loaded before the model moved
            buf = st["buf"] = buf.to(p.device)
        st["step"] = int(st.get("step", 0)) + 1
        ops.sgd_step(p, g, buf, group["lr"], mom, group["dampening"], group["weight_decay"], self.grad_scale, coef,
                     group["nesterov"], first, group["maximize"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        coef = self._clip_pass() if self.max_grad_norm is not None else None
        for gi, group in enumerate(self.param_groups):
            hyper = self._graph_hyper[gi][0] if self._graph_hyper is not None else None
            flat = self._flat(group)
            rest = group["params"]
            if flat is not None:
                pb, gb, rest = flat
                # (keyed on the group's first arena parameter, for the reason FusedAdamW.step gives)
                key = self._arena_key(group, rest)
                st = self.state[key]
                if group["momentum"] != 0 and "buf" not in st and hyper is None:  # the first step, or a torch.optim.SGD checkpoint
                    skip = {id(p) for p in rest}
                    self._adopt_reference_state(pb, group, [p for p in group["params"] if id(p) not in skip and p.requires_grad], key)
                self._update(pb, gb, st, group, hyper, coef)
                bump_param_epoch()  # raw-pointer writes bump no torch version counter: tell the engines
            for p in rest:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "momentum_buffer" in st:  # a torch.optim.SGD checkpoint: its buffer under this class's name (None: first step)
                    mb = st.pop("momentum_buffer")
                    if mb is not None and "buf" not in st:
                        st["buf"] = mb.to(device=p.device, dtype=torch.float32).contiguous()
                self._update(p.data, p.grad, st, group, hyper, coef)
            bump_param_epoch()
        return loss


class FusedMuon(FusedArenaOptimizer):
    """``torch.optim.Muon``'s update (``configs/optimizer/muon.yaml``: momentum, then ``ns_steps`` quintic Newton-Schulz iterations
    per weight matrix in bf16) for the hidden matrices of a model and ``torch.optim.AdamW``'s for everything else, over the flat
    parameter arena.  Unlike torch's class it takes a whole model (a module or all of its parameters).

    A parameter takes the Muon rule iff it is 2-D and both dimensions are multiples of 64 -- in the transformer engines exactly the
    hidden matrices; biases, gains, embedding tables with ``n_classes + 1`` rows, ``conv_proj.weight`` and a 16-row output head take
    AdamW with ``aux_lr`` (``None``: ``lr``), ``aux_betas``, ``aux_eps``, ``aux_weight_decay``.  A param group with ``use_muon: False``
    keeps all its tensors on the auxiliary rule; ``use_muon: True`` insists and raises on a tensor that does not qualify.

    Launches of one ``step()`` per arena (and per tensor outside it), whatever the number of matrices: ``1 + (2 + 3 * ns_steps) + 1``
    = 19 at the default five iterations -- the elementwise pre pass (AdamW on auxiliary ranges; momentum, bf16 staging and partial
    sums of squares on Muon ranges), the fold of the norms, the scaling, three grouped GEMM launches per iteration (Gram, polynomial,
    apply) and the post pass -- or one (the pre pass) when nothing qualifies, plus with ``max_grad_norm`` one sum of squares per
    buffer and the fold of `FusedArenaOptimizer`.  The momentum rule is the one torch's class executes (``buf.lerp_(grad, 1 -
    momentum)``; ``grad.lerp(buf, momentum)`` with Nesterov), which is its docstring's ``B = momentum * B + g`` up to the factor
    ``1 - momentum`` the normalisation removes.

    State: ``m`` (arena-sized f32: AdamW's first moment on auxiliary ranges, the Muon momentum buffer on Muon ranges), ``v`` (AdamW's
    second moment; arena-sized, unused on Muon ranges, absent for a loose Muon matrix) and ``step`` under the group's first arena
    parameter, the same three per tensor outside the arena.  The matrix table, the chunk table and the bf16 workspaces (two copies
    of X, A and P) are not state: they are built once per arena and rebuilt only when the arena scan runs again.  ``grad_scale``,
    ``last_grad_norm`` and ``zero_grad`` are `FusedArenaOptimizer`'s; captured steps are not supported."""

    def __init__(self, params, lr: float = 1e-3, weight_decay: float = 0.1, momentum: float = 0.95, nesterov: bool = True,
                 ns_coefficients: tuple[float, float, float] = (3.4445, -4.7750, 2.0315), eps: float = 1e-7, ns_steps: int = 5,
                 adjust_lr_fn: str | None = None, aux_lr: float | None = None, aux_betas: tuple[float, float] = (0.9, 0.999),
                 aux_eps: float = 1e-8, aux_weight_decay: float = 1e-2, max_grad_norm: float | None = None) -> None:
        if isinstance(lr, Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {lr}")
        if not 0.0 <= momentum:
            raise ValueError(f"momentum should be >= 0 but is: {momentum}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"weight decay should be >= 0 but is: {weight_decay}")
        if adjust_lr_fn is not None and adjust_lr_fn not in ["original", "match_rms_adamw"]:
            raise ValueError(f"Adjust learning rate function {adjust_lr_fn} is not supported")
        # (torch raises these two from the first step(), inside _zeropower_via_newtonschulz)
        if ns_steps >= 100:
            raise ValueError("Number of steps must be less than 100 for computational efficiency")
        if len(ns_coefficients) != 3:
            raise ValueError("Coefficients must be a tuple of exactly 3 values")
        if ns_steps < 0:
            raise ValueError(f"ns_steps should be >= 0 but is: {ns_steps}")
        if aux_lr is not None and not 0.0 <= aux_lr:
            raise ValueError(f"Learning rate should be >= 0 but is: {aux_lr}")
        if isinstance(params, torch.nn.Module):
            params = params.parameters()
        super().__init__(params, dict(lr=float(lr), weight_decay=weight_decay, momentum=momentum, nesterov=nesterov,
                                      ns_coefficients=tuple(ns_coefficients), eps=eps, ns_steps=ns_steps, adjust_lr_fn=adjust_lr_fn,
                                      aux_lr=aux_lr, aux_betas=tuple(aux_betas), aux_eps=aux_eps, aux_weight_decay=aux_weight_decay,
                                      use_muon=None), max_grad_norm)
        self._plans: dict = {}
        for group in self.param_groups:
            if group["use_muon"]:
                for p in group["params"]:
                    if not self.qualifies(p):
                        raise ValueError(f"use_muon=True on a parameter of shape {tuple(p.shape)}: the Muon rule takes 2-D tensors whose "
                                         "dimensions are both multiples of 64")

    @staticmethod
    def qualifies(p: Tensor) -> bool:
        return p.ndim == 2 and p.shape[0] % ops.MUON_TILE == 0 and p.shape[1] % ops.MUON_TILE == 0

    def is_muon(self, p: Tensor, group: dict) -> bool:
        """does `p` (a parameter of `group`) take the Muon rule?"""
        return group.get("use_muon") is not False and self.qualifies(p)

    def begin_graph_mode(self) -> None:
        raise NotImplementedError("FusedMuon has no captured-step form: its launch count depends on ns_steps and its scalars travel "
                                  "by value")

    def _flat_scan(self, group):
        self._plans.pop(("arena", id(group)), None)  # (the arena scan runs again: its tables are rebuilt with it)
        return super()._flat_scan(group)

    def _plan(self, key, buf: Tensor, matrices) -> "ops.MuonPlan":
        sig = (buf.data_ptr(), buf.numel(), buf.device)
        hit = self._plans.get(key)
        if hit is None or hit[0] != sig:
            hit = self._plans[key] = (sig, ops.MuonPlan(buf.numel(), matrices(), (buf.data_ptr() // 4) % 4, buf.device))
        return hit[1]

    def _update(self, p: Tensor, g: Tensor, st: dict, group: dict, plan, coef: Tensor | None) -> None:
        if not st:
            st["step"], st["m"] = 0, torch.zeros_like(p)
            if plan.has_aux:
                st["v"] = torch.zeros_like(p)
        if st["m"].numel() != p.numel() or (plan.has_aux and "v" not in st):
            raise RuntimeError(f"optimizer state does not match its parameters: moments of {st['m'].numel()} elements for {p.numel()}")
        for k in ("m", "v"):
            if k in st and st[k].device != p.device:  # state loaded before the model moved
                st[k] = st[k].to(p.device)
        st["step"] = int(st["step"]) + 1
        b1, b2 = group["aux_betas"]
        ops.muon_pre(plan, p, g, st["m"], st.get("v"), group["lr"] if group["aux_lr"] is None else group["aux_lr"], b1, b2,
                     group["aux_eps"], group["aux_weight_decay"], st["step"], group["momentum"], group["nesterov"], self.grad_scale, coef)
        if plan.n_mat:
            ops.muon_orthogonalize(plan, group["eps"], group["ns_coefficients"], group["ns_steps"])
            ops.muon_post(plan, p, group["lr"], group["weight_decay"], group["ns_steps"])

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        coef = self._clip_pass() if self.max_grad_norm is not None else None
        for group in self.param_groups:
            flat = self._flat(group)
            rest = group["params"]
            if flat is not None:
                pb, gb, rest = flat
                skip = {id(p) for p in rest}

                def arena_matrices():
                    base = pb.storage_offset()
                    found = [(p.data.storage_offset() - base, p.shape[0], p.shape[1], ops.muon_ratio(*p.shape, group["adjust_lr_fn"]))
                             for p in group["params"] if id(p) not in skip and p.requires_grad and self.is_muon(p, group)]
                    return sorted(found)

                # (keyed on the group's first arena parameter, for the reason FusedAdamW.step gives)
                self._update(pb, gb, self.state[self._arena_key(group, rest)], group, self._plan(("arena", id(group)), pb, arena_matrices),
                             coef)
                bump_param_epoch()  # raw-pointer writes bump no torch version counter: tell the engines
            for p in rest:
                if p.grad is None:
                    continue
                muon = self.is_muon(p, group)
                plan = self._plan(("tensor", id(p)), p.data, lambda: (
                    [(0, p.shape[0], p.shape[1], ops.muon_ratio(*p.shape, group["adjust_lr_fn"]))] if muon else []))
                self._update(p.data, p.grad, self.state[p], group, plan, coef)
            bump_param_epoch()
        return loss
