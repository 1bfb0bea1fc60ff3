from __future__ import annotations

from typing import Any


class AverageMeter:
    """running means keyed by name (reference training/utils.py:1-25: ``keys`` / ``avg`` / ``sum`` / ``count``, ``update(val, key, n)``,
    ``reset()``).

    ``update`` also takes a 0-d DEVICE tensor (the trainer hands in ``loss.detach()`` instead of ``loss.item()``): the value is read
    back LATER -- when ``avg`` / ``sum`` / ``count`` are looked at, at ``reset()``, or after ``MAX_PENDING`` updates -- with one stacked
    device-to-host copy per flush, and then enters the sums in the order of the calls, as the same Python floats ``.item()`` would
    have produced.  The reference's per-step ``loss.item()`` (base_trainer.py:122) is a host synchronisation between the forward and
    the backward of EVERY step; nothing reads the meter before the end of an epoch."""

    MAX_PENDING = 256

    def __init__(self) -> None:
        self.keys: list[str] = []
        self._avg: dict[str, float] = {}
        self._sum: dict[str, float] = {}
        self._count: dict[str, int] = {}
        self._pending: list[tuple[Any, str, int]] = []

    # the three dictionaries of the reference, flushed on access
    @property
    def avg(self) -> dict[str, float]:
        self.flush()
        return self._avg

    @property
    def sum(self) -> dict[str, float]:
        self.flush()
        return self._sum

    @property
    def count(self) -> dict[str, int]:
        self.flush()
        return self._count

    def reset(self) -> None:
        self.flush()
        for k in self.keys:
            self._avg[k], self._sum[k], self._count[k] = 0, 0, 0

    def _add(self, val: float, key: str, n: int) -> None:
        if key not in self.keys:
            self.keys.append(key)
            self._sum[key], self._count[key] = 0.0, 0
        self._sum[key] += val * n
        self._count[key] += n
        self._avg[key] = self._sum[key] / self._count[key]

    def update(self, val: Any, key: str, n: int = 1) -> None:
        if hasattr(val, "is_cuda") and val.is_cuda and val.dim() == 0:
            if key not in self.keys:  # (the key exists from the first call on, like in the reference)
                self.keys.append(key)
                self._sum[key], self._count[key] = 0.0, 0
                self._avg[key] = 0
            self._pending.append((val.detach(), key, n))
            if len(self._pending) >= self.MAX_PENDING:
                self.flush()
            return
        self.flush()
        self._add(float(val), key, n)

    def flush(self) -> None:
        if not self._pending:
            return
        import torch

        pend, self._pending = self._pending, []
        vals = torch.stack([v.float() if v.dtype != torch.float64 else v for v, _, _ in pend]).tolist()  # one copy, one sync
        for v, (_, key, n) in zip(vals, pend):
            self._add(v, key, n)


def clip_grad_norm_(parameters: Any, max_norm: float, grad_scale: float = 1.0):
    """``torch.nn.utils.clip_grad_norm_`` (norm_type=2, error_if_nonfinite=False) on the HIP path, for optimizers other than
    ``FusedAdamW`` (which clips inside its update and never rewrites the gradients: ``FusedAdamW(max_grad_norm=...)``): every
    gradient is multiplied IN PLACE by ``min(1, max_norm / (total_norm + 1e-6))`` and the total norm comes back as a 0-d device
    tensor.  Nothing synchronises with the host.

    Gradients are grouped by the storage they live in: a storage that the listed gradients (almost) fill -- the flat gradient arena
    of a denoiser, or a loose tensor's own allocation -- costs ONE sum-of-squares launch and one scale launch; the gradients of a
    storage shared with other data are taken tensor by tensor.  ``grad_scale`` (data parallel: 1/world on SUM-reduced gradients)
    scales the reported norm, and with it the coefficient; the gradients themselves are multiplied by the coefficient only."""
    import torch

    from .. import ops

    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = list({id(p.grad): p.grad for p in parameters if p.grad is not None}.values())
    if not grads:
        raise RuntimeError("clip_grad_norm_: no parameter has a gradient")
    by_store: dict[int, list] = {}
    for g in grads:
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
            raise RuntimeError("clip_grad_norm_ needs contiguous f32 device gradients (there is no fallback path)")
        by_store.setdefault(g.untyped_storage().data_ptr(), []).append(g)
    bufs = []
    for gs in by_store.values():
        store = gs[0].untyped_storage()
        n = store.nbytes() // 4
        if sum(g.numel() for g in gs) >= 0.9 * n:  # (FusedAdamW._flat_scan's ownership rule; the gaps of an arena hold zeros)
            bufs.append(torch.empty(0, dtype=torch.float32, device=gs[0].device).set_(store, 0, (n,)))
        else:
            bufs.extend(g.view(-1) for g in gs)
    dev = bufs[0].device
    partials = torch.empty(sum(ops.grad_sumsq_slots(b.numel()) for b in bufs), device=dev)
    out = torch.empty(2, device=dev)
    slot = 0
    for b in bufs:
        slot += ops.grad_sumsq(b, partials, slot)
    ops.clip_coef(partials, slot, max_norm, out, grad_scale)
    for b in bufs:
        ops.scale_inplace(b, out[1:2])
    return out[0]
