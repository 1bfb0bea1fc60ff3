"""``BaseTrainer``: the training loop of the reference (training/trainers/base_trainer.py:104-399) on the MI355X runtime.

``training_step`` keeps the reference's order of operations (base_trainer.py:138-153): zero_grad -> draw timesteps (CPU generator)
-> compute_loss -> every loss into the tracker (the reference's ``.item()``; here a device scalar the meter reads back lazily) -> backward -> [clip by
global gradient norm when ``max_grad_norm`` is set: fused into the AdamW / SGD update, ``train/grad_norm`` into the tracker] -> optimizer.step -> scheduler -> EMA update.
What Accelerate did implicitly is spelled out (see trainers/common.py): loss / gradient_accumulation_step before backward,
``zero_grad`` / ``step`` / scheduler gated on the synchronising micro-step (so with k > 1 the default reproduces the reference's
"(1/k) * gradient of the last micro-batch" update), EMA on every micro-step, gradient all-reduce overlapped
with backward.
"""

from __future__ import annotations

import logging
from contextlib import contextmanager
from typing import TYPE_CHECKING, Any, Iterable

import torch
from torch.optim.lr_scheduler import LRScheduler
from torch.optim.optimizer import Optimizer

from ...datasets.base import BatchData
from ..ema import EMA, PowerEMA
from ...diffuse.modelizations.flow import NO_VARIATIONAL_BOUND
from ...diffuse.modelizations.gaussian_diffusion import NO_ODE_LIKELIHOOD
from ...diffuse.utils import to_device
from ..utils import AverageMeter
from .common import Trainer

if TYPE_CHECKING:
    from ...diffuse import Diffuser


BPD_KEYS = ("val/bpd", "val/prior_bpd")  # evaluated on request (train(val_bpd_batches=...)), logged, never part of the criterion
NLL_KEYS = ("val/nll",)  # the ODE likelihood of a flow model (train(val_nll_batches=...)): logged only as well; its val/bpd is in BPD_KEYS


class BaseTrainer(Trainer):
    def training_step(
        self,
        diffuser: "Diffuser",
        optimizer: Optimizer,
        batch: BatchData,
        tracker: AverageMeter,
        p_classifier_free_guidance: float = 0,
        scheduler: LRScheduler | None = None,
        per_batch_scheduler: bool = False,
        ema_denoiser: EMA | None = None,
    ) -> None:
        self.begin_micro_step()
        # AcceleratedOptimizer.zero_grad() only acts while gradient_state.sync_gradients is set, and accumulate() sets that flag
        # for the micro-step being entered: the reference therefore clears the window's gradients right before the LAST backward
        if self.sync_gradients if self.reference_accumulation else self.window_start:
            optimizer.zero_grad()
        batch = self.shard_batch(batch)
        model_inputs = self.move_dict_to_device(dict(batch["model_inputs"]))
        t_host = diffuser.draw_timesteps(model_inputs["x"].shape[0])
        timesteps = to_device(t_host, self.device, t_host.dtype)  # (no host synchronisation: pinned staging ring, diffuse/utils.py)
        model_inputs.update({"p": p_classifier_free_guidance})
        extra = self.move_dict_to_device(dict(batch.get("extra", {})))
        losses = diffuser.compute_loss(model_inputs=model_inputs, timesteps=timesteps, extra_args=extra)
        for key, loss in losses.items():
            # the reference reads `loss.item()` here (base_trainer.py:122): a host synchronisation between forward and backward of
            # every step; the meter takes the device scalar and reads it back when it is looked at (same floats, same order)
            tracker.update(loss.detach(), key=f"train/{key}")
        loss = sum(losses.values())
        (loss / self.gradient_accumulation_step).backward()
        if self.sync_gradients:
            self.reduce_extra_grads(diffuser)
            norm = self.clip_gradients(optimizer) if self.max_grad_norm is not None else None
            optimizer.step()
            if self.max_grad_norm is not None:  # once per accumulation window, on the accumulated gradient; read back with the losses
                tracker.update((optimizer.last_grad_norm if norm is None else norm).clone(), key="train/grad_norm")
            if scheduler is not None and per_batch_scheduler:
                scheduler.step()
        if ema_denoiser is not None:
            ema_denoiser.update()  # counts micro-steps: update_after_step / update_every were scaled in __init__ (common.py:97-98)
            if self.ema_type == "power":
                self._snapshot_power_ema(ema_denoiser)
        self.end_micro_step()

    def _snapshot_power_ema(self, ema: PowerEMA) -> None:
        """rank 0 writes every profile under save_path/phema once per `ema_snapshot_every` profile updates"""
        every = self.ema_snapshot_every
        if every and self.is_main_process and ema.t > 0 and ema.t % every == 0 and ema.t != self.__dict__.get("_phema_t"):
            ema.snapshot(self.save_path / "phema")
            self._phema_t = ema.t  # (update() calls between two profile updates leave t where it was)

    @torch.no_grad()
    def validation_step(self, diffuser: "Diffuser", val_batch: BatchData, tracker: AverageMeter) -> None:
        val_batch = self.shard_batch(val_batch)
        model_inputs = self.move_dict_to_device(dict(val_batch["model_inputs"]))
        timesteps = diffuser.draw_timesteps(model_inputs["x"].shape[0]).to(self.device)
        extra_args = self.move_dict_to_device(dict(val_batch.get("extra", {})))
        val_losses = diffuser.compute_loss(model_inputs=model_inputs, timesteps=timesteps, extra_args=extra_args)
        for key, val_loss in val_losses.items():
            tracker.update(val_loss.detach(), key=f"val/{key}")  # (read back when the meter is looked at, like the training losses)

    @torch.no_grad()
    def bpd_step(self, diffuser: "Diffuser", val_batch: BatchData, tracker: AverageMeter) -> None:
        """the variational bound of one validation batch in bits per dimension (`Diffuser.evaluate_bpd`: the whole chain, fresh noise)
        into the tracker as val/bpd and val/prior_bpd, weighted by the batch size"""
        val_batch = self.shard_batch(val_batch)
        model_inputs = self.move_dict_to_device(dict(val_batch["model_inputs"]))
        out = diffuser.evaluate_bpd(model_inputs)
        n = model_inputs["x"].shape[0]
        tracker.update(out["total_bpd"].mean(), key="val/bpd", n=n)
        tracker.update(out["prior_bpd"].mean(), key="val/prior_bpd", n=n)

    def nll_step(self, diffuser: "Diffuser", val_batch: BatchData, tracker: AverageMeter, nll_args: dict[str, Any] = {}) -> None:
        """the ODE likelihood of one validation batch (`Diffuser.evaluate_nll`: the diffuser's own grid, fresh probes) into the tracker
        as val/nll (nats per dimension) and, in pixel space, val/bpd, weighted by the batch size.  The evaluation differentiates the
        denoiser with respect to its input inside `input_grad_only()`: no parameter gradient is touched."""
        val_batch = self.shard_batch(val_batch)
        model_inputs = self.move_dict_to_device(dict(val_batch["model_inputs"]))
        out = diffuser.evaluate_nll(model_inputs, **nll_args)
        n = model_inputs["x"].shape[0]
        tracker.update(out["nll"].mean(), key="val/nll", n=n)
        if "total_bpd" in out:
            tracker.update(out["total_bpd"].mean(), key="val/bpd", n=n)

    def train(
        self,
        diffuser: "Diffuser",
        optimizer: Optimizer,
        train_dataloader: Iterable[BatchData],
        val_dataloader: Iterable[BatchData] | None = None,
        scheduler: LRScheduler | None = None,
        per_batch_scheduler: bool = False,
        log_validation_images: bool = True,
        train_embedder: bool = False,
        p_classifier_free_guidance: float = 0.2,
        val_steps: int = 50,
        val_step_shift: float | None = None,
        optimizer_ckpt: str | None = None,
        denoiser_ckpt: str | None = None,
        ema_ckpt: str | None = None,
        epoch_start: int = 0,
        val_bpd_batches: int = 0,
        val_nll_batches: int = 0,
        val_nll_args: dict[str, Any] = {},
    ) -> None:
        """val_bpd_batches (this project's): for the first that-many validation batches of each epoch the variational bound is
        evaluated under the same validation context (EMA weights where configured) and logged as val/bpd and val/prior_bpd.  Logged
        only: the sum that picks the best checkpoint leaves them out.  Gaussian diffusion only; at 0 nothing changes."""
        if val_bpd_batches < 0:
            raise ValueError(f"val_bpd_batches must be >= 0, got {val_bpd_batches}")
        if val_bpd_batches and diffuser.model_type == "rectified_flow":
            raise NotImplementedError(NO_VARIATIONAL_BOUND)
        # val_nll_batches / val_nll_args (this project's): the same for the ODE likelihood of a rectified-flow model (`evaluate_nll` with
        # the keywords val_nll_args), logged as val/nll and, in pixel space, val/bpd; logged only; refused for Gaussian diffusion
        if val_nll_batches < 0:
            raise ValueError(f"val_nll_batches must be >= 0, got {val_nll_batches}")
        if val_nll_batches and diffuser.model_type != "rectified_flow":
            raise NotImplementedError(NO_ODE_LIKELIHOOD)
        if val_step_shift is not None:
            assert diffuser.model_type == "rectified_flow", "Time-shifting during validation is only supported for flow-based models."
        p_cfg = p_classifier_free_guidance if diffuser.denoiser.classifier_free else 0
        ema = self._setup_run(diffuser, optimizer, train_embedder, optimizer_ckpt, denoiser_ckpt, ema_ckpt)
        meter, best = AverageMeter(), float("inf")
        logging.info("Begin training")
        for epoch in range(epoch_start, self.n_epoch):
            self._train_epoch(diffuser, optimizer, train_dataloader, meter, p_cfg, scheduler, per_batch_scheduler, ema)
            self._log_group(meter, "train/", epoch + 1)
            meter.reset()
            if val_dataloader is not None:
                with self._validating(diffuser, ema) as online:
                    for i, val_batch in enumerate(self.even_batches(val_dataloader)):
                        self.validation_step(diffuser=diffuser, val_batch=val_batch, tracker=meter)
                        if i < val_bpd_batches:
                            self.bpd_step(diffuser=diffuser, val_batch=val_batch, tracker=meter)
                        if i < val_nll_batches:
                            self.nll_step(diffuser=diffuser, val_batch=val_batch, tracker=meter, nll_args=val_nll_args)
                    val_total = self.val_total = self._log_group(meter, "val/", epoch + 1, logged_only=BPD_KEYS + NLL_KEYS)
                    if log_validation_images and self.is_main_process:
                        logging.info("creating validation images")
                        self.log_images(diffuser, val_dataloader, epoch, val_steps, step_shift=val_step_shift,
                                        guidance_scale=4 if online.classifier_free else 0)
                if val_total < best:  # (the checkpoint holds the online weights AND the EMA copy, base_trainer.py:246-251)
                    best = val_total
                    self.save_model(optimizer, diffuser, ema, scheduler)
                meter.reset()
            self.wait_for_everyone()
        logging.info("Training complete")

    # ---- the pieces of train() (reference: one function, base_trainer.py:277-399; same order of effects)
    def _setup_run(self, diffuser: "Diffuser", optimizer: Optimizer, train_embedder: bool, optimizer_ckpt: str | None,
                   denoiser_ckpt: str | None, ema_ckpt: str | None) -> EMA | PowerEMA | None:
        """checkpoints in, device placement / rank-0 broadcast / reducer (``prepare``), the EMA copy, auxiliary loss heads hooked
        onto the denoiser, a frozen context embedder unless it is trained"""
        if denoiser_ckpt:
            diffuser.denoiser.load_state_dict(torch.load(denoiser_ckpt))
        self.prepare(diffuser, optimizer)
        if optimizer_ckpt:  # after prepare(): the state follows the parameters' device (and the arena exists)
            optimizer.load_state_dict(torch.load(optimizer_ckpt, weights_only=False))
        ema = None
        if self.use_ema and self.ema_type == "power":
            ema = PowerEMA(diffuser.denoiser, sigma_rels=self.ema_sigma_rels, update_every=self.ema_update_every,
                           eval_sigma_rel=self.ema_eval_sigma_rel).to(self.device)
            if ema_ckpt:  # ema_state.pt of save_model: t, the call counter and every profile
                ema.load_state_dict(torch.load(ema_ckpt, weights_only=True))
        elif self.use_ema:
            ema = EMA(diffuser.denoiser, beta=self.ema_rate, update_after_step=self.ema_update_after_step,
                      update_every=self.ema_update_every).to(self.device)
            if ema_ckpt:
                ema.ema_model.load_state_dict(torch.load(ema_ckpt, weights_only=True))
        for head in diffuser.extra_losses:  # accelerator.prepare(loss) in the reference: device placement, then the hooks
            head.to(self.device)
            head.set_model(diffuser.denoiser)
        self.broadcast_extra_losses(diffuser)
        embedder = getattr(diffuser.denoiser, "context_embedder", None)
        if embedder is not None and not train_embedder:
            for q in embedder.parameters():
                q.requires_grad = False
        return ema

    def _train_epoch(self, diffuser: "Diffuser", optimizer: Optimizer, loader: Iterable[BatchData], meter: AverageMeter, p_cfg: float,
                     scheduler: LRScheduler | None, per_batch_scheduler: bool, ema: EMA | None) -> None:
        diffuser.train()
        for batch in self.iterate(loader):
            self.training_step(diffuser=diffuser, optimizer=optimizer, batch=batch, tracker=meter, p_classifier_free_guidance=p_cfg,
                               scheduler=scheduler, per_batch_scheduler=per_batch_scheduler, ema_denoiser=ema)
        if scheduler is not None and not per_batch_scheduler:
            scheduler.step()

    def _log_group(self, meter: AverageMeter, prefix: str, step: int, logged_only: tuple[str, ...] = ()) -> float:
        """log the rank-mean of every tracked average under ``prefix``; returns their sum (the validation criterion) without the
        keys in ``logged_only``"""
        total = 0.0
        for key, value in meter.avg.items():
            if key.startswith(prefix):
                mean = self.gather_mean(value)
                self.log({key: mean}, step=step)
                if key not in logged_only:
                    total += mean
        return total

    @contextmanager
    def _validating(self, diffuser: "Diffuser", ema: EMA | None):
        """eval mode with the EMA weights in place of the online ones (and the auxiliary heads hooked onto them); yields the online
        denoiser and puts everything back on exit"""
        diffuser.eval()
        online = diffuser.denoiser
        if ema is not None:
            diffuser.denoiser = ema.ema_model.eval()
            for head in diffuser.extra_losses:
                head.set_model(ema.ema_model)
        try:
            yield online
        finally:
            if ema is not None:
                diffuser.denoiser = online
                for head in diffuser.extra_losses:
                    head.set_model(online)
