"""``UNetModel`` denoiser, MI355X build -- drop-in for ``diffulab.networks.denoisers.unet.UNetModel``.

Same constructor kwargs (unet.py:531-551 of the reference), same ``forward`` kwargs (unet.py:749-757), same ``state_dict``
key names / shapes (``input_blocks.{i}.{j}...``, ``middle_block.{j}...``, ``output_blocks.{i}.{j}...``, ``out.{0,2}``,
``time_embed.{0,2}``, ``label_embed.embedding``) and the same initialisation (torch defaults, ``zero_module`` on the second
conv of every ResBlock and on the output conv: unet.py:172,744), so Hydra ``_target_`` configs (configs/model/unet.yaml,
configs/train_mnist_ddpm.yaml) and ``denoiser.pt`` checkpoints carry over.  The ``nn.Module`` tree below only OWNS the
parameters (views into one flat HBM arena); the arithmetic is the hand-written HIP path driven by
``diffulab_amd.unet_engine.UNetEngine``.  No PyTorch/CPU fallback exists.

Covered: FiLM (``use_scale_shift_norm=True``, what ``configs/model/unet.yaml`` builds) and additive conditioning, ResBlock
resampling (``resblock_updown=True``) and the plain ``Downsample`` / ``Upsample`` modules with or without their 3x3 conv
(``conv_resample``), labels or unconditional -- the constructor defaults included -- and text / multimodal conditioning through a
parameter-free context embedder with one output (``context_embedder=``, ``transformer_depth=``): a ``TransformerBlock`` (unet.py:409-464:
self-attention, masked cross-attention to the context tokens, GEGLU feed-forward) wherever an ``AttentionBlock`` would go, the middle
block included.  The context contract is the reference's: ``embeddings`` channel-first ``[B, C_ctx, L]`` (a ``[B, L, C]`` tensor raises
``ValueError``, nothing is transposed), ``attn_mask`` a boolean ``[B, L]`` (True = attend) or absent; a context model takes ``p = 0``
only (unet.py:825-831), so guided sampling raises the reference's ``AssertionError``.  Trainable or pooled-embedding context
embedders raise ``NotImplementedError``.

Dropout (``dropout=p``, 0 <= p < 1) is built for the unconditional and class-conditional UNet, at the reference's two sites:
``ResBlock.out_layers`` (GroupNorm -> SiLU -> Dropout -> conv, unet.py:171) and ``AttentionBlock.to_out`` (Conv1d -> Dropout in front of
the residual add, unet.py:272).  Masks are applied iff ``self.training and p > 0`` (``nn.Dropout``'s rule: a no-grad forward in
training mode has them, every eval-mode path is untouched) by the stand-alone HIP kernel ``dl_dropout``: element i of a block's
``[B * pixels, C]`` activation is dropped iff a 16-bit half of Philox4x32-10(counter (i >> 3, block index, step), key seed) is below
``floor(p * 65536 + 0.5)`` -- p is quantised to 1 / 65536 -- and kept elements are scaled by ``float32(1 / (1 - p))``.  The backward
regenerates the forward's masks; nothing is stored.  ``set_dropout_seed(seed, step=0)`` fixes the stream (otherwise the seed is
drawn from torch's global CPU generator at the first active forward); every active forward advances ``step`` by one; a data-parallel
rank uses ``seed + rank``.  With a context embedder ``dropout > 0`` raises ``NotImplementedError`` (the TransformerBlock's sites are not
built).
"""

from __future__ import annotations

from typing import Any

import torch
import torch.distributed as dist
import torch.nn as nn
from torch import Tensor

from ...unet_engine import UNetDims, UNetEngine, build_plan
from .common import FlatArenaDenoiser, ModelOutput
from ...diffuse.utils import to_device
from .mmdit import _LabelEmbed


def dropout_rank_seed(seed: int, rank: int) -> int:
    """the seed a data-parallel rank's masks are drawn under: ranks see different samples and must not share masks"""
    return (int(seed) + int(rank)) & ((1 << 64) - 1)


class _ResBlock(nn.Module):  # parameter holder for unet.py:80-237
    def __init__(self, cin: int, cout: int, emb: int, film: bool, dropout: float = 0.0) -> None:
        super().__init__()
        self.in_layers = nn.Sequential(nn.GroupNorm(32, cin), nn.SiLU(), nn.Conv2d(cin, cout, 3, padding=1))
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb, 2 * cout if film else cout))
        conv = nn.Conv2d(cout, cout, 3, padding=1)
        for p in conv.parameters():  # zero_module (unet.py:172)
            p.detach().zero_()
        self.out_layers = nn.Sequential(nn.GroupNorm(32, cout), nn.SiLU(), nn.Dropout(dropout), conv)
        self.skip_connection = nn.Identity() if cin == cout else nn.Conv2d(cin, cout, 1)


class _Downsample(nn.Module):  # parameter holder for nn.py:59-88
    def __init__(self, c: int, use_conv: bool) -> None:
        super().__init__()
        self.op = nn.Conv2d(c, c, 3, stride=2, padding=1) if use_conv else nn.AvgPool2d(kernel_size=2, stride=2)


class _Upsample(nn.Module):  # parameter holder for nn.py:28-56
    def __init__(self, c: int, use_conv: bool) -> None:
        super().__init__()
        if use_conv:
            self.conv = nn.Conv2d(c, c, 3, padding=1)


class _AttentionBlock(nn.Module):  # parameter holder for unet.py:240-322
    def __init__(self, c: int, context_channels: int | None = None, dropout: float = 0.0) -> None:
        super().__init__()
        cc = context_channels or c
        self.norm_x = nn.GroupNorm(32, c)
        self.norm_context = nn.GroupNorm(32, cc)
        self.to_q = nn.Conv1d(c, c, 1)
        self.to_kv = nn.Conv1d(cc, 2 * c, 1)
        self.to_out = nn.Sequential(nn.Conv1d(c, c, 1), nn.Dropout(dropout))


class _GEGLU(nn.Module):  # parameter holder for unet.py:325-336
    def __init__(self, cin: int, cout: int) -> None:
        super().__init__()
        self.proj = nn.Conv1d(cin, 2 * cout, 1)


class _FeedForward(nn.Module):  # parameter holder for unet.py:339-355
    def __init__(self, c: int, inner: int) -> None:
        super().__init__()
        self.net = nn.Sequential(_GEGLU(c, inner), nn.Dropout(0.0), nn.Conv1d(inner, c, 1))
        self.norm = nn.GroupNorm(32, c)


class _TransformerAttentionBlock(nn.Module):  # parameter holder for unet.py:358-406
    def __init__(self, c: int, context_channels: int) -> None:
        super().__init__()
        self.self_attn = _AttentionBlock(c)
        self.cross_attn = _AttentionBlock(c, context_channels)
        self.ff = _FeedForward(c, 4 * c)


class _TransformerBlock(nn.Module):  # parameter holder for unet.py:409-464 (proj_out is not zero-initialised there)
    def __init__(self, c: int, context_channels: int, depth: int) -> None:
        super().__init__()
        self.norm_x = nn.GroupNorm(32, c)
        self.proj_in = nn.Conv2d(c, c, 1)
        self.attn_blocks = nn.ModuleList([_TransformerAttentionBlock(c, context_channels) for _ in range(depth)])
        self.proj_out = nn.Conv2d(c, c, 1)


class UNetModel(FlatArenaDenoiser):
    cfg_pair_capable = True  # `p` only reaches the label drop: guided sampler steps batch their two forwards (forward_cfg_pair)

    def __init__(
        self,
        image_size: list[int],
        in_channels: int,
        model_channels: int,
        out_channels: int,
        num_res_blocks: int,
        attention_resolutions: list[int],
        dropout: float = 0,
        channel_mult: str = "1, 2, 4, 8",
        conv_resample: bool = True,
        use_checkpoint: bool = False,
        num_heads: int = 1,
        use_scale_shift_norm: bool = False,
        resblock_updown: bool = False,
        n_classes: int | None = None,
        classifier_free: bool = False,
        context_embedder: Any | None = None,
        transformer_depth: int = 1,
    ) -> None:
        super().__init__()
        assert not (n_classes is not None and context_embedder is not None), (
            "n_classes and context_embedder cannot both be specified")
        if context_embedder:
            assert context_embedder.n_output == 1, (
                "For UNet please provide a context embedder with n_output=1 (context and attention mask)")
            if any(True for _ in context_embedder.parameters()):
                raise NotImplementedError("diffulab_amd.UNetModel: the context embedder must be parameter-free (precomputed embeddings)")
        dropout = float(dropout)
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"diffulab_amd.UNetModel: dropout must satisfy 0 <= p < 1 (got {dropout!r})")
        if dropout and context_embedder is not None:
            raise NotImplementedError("diffulab_amd.UNetModel: dropout > 0 is built for the unconditional and class-conditional UNet "
                                      "only; the text-conditioned TransformerBlock's sites (the to_out Dropout of its self- and "
                                      "cross-attention, FeedForward.net.1) are not built")
        self._dropout_seed: int | None = None  # host-side mask state: set_dropout_seed, or drawn at the first active forward
        self._dropout_step = 0
        self.image_size = list(image_size)
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        self.num_res_blocks = num_res_blocks
        self.attention_resolutions = list(attention_resolutions)
        self.dropout = dropout
        self.channel_mult: list[int] = [int(v) for v in str(channel_mult).split(",")]
        self.conv_resample = conv_resample
        self.use_checkpoint = use_checkpoint  # activations stay resident in HBM; nothing to checkpoint
        self.num_heads = num_heads
        self.context_channels = None if context_embedder is None else int(context_embedder.output_size[0])
        self.transformer_depth = transformer_depth
        self.use_context = self.context_channels is not None
        self.context_embedder = context_embedder
        if self.use_context:
            self.cfg_pair_capable = False  # p > 0 is refused for context models (unet.py:825-831): no batched guided pair either
        self.classifier_free = classifier_free
        self.n_classes = n_classes
        self.time_embed_dim = model_channels * 4
        self.dims = UNetDims(image_size=tuple(self.image_size), in_channels=in_channels, model_channels=model_channels,
                             out_channels=out_channels, num_res_blocks=num_res_blocks,
                             attention_resolutions=tuple(self.attention_resolutions), channel_mult=tuple(self.channel_mult),
                             num_heads=num_heads, use_scale_shift_norm=use_scale_shift_norm, resblock_updown=resblock_updown,
                             conv_resample=conv_resample, n_classes=n_classes, classifier_free=classifier_free,
                             context_channels=self.context_channels, transformer_depth=transformer_depth, dropout=dropout)
        self.dims.validate()

        te = self.time_embed_dim
        self.time_embed = nn.Sequential(nn.Linear(model_channels, te), nn.SiLU(), nn.Linear(te, te))
        self.label_embed = _LabelEmbed(n_classes, te, classifier_free) if n_classes is not None else None
        plan = build_plan(self.dims)

        def group(blocks) -> nn.Sequential:
            mods: list[nn.Module] = []
            for b in blocks:
                if b.kind == "conv":
                    mods.append(nn.Conv2d(b.cin, b.cout, 3, padding=1))
                elif b.kind == "res":
                    mods.append(_ResBlock(b.cin, b.cout, te, use_scale_shift_norm, dropout))
                elif b.kind == "down":
                    mods.append(_Downsample(b.cin, conv_resample))
                elif b.kind == "up":
                    mods.append(_Upsample(b.cin, conv_resample))
                elif b.kind == "xf":
                    mods.append(_TransformerBlock(b.cin, self.context_channels, transformer_depth))
                else:
                    mods.append(_AttentionBlock(b.cin, dropout=dropout))
            return nn.Sequential(*mods)

        self.input_blocks = nn.ModuleList([group(g) for g in plan.input_blocks])
        self.middle_block = group(plan.middle)
        self.output_blocks = nn.ModuleList([group(g) for g in plan.output_blocks])
        conv = nn.Conv2d(int(self.channel_mult[0] * model_channels), out_channels, 3, padding=1)
        for p in conv.parameters():  # zero_module (unet.py:744)
            p.detach().zero_()
        self.out = nn.Sequential(nn.GroupNorm(32, plan.final_ch), nn.SiLU(), conv)

    precisions = ("bf16", "fp32")  # the fp32-class regime: unet_engine_f32.py (round 4)

    def _make_engine(self, device: torch.device) -> UNetEngine:
        if self.precision == "fp32":
            from ...unet_engine_f32 import UNetEngineF32

            return UNetEngineF32(self.dims, device)
        return UNetEngine(self.dims, device)

    # ------------------------------------------------------------------ forward (unet.py:749-853)
    def forward(
        self,
        x: Tensor,
        timesteps: Tensor,
        y: Tensor | None = None,
        context: Any | None = None,
        p: float = 0.0,
        x_context: Tensor | None = None,
    ) -> ModelOutput:
        assert (y is not None) == (self.n_classes is not None), "must specify y if and only if the model is class-conditional"
        assert (context is not None) == (self.context_embedder is not None), (
            "must specify context if and only if the model is context-conditional")
        if p > 0:
            assert self.classifier_free, (
                "probability of dropping for classifier free guidance is only available if model is set up to be classifier free")
            assert self.n_classes, (
                "probability of dropping for classifier free guidance is only available if a number of classes is set")
        if x_context is not None:
            x = torch.cat([x, x_context], dim=1)
        assert list(x.shape[2:]) == self.image_size, f"Input shape {x.shape[2:]} does not match model image size {self.image_size}"
        dev = self.engine.dev
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        t = to_device(timesteps, dev, torch.float32)
        y_eff = None
        if self.label_embed is not None:
            y_eff = self._effective_labels(y.to(device=dev, dtype=torch.int64), p).contiguous()  # (drop_labels nn.py:149)
        if self.context_embedder is not None:
            self.engine.context = self._context_inputs(context, p, x.shape[0], dev)
        self._dropout_begin()
        return {"x": self._run(x, t, y_eff)}

    # ------------------------------------------------------------------ dropout (unet.py:171, :272)
    @property
    def dropout_active(self) -> bool:
        """the reference's rule: nn.Dropout follows ``module.training``, not grad mode"""
        return bool(self.training and self.dropout > 0)

    def set_dropout_seed(self, seed: int, step: int = 0) -> None:
        """masks are a pure function of (seed + rank, step, block, element); every dropout-active forward uses the current step
        (its backward the same one) and advances it by one"""
        self._dropout_seed, self._dropout_step = int(seed), int(step)

    def _dropout_begin(self) -> None:
        """tell the engine whether this forward applies masks and, if so, hand it (seed, step): an asynchronous 16-byte copy in
        front of the launch sequence, outside any recorded plan or captured graph; no device value is read back"""
        eng = self.engine
        eng.drop_active = self.dropout_active
        if not eng.drop_active:
            return
        if self._dropout_seed is None:  # drawn once, from torch's global CPU generator: torch.manual_seed governs it
            self._dropout_seed = int(torch.randint(0, 2**62, (1,), dtype=torch.int64, device="cpu").item())
        rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        eng.set_dropout_state(dropout_rank_seed(self._dropout_seed, rank), self._dropout_step)
        self._dropout_step += 1

    def _graph_key(self, eng) -> tuple | None:
        return None if self.dropout_active else ()  # a no-grad forward in training mode runs eagerly, with masks: no hipGraph replay

    def _context_inputs(self, context: Any, p: float, B: int, dev: torch.device) -> tuple[Tensor, Tensor | None]:
        """unet.py:838-841: the embedder runs host-side; -> (embeddings f32 [B, C_ctx, L], key bias f32 [B, L] (0 / -inf) or None)"""
        out = self.context_embedder(context, p)
        emb = out["embeddings"]
        if emb.dim() != 3 or emb.shape[0] != B or emb.shape[1] != self.context_channels:
            raise ValueError(f"diffulab_amd.UNetModel: context embeddings must be channel-first [B, C_ctx, L] = [{B}, "
                             f"{self.context_channels}, L] (the reference's layout: they enter GroupNorm(32, C_ctx) and a Conv1d), got "
                             f"{tuple(emb.shape)}")
        emb = emb.to(device=dev, dtype=torch.float32).contiguous()
        mask = out.get("attn_mask")
        if mask is None:
            return emb, None
        if tuple(mask.shape) != (B, emb.shape[2]):
            raise ValueError(f"diffulab_amd.UNetModel: attn_mask must be [B, L] = [{B}, {emb.shape[2]}], got {tuple(mask.shape)}")
        keep = mask.to(device=dev).bool()
        bias = torch.zeros(keep.shape, device=dev, dtype=torch.float32).masked_fill_(~keep, float("-inf"))
        return emb, bias

    # the context is a per-call input of the launch sequence: a captured graph reads static copies of it
    def _graph_inputs(self, eng) -> tuple:
        return tuple(eng.context) if self.use_context else ()

    def _graph_set_inputs(self, eng, tensors: tuple) -> None:
        if self.use_context:
            eng.context = tuple(tensors)
