"""Shared pieces of the text-conditioned UNet tests (tests/test_unet_context_*.py): the parameter-free channel-first context
embedder of tests/golden/make_unet_context_golden.py and the fixture's cases, built on the port's classes."""

from __future__ import annotations

import torch

from diffulab_amd.networks.embedders.common import ContextEmbedder

B, L, C_CTX = 4, 20, 96
MASK_LENGTHS = (20, 7, 1, 0)
TIMESTEPS = (3, 500, 999, 0)
BASE = dict(image_size=[16, 16], in_channels=3, model_channels=32, out_channels=3, num_res_blocks=1, attention_resolutions=[2],
            channel_mult="1, 2", num_heads=2)
CASES = {
    "d1": dict(BASE, use_scale_shift_norm=True, resblock_updown=True, transformer_depth=1),
    "d2": dict(BASE, use_scale_shift_norm=True, resblock_updown=True, transformer_depth=2),
    "dflt": dict(BASE, transformer_depth=1),
}


class ChannelFirstEmbedder(ContextEmbedder):
    """parameter-free: hands precomputed channel-first embeddings [B, C_ctx, L] and a boolean key mask [B, L] through"""

    def __init__(self, channels: int, n_output: int = 1) -> None:
        super().__init__()
        self._n_output = n_output
        self._output_size = (channels,)

    def drop_conditions(self, context, p):
        return context

    def forward(self, context, p: float = 0):
        out = {"embeddings": context["embeddings"]}
        if context.get("attn_mask") is not None:
            out["attn_mask"] = context["attn_mask"]
        return out


def mask_of(lengths, L: int) -> torch.Tensor:
    return torch.arange(L)[None, :] < torch.tensor(list(lengths))[:, None]
