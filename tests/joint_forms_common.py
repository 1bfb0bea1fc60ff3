"""Shared pieces of the joint-form tests (tests/test_joint_forms_*.py) and of their fixture's generator
(tests/golden/make_joint_forms_golden.py): the case table (pooled context embeddings in MMDiT / SprintDiT / DDT, single-stream
encoder blocks in the joint DDT), the named input draws, the parameter-free two-output context embedder and the rule by which a large
gradient tensor is stored (a fixed, well-spread sample of its elements plus its norm).

Nothing here imports the package under test at module level: the generator builds the embedder on the reference's ``ContextEmbedder``
base class, the tests on the port's.
"""

from __future__ import annotations

import torch

B, LC, C_CTX, C_POOL = 2, 12, 96, 48
MASK_LENGTHS = (12, 5)
NULL_MASK_LENGTH = 3          # the null context attends to its first 3 tokens
IMAGE = (4, 16, 16)           # 64 tokens at patch 2
SPRINT_DROP_RATE = 0.5        # 32 of 64 image tokens kept: B * kept = 64 rows
FULL_BELOW = 768              # gradients up to this many elements are stored whole
SAMPLE = 384                  # larger ones: this many elements (sample_index) and the norm of the whole tensor

_BASE = dict(input_channels=4, output_channels=4, inner_dim=128, num_heads=2, mlp_ratio=2, patch_size=2, rope_axes_dim=[16, 24, 24],
             rope_base=1000, classifier_free=True)
_DIT = dict(_BASE, simple_dit=False, embedding_dim=128)
_DDT = dict(_BASE, simple_ddt=False)
# tag -> (class name, constructor kwargs, pooled embedder?, weight seed)
CASES = {
    "mmdit_d2_p": ("MMDiT", dict(_DIT, depth=2), True, 211),
    "mmdit_d3s1_p": ("MMDiT", dict(_DIT, depth=3, n_single_stream_blocks=1), True, 212),
    "sprint_p": ("SprintDiT", dict(_DIT, encoder_depth=1, deep_layers_depth=1, decoder_depth=1, drop_rate=SPRINT_DROP_RATE), True, 213),
    "ddt_e2d1_p": ("DDT", dict(_DDT, encoder_depth=2, decoder_depth=1), True, 214),
    "ddt_e3s1_p": ("DDT", dict(_DDT, encoder_depth=3, n_single_stream_blocks=1, decoder_depth=1), True, 215),
    "ddt_e3s1": ("DDT", dict(_DDT, encoder_depth=3, n_single_stream_blocks=1, decoder_depth=1), False, 216),
    "ddt_e3s2": ("DDT", dict(_DDT, encoder_depth=3, n_single_stream_blocks=2, decoder_depth=1), False, 217),
}


def cases_json() -> str:
    import json

    return json.dumps({k: [c, kw, pooled, seed] for k, (c, kw, pooled, seed) in CASES.items()}, sort_keys=True)


def mask_of(lengths, L: int) -> torch.Tensor:
    return torch.arange(L)[None, :] < torch.tensor(list(lengths))[:, None]


def inputs(synth) -> dict:
    """the named draws every case runs on (synth = oracle.synth)"""
    return dict(x=synth.normal("jf.x", (B, *IMAGE)), t=synth.uniform("jf.t", (B,), lo=0.05, hi=0.95),
                ctx=synth.normal("jf.ctx", (B, LC, C_CTX)), pooled=synth.normal("jf.pool", (B, C_POOL)), mask=mask_of(MASK_LENGTHS, LC),
                g=synth.normal("jf.g", (B, *IMAGE)), scores=synth.uniform("jf.scores", (B, 64)),
                null_ctx=synth.normal("jf.null_ctx", (1, LC, C_CTX)) * 0.5, null_pooled=synth.normal("jf.null_pool", (1, C_POOL)) * 0.5)


def context_of(inp: dict, pooled: bool, device=None) -> dict:
    c = {"embeddings": inp["ctx"], "attn_mask": inp["mask"]}
    if pooled:
        c["pooled_embeddings"] = inp["pooled"]
    return {k: v.to(device) for k, v in c.items()} if device is not None else c


def null_context(inp: dict, pooled: bool, device=None) -> dict:
    """the null triple expanded to the batch: what a forward with every sample dropped runs on"""
    c = {"embeddings": inp["null_ctx"].expand(B, -1, -1).contiguous(), "attn_mask": mask_of((NULL_MASK_LENGTH,) * B, LC)}
    if pooled:
        c["pooled_embeddings"] = inp["null_pooled"].expand(B, -1).contiguous()
    return {k: v.to(device) for k, v in c.items()} if device is not None else c


def embedder_class(base):
    """the parameter-free test embedder on the ``ContextEmbedder`` base class `base` (the reference's or the port's)"""

    class PrecomputedTriple(base):
        """hands precomputed token embeddings [B, L, C], a boolean key mask [B, L] and (pooled) one pooled vector [B, P] per sample
        through; ``drop_conditions`` swaps the null triple in for the dropped samples.  With pooled, ``output_size`` is
        (pooled width, token width), the order the denoisers read it in"""

        def __init__(self, null_ctx: torch.Tensor, null_pooled: torch.Tensor | None) -> None:
            super().__init__()
            self._n_output = 2 if null_pooled is not None else 1
            self._output_size = (null_pooled.shape[-1], null_ctx.shape[-1]) if null_pooled is not None else (null_ctx.shape[-1],)
            self.null_ctx, self.null_pooled = null_ctx, null_pooled  # plain attributes: no parameters, no buffers

        def _draw_drop(self, batch_size: int, p: float, device) -> torch.Tensor:
            return torch.rand(batch_size, device=device) < p

        def drop_conditions(self, context, p):
            emb, mask = context["embeddings"], context["attn_mask"]
            drop = self._draw_drop(emb.shape[0], p, emb.device)
            null_mask = torch.arange(emb.shape[1], device=emb.device) < NULL_MASK_LENGTH
            out = {"embeddings": torch.where(drop[:, None, None], self.null_ctx.to(emb), emb),
                   "attn_mask": torch.where(drop[:, None], null_mask[None, :], mask)}
            if self.null_pooled is not None:
                pooled = context["pooled_embeddings"]
                out["pooled_embeddings"] = torch.where(drop[:, None], self.null_pooled.to(pooled), pooled)
            return out

        def forward(self, context, p: float = 0):
            if p > 0:
                context = self.drop_conditions(context, p)
            out = {"embeddings": context["embeddings"], "attn_mask": context["attn_mask"]}
            if self.null_pooled is not None and "pooled_embeddings" in context:
                out["pooled_embeddings"] = context["pooled_embeddings"]
            return out

    return PrecomputedTriple


def make_embedder(base, inp: dict, pooled: bool):
    return embedder_class(base)(inp["null_ctx"], inp["null_pooled"] if pooled else None)


def sample_index(numel: int) -> torch.Tensor | None:
    """None: the tensor is stored whole; else the SAMPLE flat indices stored of it (a multiplicative hash: spread over rows and
    columns of every matrix shape, unlike a regular stride)"""
    if numel <= FULL_BELOW:
        return None
    return (torch.arange(SAMPLE, dtype=torch.int64) * 2654435761) % numel


def stored(t: torch.Tensor) -> torch.Tensor:
    """the elements of gradient `t` the fixture holds"""
    idx = sample_index(t.numel())
    flat = t.detach().reshape(-1)
    return flat if idx is None else flat[idx.to(flat.device)]
