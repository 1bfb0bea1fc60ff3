"""Text-conditioned UNetModel (context embedder -> TransformerBlocks, unet.py:358-464), host side: the constructor's parameter tree
against the reference's (tests/golden/unet_context.npz), the reference's assertion / error paths, the engine plan and arena layout,
and the new C-ABI entry points."""

import pytest
import torch

from unet_context_common import B, C_CTX, CASES, L, MASK_LENGTHS, ChannelFirstEmbedder, mask_of


def _model(tag="d1", **over):
    from diffulab_amd.networks.denoisers import UNetModel

    kw = dict(CASES[tag], **over)
    kw.setdefault("context_embedder", ChannelFirstEmbedder(C_CTX))
    return UNetModel(**kw)


@pytest.mark.parametrize("tag", list(CASES))
def test_state_dict_names_and_shapes_match_the_reference(golden, tag):
    g = golden("unet_context")
    m = _model(tag)
    sd = m.state_dict()
    ref = {n: tuple(int(v) for v in s.split(",")) for n, s in zip(g[f"{tag}_sd_names"].tolist(), g[f"{tag}_sd_shapes"].tolist())}
    assert list(sd) == list(ref)  # (same module order: a reference checkpoint loads key for key)
    assert {n: tuple(t.shape) for n, t in sd.items()} == ref
    # every parameter has its slot in the engine's flat arena
    from diffulab_amd.unet_engine import UNetLayout, build_plan

    assert set(UNetLayout(m.dims, build_plan(m.dims)).entries) == set(dict(m.named_parameters()))


def test_shared_case_definitions_match_the_fixture(golden):
    """tests/unet_context_common.py restates the generator's cases and inputs: they must be what the fixture was made from"""
    import json

    from unet_context_common import TIMESTEPS

    g = golden("unet_context")
    assert json.loads(str(g["cases_json"])) == json.loads(json.dumps(CASES, sort_keys=True))
    assert tuple(g["mask_lengths"].tolist()) == MASK_LENGTHS and tuple(g["timesteps"].tolist()) == TIMESTEPS
    assert tuple(g["shape_b_l_cctx"].tolist()) == (B, L, C_CTX)


def test_plan_puts_transformer_blocks_where_attention_blocks_go():
    from diffulab_amd.unet_engine import build_plan

    m = _model("d2")
    plain = _model("d2", context_embedder=None)
    kinds = [(b.prefix, b.kind) for b in build_plan(m.dims).all_blocks()]
    kinds0 = [(b.prefix, b.kind) for b in build_plan(plain.dims).all_blocks()]
    assert [p for p, _ in kinds] == [p for p, _ in kinds0]
    assert [k for _, k in kinds] == [("xf" if k == "attn" else k) for _, k in kinds0]
    assert ("middle_block.1.", "xf") in kinds
    assert m.dims.context_channels == C_CTX and m.dims.transformer_depth == 2 and plain.dims.context_channels is None


def test_reference_assertions_and_errors():
    from diffulab_amd.networks.denoisers import UNetModel

    with pytest.raises(AssertionError, match="n_classes and context_embedder cannot both be specified"):
        _model(n_classes=10)
    with pytest.raises(AssertionError, match="n_output=1"):
        _model(context_embedder=ChannelFirstEmbedder(C_CTX, n_output=2))

    class WithParams(ChannelFirstEmbedder):
        def __init__(self):
            super().__init__(C_CTX)
            self.proj = torch.nn.Linear(4, 4)

    with pytest.raises(NotImplementedError, match="parameter-free"):
        _model(context_embedder=WithParams())
    with pytest.raises(NotImplementedError, match="dropout"):
        _model(dropout=0.1)
    with pytest.raises(ValueError, match="num_channels must be divisible by num_groups"):  # torch's GroupNorm(32, C_ctx) error
        _model(context_embedder=ChannelFirstEmbedder(48))

    m = _model()
    x, t = torch.zeros(B, 3, 16, 16), torch.zeros(B)
    ctx = {"embeddings": torch.zeros(B, C_CTX, L), "attn_mask": mask_of(MASK_LENGTHS, L)}
    with pytest.raises(AssertionError, match="must specify context if and only if the model is context-conditional"):
        m(x=x, timesteps=t)
    with pytest.raises(AssertionError, match="must specify context if and only if the model is context-conditional"):
        UNetModel(**CASES["d1"])(x=x, timesteps=t, context=ctx)
    with pytest.raises(AssertionError, match="model is set up to be classifier free"):  # a guided sampler step calls p = 1
        m(x=x, timesteps=t, context=ctx, p=1.0)
    # the batched guided pair never takes over (it would turn the reference's AssertionError into a result)
    assert m.forward_cfg_pair(t, x=x, context=ctx) is None


def test_context_layout_is_channel_first():
    m = _model()
    cpu = torch.device("cpu")
    emb, bias = m._context_inputs({"embeddings": torch.randn(B, C_CTX, L), "attn_mask": mask_of(MASK_LENGTHS, L)}, 0.0, B, cpu)
    assert emb.shape == (B, C_CTX, L) and emb.dtype == torch.float32
    assert bias.shape == (B, L) and bias.dtype == torch.float32
    assert torch.equal(bias == 0, mask_of(MASK_LENGTHS, L)) and bool(torch.isneginf(bias[3]).all())
    emb, bias = m._context_inputs({"embeddings": torch.randn(B, C_CTX, L)}, 0.0, B, cpu)
    assert bias is None
    with pytest.raises(ValueError, match=r"channel-first \[B, C_ctx, L\]"):  # PrecomputedEmbedder's [B, L, C]: not transposed
        m._context_inputs({"embeddings": torch.randn(B, L, C_CTX)}, 0.0, B, cpu)
    with pytest.raises(ValueError, match="attn_mask"):
        m._context_inputs({"embeddings": torch.randn(B, C_CTX, L), "attn_mask": mask_of(MASK_LENGTHS, L + 1)}, 0.0, B, cpu)


def test_new_entry_points_are_declared():
    from diffulab_amd import _lib

    protos = _lib.parse_header()
    for name in ("dl_attn_cross_fwd", "dl_attn_cross_bwd", "dl_geglu_fwd", "dl_geglu_bwd", "dl_f32_softmax_keymask_fwd",
                 "dl_f32_geglu_fwd", "dl_f32_geglu_bwd"):
        assert name in protos, name
    assert protos["dl_attn_cross_fwd"][2][5] == "key_bias"
