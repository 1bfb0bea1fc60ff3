"""Host-side checks of the joint forms behind a two-output context embedder (pooled embeddings -> ``mlp_pooled_context``) and of the
joint DDT with single-stream encoder blocks: module tree against the reference's (tests/golden/joint_forms.npz), arena layouts,
the reference's assertions and the refusals that stay.  No GPU."""

import json

import pytest
import torch

import joint_forms_common as jc
from oracle import synth


def _classes():
    import diffulab_amd

    return {"MMDiT": diffulab_amd.MMDiT, "SprintDiT": diffulab_amd.SprintDiT, "DDT": diffulab_amd.DDT}


def build(tag, inp=None, **over):
    from diffulab_amd.networks.embedders.common import ContextEmbedder

    cls, kw, pooled, _ = jc.CASES[tag]
    inp = inp or jc.inputs(synth)
    return _classes()[cls](context_embedder=jc.make_embedder(ContextEmbedder, inp, pooled), **dict(kw, **over))


def test_shared_case_definitions_match_the_fixture(golden):
    g = golden("joint_forms")
    assert json.loads(str(g["cases_json"])) == json.loads(jc.cases_json())
    assert tuple(g["mask_lengths"]) == jc.MASK_LENGTHS
    assert tuple(g["shape_b_lc_cctx_cpool"]) == (jc.B, jc.LC, jc.C_CTX, jc.C_POOL)
    assert tuple(g["store_rule"]) == (jc.FULL_BELOW, jc.SAMPLE)


@pytest.mark.parametrize("tag", list(jc.CASES))
def test_state_dict_matches_the_reference_and_every_parameter_has_a_slot(tag, golden):
    g = golden("joint_forms")
    m = build(tag)
    sd = m.state_dict()
    assert list(sd) == [str(n) for n in g[f"{tag}_sd_names"]]  # names AND order: a reference checkpoint loads key for key
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g[f"{tag}_sd_shapes"]]
    assert not list(m.context_embedder.parameters())
    pooled = jc.CASES[tag][2]
    assert m.pooled_embedding is pooled and (m.mlp_pooled_context is not None) is pooled
    if pooled:  # reference widths (mmdit.py:650-657): Linear(pooled width, 2E) -> SiLU -> Linear(2E, E); zero biases, xavier weights
        l0, l2 = m.mlp_pooled_context[0], m.mlp_pooled_context[2]
        assert tuple(l0.weight.shape) == (256, jc.C_POOL) and tuple(l2.weight.shape) == (128, 256)
        assert tuple(m.context_embed.weight.shape) == (128, jc.C_CTX)
        assert float(l0.bias.detach().abs().max()) == 0.0 and float(l0.weight.detach().abs().max()) > 0.0
    m.dims.validate()
    from diffulab_amd import ddt_engine, mmdit_engine, sprint_joint_engine

    d = m.dims
    if isinstance(d, ddt_engine.DDTJointDims):
        lay = ddt_engine.DDTJointLayout(d)
    elif isinstance(d, sprint_joint_engine.SprintJointDims):
        lay = sprint_joint_engine.SprintJointLayout(d)
    elif isinstance(d, sprint_joint_engine.JointStackDims):
        lay = sprint_joint_engine.SprintJointLayout(d, sprint=False)
    else:
        lay = mmdit_engine.JointLayout(d)
    named = dict(m.named_parameters())
    assert set(lay.entries) == set(named)
    spans = sorted((off, off + named[n].numel()) for n, (off, shp) in lay.entries.items() if tuple(shp) == tuple(named[n].shape))
    assert len(spans) == len(named) and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= lay.size
    assert d.pooled_dim == (jc.C_POOL if pooled else 0) and d.context_dim == jc.C_CTX
    # the stacked per-sample adaLN matrix: 12 D rows per joint block, 3 D per single-stream block, contiguous in block order
    D = d.inner_dim
    rows = sum({"J": 12, "S": 3}.get(k, 0) for _, k in d.kinds()) * D if hasattr(d, "kinds") else d.depth * 12 * D
    assert lay.mod_rows == rows + (0 if isinstance(d, ddt_engine.DDTJointDims) else 2 * D)
    off0 = lay.entries[lay.mod_w0][0]
    kinds = d.kinds() if hasattr(d, "kinds") else [(f"layers.{i}.", "J") for i in range(d.depth)]
    for (pre, kind), mo in zip(kinds, lay.mod_off):
        if kind == "S":
            assert lay.entries[pre + "modulation.1.weight"] == (off0 + mo * d.embedding_dim, (3 * D, d.embedding_dim))
        elif kind == "J":
            assert lay.entries[pre + "modulation_input.lin.weight"][0] == off0 + mo * d.embedding_dim
            assert lay.entries[pre + "modulation_context.lin.weight"][0] == off0 + (mo + 6 * D) * d.embedding_dim


@pytest.mark.parametrize("tag", list(jc.CASES))
def test_construction_on_the_meta_device(tag):
    with torch.device("meta"):
        m = build(tag)
    assert all(p.is_meta for p in m.parameters())
    assert len(list(m.parameters())) == len(m.state_dict())


@pytest.mark.parametrize("tag", ["mmdit_d2_p", "sprint_p", "ddt_e3s1_p"])
def test_missing_pooled_embeddings_fire_the_reference_assertion(tag):
    inp = jc.inputs(synth)
    m = build(tag, inp)
    ctx = jc.context_of(inp, pooled=False)
    with pytest.raises(AssertionError, match="pooled embeddings must be in context_output"):
        m(x=inp["x"], timesteps=inp["t"], initial_context=ctx, p=0.0)
    m.mlp_pooled_context = None
    with pytest.raises(AssertionError, match="mlp_pooled_context must be defined"):
        m(x=inp["x"], timesteps=inp["t"], initial_context=jc.context_of(inp, pooled=True), p=0.0)


def test_single_stream_blocks_must_be_fewer_than_the_encoder_depth():
    for ns in (3, 4):
        with pytest.raises(AssertionError, match="n_single_stream_blocks must be less than encoder_depth"):
            build("ddt_e3s1", n_single_stream_blocks=ns)
    m = build("ddt_e3s1", n_single_stream_blocks=2)
    assert [k for _, k in m.dims.kinds()] == ["J", "S", "S", "D"]
    from diffulab_amd.networks.denoisers.mmdit import MMDiTBlock, MMDiTSingleStreamBlock

    assert [type(layer) for layer in m.layers] == [MMDiTBlock, MMDiTSingleStreamBlock, MMDiTSingleStreamBlock]


@pytest.mark.parametrize("tag", ["mmdit_d2_p", "sprint_p", "ddt_e2d1_p"])
def test_a_pooled_width_that_is_no_multiple_of_8_is_refused_by_name(tag):
    from diffulab_amd.networks.embedders.common import ContextEmbedder

    inp = jc.inputs(synth)
    cls, kw, _, _ = jc.CASES[tag]
    emb = jc.embedder_class(ContextEmbedder)(inp["null_ctx"], inp["null_pooled"][:, :44])
    with pytest.raises(NotImplementedError, match="pooled_dim 44"):
        _classes()[cls](context_embedder=emb, **kw)


def test_an_embedder_with_parameters_is_still_refused():
    from diffulab_amd.networks.embedders.common import ContextEmbedder

    inp = jc.inputs(synth)
    emb = jc.make_embedder(ContextEmbedder, inp, True)
    emb.proj = torch.nn.Linear(4, 4)
    with pytest.raises(NotImplementedError, match="parameter-free"):
        _classes()["DDT"](context_embedder=emb, **jc.CASES["ddt_e2d1_p"][1])


@pytest.mark.parametrize("tag", list(jc.CASES))
def test_the_fp32_regime_of_these_forms_still_raises(tag):
    m = build(tag)
    assert m.precisions == ("bf16",)
    with pytest.raises(NotImplementedError, match="no fp32 launch sequence"):
        m.set_precision("fp32")
