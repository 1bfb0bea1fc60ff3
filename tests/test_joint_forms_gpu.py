"""GPU checks of the joint forms with pooled context embeddings (``mlp_pooled_context``) and of the joint DDT with single-stream
encoder blocks, against outputs of the reference (tests/golden/joint_forms.npz, cases and inputs of tests/joint_forms_common.py), and
of the dense-addend conditioning combine kernels through the C ABI.

Parity rule: per tensor, the relative L2 error against the reference's fp32 run is at most 1.5 x the reference's OWN error under
``torch.autocast("cpu", bfloat16)`` on the same step (the fixture's ``ac_*`` figures, measured on the same stored elements), with a
floor of 4e-3 = one bf16 ulp for tensors whose reference error is ~0 (the floor of tests/test_full_dims_gpu.py's yardstick check).
Measured on an MI355X (worst error / bound per case, over the prediction and every gradient): mmdit_d2_p 0.62, mmdit_d3s1_p 0.73,
sprint_p 0.74, ddt_e2d1_p 0.75, ddt_e3s1_p 0.75, ddt_e3s1 0.81, ddt_e3s2 0.76.
"""

import hashlib
import json

import pytest
import torch

import elementwise_bounds as eb
import joint_forms_common as jc
from oracle import synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
FLOOR = 4e-3
_INP: dict = {}


def inputs() -> dict:
    if not _INP:
        _INP.update(jc.inputs(synth))
    return _INP


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def build(tag, g=None, train=True):
    import diffulab_amd
    from diffulab_amd.networks.embedders.common import ContextEmbedder

    cls, kw, pooled, seed = jc.CASES[tag]
    inp = inputs()
    m = getattr(diffulab_amd, cls)(context_embedder=jc.make_embedder(ContextEmbedder, inp, pooled), **kw)
    m.load_state_dict(synth.generic_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=seed))
    m = m.to(DEV)
    if cls == "SprintDiT":
        m._draw_scores = lambda Bn, S, device: inp["scores"].to(device)
    return m.train(train)


def run(m, ctx, p=0.0):
    inp = inputs()
    return m(x=inp["x"].to(DEV), timesteps=inp["t"].to(DEV), initial_context=ctx, p=p)["x"]


# ------------------------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("tag", list(jc.CASES))
def test_prediction_and_every_gradient_against_the_reference(tag, golden):
    g = {k[len(tag) + 1:]: v for k, v in golden("joint_forms").items() if k.startswith(tag + "_")}
    pooled = jc.CASES[tag][2]
    inp = inputs()
    m = build(tag)
    pred = run(m, jc.context_of(inp, pooled, DEV))
    (pred * inp["g"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    ratios = [(rel(pred, g["pred"]) / (1.5 * max(float(g["ac_pred_err"]), FLOOR)), "prediction")]
    names = [str(n) for n in g["names"]]
    named = dict(m.named_parameters())
    assert list(named) == names
    gmax = float(g["grad_norms"].max())
    checked = set()
    for n, norm, ac in zip(names, g["grad_norms"].tolist(), g["ac_err"].tolist()):
        got = named[n].grad
        if norm <= 1e-6 * gmax:  # no gradient in the reference (context half of the last joint block): exact zeros here
            assert float(got.abs().max()) == 0.0, n
            continue
        bound = 1.5 * max(ac, FLOOR)
        ratios.append((rel(jc.stored(got), g["g_" + n]) / bound, n))
        ratios.append((abs(float(got.double().norm()) - norm) / norm / bound, n + " (norm)"))
        checked.add(n)
    ratios.sort(reverse=True)
    print(f"{tag}: worst error / bound {ratios[0][0]:.3f} ({ratios[0][1]}); prediction {rel(pred, g['pred']):.2e} (reference under bf16 "
          f"autocast {float(g['ac_pred_err']):.2e}); next: {[(round(r, 3), n) for r, n in ratios[1:4]]}")
    # the new pieces by name: non-zero in the reference, and among the tensors held to the bound
    new = [n for n in names if n.startswith("mlp_pooled_context.")]
    new += [n for n in names for pre, kind in (m.dims.kinds() if hasattr(m.dims, "kinds") else ()) if kind == "S" and n.startswith(pre)]
    assert len([n for n in new if n.startswith("mlp_pooled_context.")]) == (4 if pooled else 0)
    assert len(new) == (4 if pooled else 0) + 10 * getattr(m.dims, "n_single_stream_blocks", 0)
    assert all(n in checked for n in new), [n for n in new if n not in checked]
    assert ratios[0][0] <= 1.0, ratios[:8]


# ------------------------------------------------------------------------------------------------------------------ combine kernels
class _Window:
    """a contiguous [B, E] window inside a poisoned 1-D allocation, 64 guard words before and after"""

    def __init__(self, B, E, dtype):
        self.buf = eb.poison_(torch.empty(64 + B * E + 64, dtype=dtype, device=DEV))
        self.win = self.buf[64 : 64 + B * E].view(B, E)

    def check(self, what):
        n = self.win.numel()
        assert bool(eb.is_poison(self.buf[:64]).all()) and bool(eb.is_poison(self.buf[64 + n :]).all()), f"{what}: guard words written"
        assert bool(torch.isfinite(self.win.float()).all()), f"{what}: window not finite"


def _dsilu(x):
    """(silu'(x), bound of the device's s * (1 + x * (1 - s)), s = rcp(1 + exp(-x))) for exact f32 inputs x (fp64 here): the
    sigmoid carries the relative error r of elementwise_bounds.silu_dev_rel; it enters through s and through (1 - s), whose absolute
    error is r s; each of the four f32 operations rounds a magnitude of at most s (1 + |x|)"""
    s = torch.sigmoid(x)
    r = eb.silu_dev_rel(x)
    d = s * (1 + x * (1 - s))
    return d, r * s * (1 + x.abs() * (1 - s)) + s * x.abs() * r * s + 4 * eb.U32 * s * (1 + x.abs()) + 2.0**-126


@pytest.mark.parametrize("B", [1, 2, 64, 65])
@pytest.mark.parametrize("E", [64, 128, 4096])
def test_dense_cond_combine_kernels(B, E):
    from diffulab_amd import ops

    e, pe = (synth.normal(f"cc.{n}.{B}.{E}", (B, E)).mul(s).to(DEV) for n, s in (("e", 2.0), ("pe", 3.0)))
    dact = synth.normal(f"cc.d.{B}.{E}", (B, E)).to(DEV)
    outs = []
    for _ in range(2):
        emb, act = _Window(B, E, torch.float32), _Window(B, E, torch.bfloat16)
        ops.cond_combine_dense_fwd(e, pe, emb.win, act.win)
        demb, demb16 = _Window(B, E, torch.float32), _Window(B, E, torch.bfloat16)
        ops.cond_combine_dense_bwd(dact, emb.win, demb.win, demb16.win)
        torch.cuda.synchronize()
        for w, what in ((emb, "emb"), (act, "act"), (demb, "demb"), (demb16, "demb16")):
            w.check(f"dense combine B={B} E={E}: {what}")
        outs.append((emb.win.clone(), act.win.clone(), demb.win.clone(), demb16.win.clone()))
    for a, b in zip(*outs):  # two runs are bit-identical
        assert torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32),
                           b.view(torch.int16 if b.element_size() == 2 else torch.int32))
    emb, act, demb, demb16 = outs[0]
    assert torch.equal(emb, e + pe)  # one f32 addition: exact against torch's
    v = emb.double()
    s, es = eb.silu(v, torch.zeros_like(v))
    eb.assert_within(act, s, eb.store_bf16(s, es), what=f"act B={B} E={E}")
    d, ed = _dsilu(v)
    gref = dact.double() * d
    eg = dact.double().abs() * ed + eb.U32 * gref.abs()
    eb.assert_within(demb, gref, eb.store_f32(gref, eg), what=f"demb B={B} E={E}")
    eb.assert_within(demb16, gref, eb.store_bf16(gref, eg), what=f"demb16 B={B} E={E}")
    # the bf16 copy is the rounding of the f32 copy, not a second computation
    assert torch.equal(demb16, demb.to(torch.bfloat16))


def test_dense_cond_combine_refuses_what_it_cannot_address():
    from diffulab_amd import ops

    e = torch.zeros(2, 66, device=DEV)
    with pytest.raises(RuntimeError, match="dl_cond_combine_dense_fwd"):
        ops.cond_combine_dense_fwd(e, e, torch.empty_like(e), torch.empty(2, 66, device=DEV, dtype=torch.bfloat16))


# ------------------------------------------------------------------------------------------------------------------ guidance, replay
@pytest.mark.parametrize("tag", ["mmdit_d2_p", "mmdit_d3s1_p", "ddt_e2d1_p", "ddt_e3s1_p", "ddt_e3s2"])
def test_every_sample_dropped_equals_the_null_triple_passed_directly(tag):
    """(not SprintDiT: there p is also the probability of dropping the deep path, sprint.py:384 -- at p = 1 the deep layers are skipped,
    in the reference too, so the two forwards differ by more than their context)"""
    pooled = jc.CASES[tag][2]
    inp = inputs()
    m = build(tag, train=False)
    with torch.no_grad():
        dropped = run(m, jc.context_of(inp, pooled, DEV), p=1.0).clone()
        direct = run(m, jc.null_context(inp, pooled, DEV), p=0.0).clone()
        cond = run(m, jc.context_of(inp, pooled, DEV), p=0.0).clone()
    assert torch.equal(dropped, direct)
    assert not torch.equal(cond, direct)


@pytest.mark.parametrize("tag", ["mmdit_d2_p", "sprint_p", "ddt_e3s1_p"])
def test_graph_replay_reads_the_pooled_vector_of_the_call(tag, monkeypatch):
    """eval mode: the second and third calls replay the captured hipGraph; each is given a DIFFERENT pooled vector and must equal the
    eager result for that vector bit for bit (a pooled tensor baked into the capture would repeat the first call's)"""
    inp = inputs()
    base = jc.context_of(inp, True, DEV)
    pools = [base["pooled_embeddings"], base["pooled_embeddings"].flip(0) * 1.5, base["pooled_embeddings"] - 0.75]
    monkeypatch.setenv("DL_HIPGRAPH", "0")
    eager_m = build(tag, train=False)
    with torch.no_grad():
        eager = [run(eager_m, dict(base, pooled_embeddings=p)).clone() for p in pools]
    assert not torch.equal(eager[0], eager[1]) and not torch.equal(eager[1], eager[2])
    monkeypatch.setenv("DL_HIPGRAPH", "1")
    m = build(tag, train=False)
    with torch.no_grad():
        got = [run(m, dict(base, pooled_embeddings=p)).clone() for p in pools]
    graphs = m.__dict__.get("_graphs")
    assert graphs and all(v is not False for v in graphs.values()) and len(graphs) == 1  # captured once, replayed twice
    for a, b in zip(got, eager):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------------ training step
@pytest.mark.parametrize("tag", ["mmdit_d3s1_p", "ddt_e3s1_p"])
def test_training_step_repeats(tag):
    """forward, backward and one AdamW step twice from the same state.  The parent joint forms assert no bit-identity of a step:
    the blocks' weight gradients and LayerNorm column sums meet through f32 atomics whose order varies (tests/test_trainer_gpu.py
    holds two such backwards to a relative 1e-4), so that spread is the rule here; the prediction of the same state is bit-identical,
    and the pooled MLP's gradients -- deterministic small GEMMs and column sums from a bit-identical-or-not demb -- stay inside it"""
    from diffulab_amd.training import FusedAdamW

    pooled = jc.CASES[tag][2]
    inp = inputs()
    res = []
    for _ in range(2):
        m = build(tag)
        opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
        opt.zero_grad()
        pred = run(m, jc.context_of(inp, pooled, DEV))
        (pred * inp["g"].to(DEV)).sum().backward()
        grads = m._flat_grad.clone()
        opt.step()
        torch.cuda.synchronize()
        res.append((pred.detach().clone(), grads, m._flat.clone(), {n: p.grad.clone() for n, p in m.named_parameters()}))
    a, b = res
    assert torch.equal(a[0], b[0])
    assert rel(a[1], b[1]) < 1e-4 and rel(a[2], b[2]) < 1e-4
    for n in a[3]:
        if n.startswith("mlp_pooled_context."):
            assert rel(a[3][n], b[3][n]) < 1e-4 and float(a[3][n].abs().max()) > 0, n


# ------------------------------------------------------------------------------------------------------------------ existing forms
# recorded on the parent commit for the joint DDT below (one-output embedder, n_single_stream_blocks = 0, B = 2, 64 + 12 tokens):
PARENT_DDT_LAYOUT_SHA256 = "41d43bda0df70dbcfe09016768c16e9007eb9fb2d09dac9266b6df67ee0c4f68"
PARENT_DDT_LAYOUT_SIZE = 1683008
PARENT_DDT_LAUNCHES = (173, "79f903c6152435cb4b11e4dc7f93ba827c95d2bb4afede9f3c17ec9f8d5d2e74")  # (C calls of one step, sha256 of their names)


def _launch_names(plan) -> list[str]:
    return [getattr(fn, "__name__", "host") for fn, _ in plan.calls]


def test_existing_joint_ddt_keeps_the_parent_layout_and_launch_list():
    from diffulab_amd import DDT, ops
    from diffulab_amd.networks.embedders.common import ContextEmbedder

    inp = inputs()
    kw = dict(jc.CASES["ddt_e2d1_p"][1], decoder_depth=2, mlp_ratio=2)
    m = DDT(context_embedder=jc.make_embedder(ContextEmbedder, inp, False), **kw)
    m.load_state_dict(synth.generic_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=301))
    m = m.to(DEV).train()
    lay = m.engine.layout
    digest = hashlib.sha256(json.dumps([[n, o, list(s)] for n, (o, s) in lay.entries.items()]).encode()).hexdigest()
    assert (digest, lay.size) == (PARENT_DDT_LAYOUT_SHA256, PARENT_DDT_LAYOUT_SIZE)
    run(m, jc.context_of(inp, False, DEV)).sum().backward()  # allocates the workspace: the recorded pass below is the steady state
    plan = ops.LaunchPlan()
    with ops.recording(plan):
        pred = run(m, jc.context_of(inp, False, DEV))
        pred.sum().backward()
    torch.cuda.synchronize()
    names = _launch_names(plan)
    print("joint DDT launch list:", len(names), hashlib.sha256("\n".join(names).encode()).hexdigest())
    assert (len(names), hashlib.sha256("\n".join(names).encode()).hexdigest()) == PARENT_DDT_LAUNCHES
