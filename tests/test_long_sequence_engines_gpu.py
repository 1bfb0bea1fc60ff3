"""bf16 engines above 2048 attention tokens (the long-sequence attention kernels): prediction and every parameter gradient against
the CPU oracle, with the tolerances of the existing oracle tests of the same family (test_mmdit_joint_gpu.py)."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import ddt as oddt  # noqa: E402
from oracle import diffusion as od  # noqa: E402
from oracle import dit as odit  # noqa: E402
from oracle import mmdit as ommdit  # noqa: E402
from oracle import sprint as osprint  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
KW = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2, depth=1)


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def check_grads(m, Pr):
    bad = []
    for n, p in m.named_parameters():
        if Pr[n].grad is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
        elif rel(p.grad, Pr[n].grad) > (8e-2 if p.dim() == 1 or n == "mask_token" else 4e-2):
            bad.append((n, rel(p.grad, Pr[n].grad)))
    assert not bad, bad


def sprint_params(shapes, seed):
    P = synth.dit_params({k: v for k, v in shapes.items() if k != "mask_token"}, seed=seed)
    P["mask_token"] = synth.normal(f"ls.mask{seed}", shapes["mask_token"]) * 0.5
    return P


def joint_inputs(tag, Br, Lr, Cd, gh, gw, lengths):
    x, t = synth.normal(f"{tag}.x", (Br, 4, gh, gw)), synth.uniform(f"{tag}.t", (Br,), lo=0.05, hi=0.95)
    ctx, dy = synth.normal(f"{tag}.ctx", (Br, Lr, Cd)), synth.normal(f"{tag}.dy", (Br, 4, gh, gw))
    keep = torch.arange(Lr)[None, :] < torch.tensor(lengths)[:, None]
    return x, t, ctx, keep, dy


@pytest.mark.parametrize("gh,gw,Bn", [(48, 48, 2), (48, 44, 1)])
def test_class_conditional_mmdit_above_2048_tokens(gh, gw, Bn):
    """48x48 = 2304 tokens, and 48x44 = 2112 tokens (not a multiple of 256) padded to 2304 with masked pad keys"""
    from diffulab_amd import MMDiT

    kw = dict(KW, n_classes=10, classifier_free=True)
    cfg = odit.DiTConfig(**kw)
    P = synth.dit_params(odit.param_shapes(cfg), seed=21)
    m = MMDiT(simple_dit=True, **kw)
    m.load_state_dict(P)
    m = m.to(DEV)
    x, t = synth.normal("lc.x", (Bn, 4, 2 * gh, 2 * gw)), synth.uniform("lc.t", (Bn,), lo=0.05, hi=0.95)
    y, dy = synth.integers("lc.y", (Bn,), 10), synth.normal("lc.dy", (Bn, 4, 2 * gh, 2 * gw))
    m.train()
    pred = m(x=x.to(DEV), timesteps=t.to(DEV), y=y.to(DEV), p=0.0)["x"]
    (pred * dy.to(DEV)).sum().backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    po = odit.dit_forward(Pr, x, t, y, cfg)
    assert rel(pred, po) < 1.5e-2
    (po * dy).sum().backward()
    check_grads(m, Pr)


@pytest.mark.parametrize("depth,ns", [(1, 0), (2, 1)])
def test_joint_mmdit_ragged_mask_above_2048_tokens(depth, ns):
    """77 context tokens with a ragged attention mask + 48x48 image tokens: 2381 tokens, padded to 2560; joint blocks only, and
    joint then single-stream blocks (the joint stack engine)"""
    from diffulab_amd import MMDiT
    from diffulab_amd.networks.embedders import PrecomputedEmbedder

    Lr, Br, Cd, gh = 77, 2, 96, 48
    kw = dict(KW, rope_axes_dim=[16, 24, 24], rope_base=2000, classifier_free=True, depth=depth, n_single_stream_blocks=ns)
    m = MMDiT(simple_dit=False, context_embedder=PrecomputedEmbedder(torch.zeros(1, Lr, Cd), null_embedding_seq_len=5), **kw)
    cfg = ommdit.JointConfig(context_dim=Cd, **kw)
    P = synth.dit_params(ommdit.param_shapes(cfg), seed=77)
    m.load_state_dict(P)
    m = m.to(DEV)
    x, t = synth.normal("lj.x", (Br, 4, 2 * gh, 2 * gh)), synth.uniform("lj.t", (Br,), lo=0.05, hi=0.95)
    ctx, dy = synth.normal("lj.ctx", (Br, Lr, Cd)), synth.normal("lj.dy", (Br, 4, 2 * gh, 2 * gh))
    keep = torch.arange(Lr)[None, :] < torch.tensor([77, 30])[:, None]
    m.train()
    pred = m(x=x.to(DEV), timesteps=t.to(DEV), initial_context={"embeddings": ctx.to(DEV), "attn_mask": keep.to(DEV)}, p=0.0)["x"]
    (pred * dy.to(DEV)).sum().backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    po = ommdit.mmdit_forward(Pr, x, t, ctx, keep, cfg)
    assert rel(pred, po) < 1.5e-2
    (po * dy).sum().backward()
    check_grads(m, Pr)


def test_sprint_dit_above_2048_tokens():
    """SprintDiT (simple) on a 64x64 token grid with drop rate 0.25: encoder / decoder on 4096 tokens, deep stage on 3072 kept"""
    from diffulab_amd import SprintDiT

    kw = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2, encoder_depth=1,
              deep_layers_depth=1, decoder_depth=1, n_classes=10, classifier_free=True, drop_rate=0.25)
    cfg = osprint.SprintConfig(**kw)
    P = sprint_params(osprint.param_shapes(cfg), seed=31)
    m = SprintDiT(simple_dit=True, **kw)
    m.load_state_dict(P)
    m = m.to(DEV)
    Bn, S = 1, 64 * 64
    x, t = synth.normal("ls.x", (Bn, 4, 128, 128)), synth.uniform("ls.t", (Bn,), lo=0.05, hi=0.95)
    y, dy = synth.integers("ls.y", (Bn,), 10), synth.normal("ls.dy", (Bn, 4, 128, 128))
    scores = synth.uniform("ls.sc", (Bn, S))
    m.train()
    m._draw_scores = lambda B, S_, device: scores.to(device)
    pred = m(x=x.to(DEV), timesteps=t.to(DEV), y=y.to(DEV), p=0.0)["x"]
    (pred * dy.to(DEV)).sum().backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    po = osprint.sprint_forward(Pr, x, t, y, cfg, kept=osprint.kept_indices(scores, 3072))
    assert rel(pred, po) < 1.5e-2
    (po * dy).sum().backward()
    check_grads(m, Pr)


def test_joint_sprint_above_2048_tokens():
    """joint SprintDiT: 77 context tokens (ragged mask) + 48x48 image tokens = 2381 (padded to 2560) in the encoder / decoder, 77 + 576
    kept tokens in the deep stage"""
    from diffulab_amd import SprintDiT
    from diffulab_amd.networks.embedders import PrecomputedEmbedder

    kw = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=1, encoder_depth=1,
              deep_layers_depth=2, n_single_stream_blocks=1, decoder_depth=1, rope_axes_dim=[16, 24, 24], rope_base=2000,
              classifier_free=True, drop_rate=0.75)
    Lr, Br, Cd, gh = 77, 2, 96, 48
    m = SprintDiT(simple_dit=False, context_embedder=PrecomputedEmbedder(torch.zeros(1, Lr, Cd), null_embedding_seq_len=5), **kw)
    cfg = osprint.SprintJointConfig(context_dim=Cd, **kw)
    P = sprint_params(osprint.joint_param_shapes(cfg), seed=37)
    m.load_state_dict(P)
    m = m.to(DEV)
    x, t, ctx, keep, dy = joint_inputs("lsj", Br, Lr, Cd, gh, gh, [77, 19])
    scores = synth.uniform("lsj.sc", (Br, gh * gh))
    m.train()
    m._draw_scores = lambda B, S_, device: scores.to(device)
    pred = m(x=x.to(DEV), timesteps=t.to(DEV), initial_context={"embeddings": ctx.to(DEV), "attn_mask": keep.to(DEV)}, p=0.0)["x"]
    (pred * dy.to(DEV)).sum().backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    po = osprint.sprint_mmdit_forward(Pr, x, t, ctx, keep, cfg, kept=osprint.kept_indices(scores, 576))
    assert rel(pred, po) < 1.5e-2
    (po * dy).sum().backward()
    check_grads(m, Pr)


def test_ddt_above_2048_tokens():
    """DDT (simple) on a 48x48 token grid (2304 tokens): encoder and decoder attention on the long-sequence kernels"""
    from diffulab_amd import DDT

    kw = dict(input_channels=4, output_channels=4, inner_dim=128, num_heads=2, mlp_ratio=4, patch_size=2, encoder_depth=1, decoder_depth=1,
              n_classes=10, classifier_free=True)
    cfg = oddt.DDTConfig(**kw)
    P = synth.dit_params(oddt.param_shapes(cfg), seed=41)
    m = DDT(simple_ddt=True, **kw)
    m.load_state_dict(P)
    m = m.to(DEV)
    Bn = 1
    x, t = synth.normal("ld.x", (Bn, 4, 96, 96)), synth.uniform("ld.t", (Bn,), lo=0.05, hi=0.95)
    y, dy = synth.integers("ld.y", (Bn,), 10), synth.normal("ld.dy", (Bn, 4, 96, 96))
    m.train()
    pred = m(x=x.to(DEV), timesteps=t.to(DEV), y=y.to(DEV), p=0.0)["x"]
    (pred * dy.to(DEV)).sum().backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    po = oddt.ddt_forward(Pr, x, t, y, cfg)
    assert rel(pred, po) < 1.5e-2
    (po * dy).sum().backward()
    check_grads(m, Pr)


def test_joint_ddt_above_2048_tokens():
    """joint DDT: 77 context tokens (ragged mask) + 48x44 image tokens = 2189 (padded to 2304) in the encoder; the decoder attends
    over the 2112 image tokens padded to 2304 with masked pad keys"""
    from diffulab_amd import DDT
    from diffulab_amd.networks.embedders import PrecomputedEmbedder

    kw = dict(input_channels=4, output_channels=4, inner_dim=128, num_heads=2, mlp_ratio=4, patch_size=2, encoder_depth=1, decoder_depth=1,
              rope_axes_dim=[16, 24, 24], rope_base=1000, classifier_free=True)
    Lr, Br, Cd = 77, 1, 96
    m = DDT(simple_ddt=False, context_embedder=PrecomputedEmbedder(torch.zeros(1, Lr, Cd), null_embedding_seq_len=5), **kw)
    cfg = oddt.DDTJointConfig(context_dim=Cd, **kw)
    P = synth.dit_params(oddt.joint_param_shapes(cfg), seed=43)
    m.load_state_dict(P)
    m = m.to(DEV)
    x, t, ctx, keep, dy = joint_inputs("ldj", Br, Lr, Cd, 96, 88, [50])
    m.train()
    pred = m(x=x.to(DEV), timesteps=t.to(DEV), initial_context={"embeddings": ctx.to(DEV), "attn_mask": keep.to(DEV)}, p=0.0)["x"]
    (pred * dy.to(DEV)).sum().backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    po = oddt.ddt_joint_forward(Pr, x, t, ctx, keep, cfg)
    assert rel(pred, po) < 1.5e-2
    (po * dy).sum().backward()
    check_grads(m, Pr)


def test_joint_mmdit_4096_image_tokens_trains_and_samples_through_the_public_api():
    """a joint MMDiT with 64x64 = 4096 image tokens + 77 context tokens (4352 padded): Diffuser.compute_loss and backward against the
    oracle's flow loss and gradients, then one guided Euler step of Diffuser.generate (the inference-graph path, the CFG pair)
    against the oracle's guided velocity: conditional and context-dropped forwards combined with the same guidance scale"""
    from diffulab_amd import Diffuser, MMDiT
    from diffulab_amd.networks.embedders import PrecomputedEmbedder

    Lr, Br, Cd, nl, g = 77, 1, 96, 5, 2.0
    kw = dict(KW, rope_axes_dim=[16, 24, 24], rope_base=2000, classifier_free=True)
    null = synth.normal("lg.null", (1, Lr, Cd)) * 0.5
    m = MMDiT(simple_dit=False, context_embedder=PrecomputedEmbedder(null, null_embedding_seq_len=nl), **kw)
    cfg = ommdit.JointConfig(context_dim=Cd, **kw)
    P = synth.dit_params(ommdit.param_shapes(cfg), seed=47)
    m.load_state_dict(P)
    m = m.to(DEV)
    x0, t, ctx, keep, _ = joint_inputs("lg", Br, Lr, Cd, 128, 128, [60])
    noise = synth.normal("lg.noise", x0.shape)
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=1)
    m.train()
    ic = {"embeddings": ctx.to(DEV), "attn_mask": keep.to(DEV)}
    loss = d.compute_loss({"x": x0.to(DEV), "initial_context": ic, "p": 0.0}, timesteps=t, noise=noise.to(DEV))["loss"]
    loss.backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ref = od.flow_loss(ommdit.mmdit_forward(Pr, od.flow_add_noise(x0, t, noise), t, ctx, keep, cfg), x0, noise)
    ref.backward()
    assert abs(loss.item() - ref.item()) / ref.item() < 2e-3, (loss.item(), ref.item())
    check_grads(m, Pr)
    m.zero_grad(set_to_none=True)
    m.eval()
    xT = synth.normal("lg.init", x0.shape)
    with torch.no_grad():
        out = d.generate({"x": xT.to(DEV), "initial_context": ic}, use_tqdm=False, guidance_scale=g)["x"]
        t1 = torch.ones(Br)
        v_c = ommdit.mmdit_forward(P, xT, t1, ctx, keep, cfg)
        v_u = ommdit.mmdit_forward(P, xT, t1, null.expand(Br, -1, -1), (torch.arange(Lr) < nl)[None].expand(Br, -1), cfg)
    v_ref = v_u + g * (v_c - v_u)
    assert rel(xT.to(DEV) - out, v_ref) < 3e-2  # one Euler step from t = 1 to 0: x_0 = x_1 - v
