"""bf16 engines at inner_dim above 1024 (the wide row kernels of csrc/norm.hip): prediction and every parameter gradient against the
CPU oracle, with the tolerances of the existing oracle tests of the same family (test_long_sequence_engines_gpu.py); one wide model
trained and sampled end to end through the public API; the standalone networks.utils.nn.qk_norm_rope at a wide row."""

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
ROPE3 = [20, 22, 22]  # the joint forms' default [dh // 3] * 3 = [21, 21, 21] has odd axis widths, which the engines refuse


def kw_for(D, **extra):
    return dict(input_channels=4, output_channels=4, inner_dim=D, embedding_dim=128, num_heads=D // 64, mlp_ratio=2, patch_size=2,
                **extra)


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
    P["mask_token"] = synth.normal(f"wd.mask{seed}", shapes["mask_token"]) * 0.5
    return P


def joint_inputs(tag, Br, Lr, Cd, gh, gw, lengths):
    x, t = synth.normal(f"{tag}.x", (Br, 4, gh, gw)), synth.uniform(f"{tag}.t", (Br,), lo=0.05, hi=0.95)
    ctx, dy = synth.normal(f"{tag}.ctx", (Br, Lr, Cd)), synth.normal(f"{tag}.dy", (Br, 4, gh, gw))
    keep = torch.arange(Lr)[None, :] < torch.tensor(lengths)[:, None]
    return x, t, ctx, keep, dy


def ctx_embedder(Lr, Cd):
    from diffulab_amd.networks.embedders import PrecomputedEmbedder

    return PrecomputedEmbedder(torch.zeros(1, Lr, Cd), null_embedding_seq_len=5)


def pred_bound(fwd, P, args, po, autocast_floor):
    """1.5e-2, or for a form whose own bf16 error is larger at this width, 1.25 x the oracle's error under CPU bf16 autocast on the
    same inputs (the yardstick of test_full_dims_gpu.py): DDT runs its embeddings at the token width and feeds every encoder token
    into the decoder's modulation, and its oracle alone drifts 1.9e-2 from fp32 at D = 1280 (6.9e-3 at D = 128)"""
    if not autocast_floor:
        return 1.5e-2
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        pa = fwd(P, *args).float()
    return max(1.5e-2, 1.25 * rel(pa, po))


def run_class_conditional(m, P, fwd, kw, tag, Bn, hw, autocast_floor=False):
    m.load_state_dict(P)
    m = m.to(DEV)
    x, t = synth.normal(f"{tag}.x", (Bn, 4, hw, hw)), synth.uniform(f"{tag}.t", (Bn,), lo=0.05, hi=0.95)
    y, dy = synth.integers(f"{tag}.y", (Bn,), 10), synth.normal(f"{tag}.dy", (Bn, 4, hw, hw))
    m.train()
    pred = m(x=x.to(DEV), timesteps=t.to(DEV), y=y.to(DEV), p=0.0)["x"]
    (pred * dy.to(DEV)).sum().backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    po = fwd(Pr, x, t, y)
    assert rel(pred, po) < pred_bound(fwd, P, (x, t, y), po, autocast_floor)
    (po * dy).sum().backward()
    check_grads(m, Pr)


def run_joint(m, P, fwd, tag, Br, Lr, Cd, hw, lengths, autocast_floor=False):
    m.load_state_dict(P)
    m = m.to(DEV)
    x, t, ctx, keep, dy = joint_inputs(tag, Br, Lr, Cd, hw, hw, lengths)
    m.train()
    pred = m(x=x.to(DEV), timesteps=t.to(DEV), initial_context={"embeddings": ctx.to(DEV), "attn_mask": keep.to(DEV)}, p=0.0)["x"]
    (pred * dy.to(DEV)).sum().backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    po = fwd(Pr, x, t, ctx, keep)
    assert rel(pred, po) < pred_bound(fwd, P, (x, t, ctx, keep), po, autocast_floor)
    (po * dy).sum().backward()
    check_grads(m, Pr)


def test_class_conditional_mmdit_1536():
    from diffulab_amd import MMDiT

    kw = kw_for(1536, depth=2, n_classes=10, classifier_free=True)
    cfg = odit.DiTConfig(**kw)
    run_class_conditional(MMDiT(simple_dit=True, **kw), synth.dit_params(odit.param_shapes(cfg), seed=101),
                          lambda P, x, t, y: odit.dit_forward(P, x, t, y, cfg), kw, "wc", 2, 16)


def test_dit_4096():
    """D = 4096, 64 heads, depth 1, mlp_ratio 1, two samples of 8 x 8 tokens"""
    from diffulab_amd import MMDiT

    kw = dict(kw_for(4096, depth=1, n_classes=10, classifier_free=True), mlp_ratio=1)
    cfg = odit.DiTConfig(**kw)
    run_class_conditional(MMDiT(simple_dit=True, **kw), synth.dit_params(odit.param_shapes(cfg), seed=103),
                          lambda P, x, t, y: odit.dit_forward(P, x, t, y, cfg), kw, "w4", 2, 16)


def test_joint_mmdit_1152_padded_context():
    from diffulab_amd import MMDiT

    Lr, Cd = 77, 96
    kw = kw_for(1152, depth=1, rope_axes_dim=ROPE3, rope_base=2000, classifier_free=True)
    m = MMDiT(simple_dit=False, context_embedder=ctx_embedder(Lr, Cd), **kw)
    cfg = ommdit.JointConfig(context_dim=Cd, **kw)
    run_joint(m, synth.dit_params(ommdit.param_shapes(cfg), seed=107), lambda P, x, t, c, k: ommdit.mmdit_forward(P, x, t, c, k, cfg),
              "wj", 2, Lr, Cd, 16, [77, 30])


def test_sprint_2048():
    from diffulab_amd import SprintDiT

    kw = kw_for(2048, encoder_depth=1, deep_layers_depth=1, decoder_depth=1, n_classes=10, classifier_free=True, drop_rate=0.75)
    cfg = osprint.SprintConfig(**kw)
    m = SprintDiT(simple_dit=True, **kw)
    Bn, S = 1, 16 * 16
    scores = synth.uniform("ws.sc", (Bn, S))
    m._draw_scores = lambda B, S_, device: scores.to(device)
    run_class_conditional(m, sprint_params(osprint.param_shapes(cfg), seed=109),
                          lambda P, x, t, y: osprint.sprint_forward(P, x, t, y, cfg, kept=osprint.kept_indices(scores, 64)), kw, "ws", Bn, 32)


def test_joint_sprint_single_stream_1536():
    from diffulab_amd import SprintDiT

    Lr, Cd = 77, 96
    kw = kw_for(1536, encoder_depth=1, deep_layers_depth=2, n_single_stream_blocks=1, decoder_depth=1, rope_axes_dim=ROPE3,
                rope_base=2000, classifier_free=True, drop_rate=0.75)
    kw["patch_size"] = 1
    m = SprintDiT(simple_dit=False, context_embedder=ctx_embedder(Lr, Cd), **kw)
    cfg = osprint.SprintJointConfig(context_dim=Cd, **kw)
    scores = synth.uniform("wsj.sc", (2, 16 * 16))
    m._draw_scores = lambda B, S_, device: scores.to(device)
    run_joint(m, sprint_params(osprint.joint_param_shapes(cfg), seed=113),
              lambda P, x, t, c, k: osprint.sprint_mmdit_forward(P, x, t, c, k, cfg, kept=osprint.kept_indices(scores, 64)),
              "wsj", 2, Lr, Cd, 16, [77, 19])


def test_ddt_1280():
    from diffulab_amd import DDT

    kw = {k: v for k, v in kw_for(1280, encoder_depth=1, decoder_depth=1, n_classes=10, classifier_free=True).items() if k != "embedding_dim"}
    cfg = oddt.DDTConfig(**kw)
    run_class_conditional(DDT(simple_ddt=True, **kw), synth.dit_params(oddt.param_shapes(cfg), seed=127),
                          lambda P, x, t, y: oddt.ddt_forward(P, x, t, y, cfg), kw, "wdd", 2, 16, autocast_floor=True)


def test_joint_ddt_1280():
    from diffulab_amd import DDT

    Lr, Cd = 77, 96
    kw = {k: v for k, v in kw_for(1280, encoder_depth=1, decoder_depth=1, rope_axes_dim=ROPE3, rope_base=1000, classifier_free=True).items()
          if k != "embedding_dim"}
    m = DDT(simple_ddt=False, context_embedder=ctx_embedder(Lr, Cd), **kw)
    cfg = oddt.DDTJointConfig(context_dim=Cd, **kw)
    run_joint(m, synth.dit_params(oddt.joint_param_shapes(cfg), seed=131), lambda P, x, t, c, k: oddt.ddt_joint_forward(P, x, t, c, k, cfg),
              "wdj", 1, Lr, Cd, 16, [50], autocast_floor=True)


def test_wide_model_trains_and_samples_through_the_public_api():
    """a 1152-wide class-conditional MMDiT (18 heads): Diffuser.compute_loss and backward against the oracle's flow loss and
    gradients, a fused AdamW step, then one guided Euler step of Diffuser.generate against the oracle's guided velocity"""
    from diffulab_amd import Diffuser, MMDiT
    from diffulab_amd.training.optim import FusedAdamW

    Bn, g = 4, 2.0
    kw = kw_for(1152, depth=2, n_classes=10, classifier_free=True)
    cfg = odit.DiTConfig(**kw)
    P = synth.dit_params(odit.param_shapes(cfg), seed=137)
    m = MMDiT(simple_dit=True, **kw)
    m.load_state_dict(P)
    m = m.to(DEV)
    x0, noise = synth.normal("we.x0", (Bn, 4, 16, 16)), synth.normal("we.noise", (Bn, 4, 16, 16))
    t, y = synth.uniform("we.t", (Bn,), lo=0.05, hi=0.95), synth.integers("we.y", (Bn,), 10)
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=1)
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    m.train()
    loss = d.compute_loss({"x": x0.to(DEV), "y": y.to(DEV), "p": 0.0}, timesteps=t, noise=noise.to(DEV))["loss"]
    loss.backward()
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    ref = od.flow_loss(odit.dit_forward(Pr, od.flow_add_noise(x0, t, noise), t, y, cfg), x0, noise)
    ref.backward()
    assert abs(loss.item() - ref.item()) / ref.item() < 2e-3, (loss.item(), ref.item())
    check_grads(m, Pr)
    opt.step()
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())
    m.zero_grad(set_to_none=True)
    m.eval()
    P1 = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    xT = synth.normal("we.init", x0.shape)
    with torch.no_grad():
        out = d.generate({"x": xT.to(DEV), "y": y.to(DEV)}, use_tqdm=False, guidance_scale=g)["x"]
        t1 = torch.ones(Bn)
        v_c = odit.dit_forward(P1, xT, t1, y, cfg)
        v_u = odit.dit_forward(P1, xT, t1, torch.full_like(y, 10), cfg)  # the classifier-free null label
    assert bool(torch.isfinite(out).all())
    assert rel(xT.to(DEV) - out, v_u + g * (v_c - v_u)) < 3e-2  # one Euler step from t = 1 to 0: x_0 = x_1 - v


def test_nn_qk_norm_rope_wide():
    """networks.utils.nn.qk_norm_rope at D = 2048 (32 heads) against QKNorm + RotaryPositionalEmbeddingNDim in f32"""
    from diffulab_amd.networks.utils import nn as dnn

    B, gh, gw, H, dh = 2, 8, 8, 32, 64
    N, D = gh * gw, H * dh
    qkv = synth.normal("wnn.qkv", (B * N, 3 * D)).to(DEV, torch.bfloat16).requires_grad_(True)
    qk = dnn.QKNorm(D).to(DEV)
    with torch.no_grad():
        qk.query_norm.scale.copy_(1 + synth.normal("wnn.sq", (D,), std=0.1).to(DEV))
        qk.key_norm.scale.copy_(1 + synth.normal("wnn.sk", (D,), std=0.1).to(DEV))
    pos = torch.stack(torch.meshgrid([torch.arange(gh), torch.arange(gw)], indexing="ij"), dim=-1).view(-1, 2)[None]
    cs = dnn.get_cos_sin_ndim_grid(pos, 10_000.0, [32, 32])
    q, k, v = dnn.qk_norm_rope(qkv, qk, cs, B, N, H)
    wq, wk, wv = (synth.normal(f"wnn.w{i}", (B, H, N, dh)).to(DEV) for i in range(3))
    ((q.float() * wq).sum() + (k.float() * wk).sum() + (v.float() * wv).sum()).backward()
    x = qkv.detach().float().view(B, N, 3 * D).requires_grad_(True)
    qk32 = dnn.QKNorm(D).to(DEV)
    qk32.load_state_dict(qk.state_dict())
    qr, kr = qk32(x[..., :D], x[..., D : 2 * D], x[..., 2 * D :])
    rope = dnn.RotaryPositionalEmbeddingNDim([32, 32])
    cosb, sinb = (c.to(DEV).expand(B, -1, -1) for c in cs)
    qr, kr, vr = rope(qr.view(B, N, H, dh), kr.view(B, N, H, dh), x[..., 2 * D :].view(B, N, H, dh), (cosb, sinb))
    qr, kr, vr = (z.transpose(1, 2) for z in (qr, kr, vr))
    ((qr * wq).sum() + (kr * wk).sum() + (vr * wv).sum()).backward()
    r = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())  # noqa: E731
    assert r(q, qr) < 6e-3 and r(k, kr) < 6e-3 and r(v, vr) < 1e-6
    assert r(qkv.grad, x.grad.view(B * N, 3 * D)) < 1.5e-2
    assert r(qk.query_norm.scale.grad, qk32.query_norm.scale.grad) < 1.5e-2
    assert r(qk.key_norm.scale.grad, qk32.key_norm.scale.grad) < 1.5e-2
