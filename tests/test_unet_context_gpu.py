"""Text-conditioned UNetModel on the GPU: the masked cross-attention core (dl_attn_cross_*), the f32 masked softmax and the GEGLU
forms against torch float64; the model in both regimes against the reference fixture (tests/golden/unet_context.npz); the bf16
regime against the fp32 regime at configs/model/unet.yaml dims; launch-plan and hipGraph replays with changing contexts; training,
EMA, checkpoints and sampling."""

import copy
import os

import numpy as np
import pytest
import torch

from oracle import synth
from unet_context_common import B, C_CTX, CASES, L, MASK_LENGTHS, TIMESTEPS, ChannelFirstEmbedder, mask_of

pytestmark = pytest.mark.gpu
DEV = "cuda"


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _bias(lengths, L):
    keep = mask_of(lengths, L)
    return torch.zeros(keep.shape).masked_fill_(~keep, float("-inf"))


def _ref_attn(q, k, v, bias, Bn, Nq, Lk, H, dh, dout):
    """float64 autograd reference: q [B*Nq, H*dh], k / v [B*L, H*dh]; rows whose keys are all masked give zeros (SDPA on CPU)"""
    q, k, v = (t.double().requires_grad_(True) for t in (q, k, v))
    qh = q.view(Bn, Nq, H, dh).transpose(1, 2)
    kh, vh = k.view(Bn, Lk, H, dh).transpose(1, 2), v.view(Bn, Lk, H, dh).transpose(1, 2)
    live = torch.isfinite(bias).any(-1)  # (a sample with every key masked: zeros, and no NaN through the float64 backward)
    safe = torch.where(live[:, None], bias, torch.zeros_like(bias)).double()
    s = qh @ kh.transpose(-1, -2) * dh ** -0.5 + safe[:, None, None, :]
    p = torch.softmax(s, -1) * live.double()[:, None, None, None]
    o = (p @ vh).transpose(1, 2).reshape(Bn * Nq, H * dh)
    (o * dout.double()).sum().backward()
    return o.detach(), q.grad, k.grad, v.grad


# MFMA kernels: dh % 64 == 0 and Nq <= 64; VALU kernels: the other shapes ((64, 20, 4, 32), (80, 30, 2, 64), (16, 40, 2, 40))
@pytest.mark.parametrize("Nq,Lk,H,dh", [(64, 77, 2, 256), (16, 256, 2, 512), (64, 20, 4, 32), (4, 1, 1, 64), (64, 512, 8, 64),
                                        (33, 130, 2, 128), (80, 30, 2, 64), (16, 40, 2, 40)])
def test_attn_cross_kernel_against_float64(Nq, Lk, H, dh):
    from diffulab_amd import ops

    Bn, c = 3, H * dh
    lengths = (Lk, max(1, (Lk + 2) // 3), 0)  # full, ragged, all masked
    g = torch.Generator().manual_seed(Nq * 7 + Lk + dh)
    q = torch.randn(Bn * Nq, c, generator=g).bfloat16()
    kv = torch.randn(Bn * Lk, 2 * c, generator=g).bfloat16()
    dout = torch.randn(Bn * Nq, c, generator=g).bfloat16()
    bias = _bias(lengths, Lk)

    def run(kv_host):
        qd, kvd, dod, bd = q.to(DEV), kv_host.to(DEV), dout.to(DEV), bias.to(DEV)
        out = torch.empty(Bn * Nq, c, device=DEV, dtype=torch.bfloat16)
        probs = torch.empty(Bn, H, Nq, Lk, device=DEV)
        ops.attn_cross_fwd(qd, kvd[:, :c], kvd[:, c:], bd, out, probs, Bn, Nq, Lk, H, dh)
        dq, dkv = torch.empty_like(qd), torch.empty_like(kvd)
        ds = torch.empty(Bn, H, Nq, Lk, device=DEV)
        ops.attn_cross_bwd(qd, kvd[:, :c], kvd[:, c:], bd, dod, probs, ds, dq, dkv[:, :c], dkv[:, c:], Bn, Nq, Lk, H, dh)
        torch.cuda.synchronize()
        return out.cpu(), dq.cpu(), dkv.cpu()

    out, dq, dkv = run(kv)
    o_r, dq_r, dk_r, dv_r = _ref_attn(q, kv[:, :c], kv[:, c:], bias, Bn, Nq, Lk, H, dh, dout)
    assert rel(out, o_r) < 1e-2 and rel(dq, dq_r) < 1e-2
    assert rel(dkv[:, :c], dk_r) < 1e-2 and rel(dkv[:, c:], dv_r) < 1e-2
    # the all-masked sample: exactly zero output and gradients
    assert not out[2 * Nq:].float().abs().max() and not dq[2 * Nq:].float().abs().max() and not dkv[2 * Lk:].float().abs().max()
    # K / V rows behind the mask contribute exact zeros: changing them leaves every output bit-identical
    kv2 = kv.clone()
    for b, n in enumerate(lengths):
        kv2[b * Lk + n:(b + 1) * Lk] = torch.randn((Lk - n), 2 * c, generator=g).bfloat16()
    out2, dq2, dkv2 = run(kv2)
    assert torch.equal(out, out2) and torch.equal(dq, dq2) and torch.equal(dkv, dkv2)


@pytest.mark.parametrize("Nq,Lk,H,dh", [(16, 20, 2, 32), (256, 77, 2, 64), (9, 5, 1, 24)])
def test_f32_masked_cross_attention_against_float64(Nq, Lk, H, dh):
    """the fp32 regime's (and the bf16 fallback's) cross-attention: batched dl_f32_gemm + dl_f32_softmax_keymask_fwd"""
    from diffulab_amd import ops

    Bn, c = 3, H * dh
    lengths = (Lk, max(1, Lk // 2), 0)
    g = torch.Generator().manual_seed(Nq + Lk)
    q, kv, dout = torch.randn(Bn * Nq, c, generator=g), torch.randn(Bn * Lk, 2 * c, generator=g), torch.randn(Bn * Nq, c, generator=g)
    bias = _bias(lengths, Lk)
    qd, kvd, dod, bd = q.to(DEV), kv.to(DEV), dout.to(DEV), bias.to(DEV)
    out, probs = torch.empty(Bn * Nq, c, device=DEV), torch.empty(Bn, H, Nq, Lk, device=DEV)
    ops.f32_xattn_fwd(qd, kvd[:, :c], kvd[:, c:], bd, out, probs, Bn, Nq, Lk, H, dh)
    dq, dkv, dP = torch.empty_like(qd), torch.empty_like(kvd), torch.empty(Bn, H, Nq, Lk, device=DEV)
    ops.f32_xattn_bwd(qd, kvd[:, :c], kvd[:, c:], dod, probs, dP, dq, dkv[:, :c], dkv[:, c:], Bn, Nq, Lk, H, dh)
    o_r, dq_r, dk_r, dv_r = _ref_attn(q, kv[:, :c], kv[:, c:], bias, Bn, Nq, Lk, H, dh, dout)
    assert rel(out, o_r) < 2e-6 and rel(dq, dq_r) < 5e-6 and rel(dkv[:, :c], dk_r) < 5e-6 and rel(dkv[:, c:], dv_r) < 5e-6
    assert not probs[2].abs().max() and not out[2 * Nq:].abs().max()


@pytest.mark.parametrize("M,F", [(80, 128), (64 * 16, 2048), (7, 8)])
def test_geglu_bf16_and_f32(M, F):
    from diffulab_amd import ops

    g = torch.Generator().manual_seed(M + F)
    u, dh = torch.randn(M, 2 * F, generator=g) * 2, torch.randn(M, F, generator=g)
    ur = u.double().requires_grad_(True)
    h_r = ur[:, :F] * torch.nn.functional.gelu(ur[:, F:])
    (h_r * dh.double()).sum().backward()
    h, du = torch.empty(M, F, device=DEV), torch.empty(M, 2 * F, device=DEV)
    ops.f32_geglu_fwd(u.to(DEV), h)
    ops.f32_geglu_bwd(dh.to(DEV), u.to(DEV), du)
    assert rel(h, h_r) < 2e-6 and rel(du, ur.grad) < 5e-6
    ub, dhb = u.bfloat16(), dh.bfloat16()
    ur = ub.double().requires_grad_(True)
    h_r = ur[:, :F] * torch.nn.functional.gelu(ur[:, F:])
    (h_r * dhb.double()).sum().backward()
    h16, du16 = torch.empty(M, F, device=DEV, dtype=torch.bfloat16), torch.empty(M, 2 * F, device=DEV, dtype=torch.bfloat16)
    ops.geglu_fwd(ub.to(DEV), h16)
    ops.geglu_bwd(dhb.to(DEV), ub.to(DEV), du16)
    assert rel(h16, h_r) < 8e-3 and rel(du16, ur.grad) < 8e-3


# ------------------------------------------------------------------ the model against the reference fixture
def _fixture_inputs():
    emb = synth.normal("uc.ctx", (B, C_CTX, L))
    ctx = {"embeddings": emb.to(DEV), "attn_mask": mask_of(MASK_LENGTHS, L).to(DEV)}
    x0, noise = synth.normal("uc.x0", (B, 3, 16, 16)), synth.normal("uc.noise", (B, 3, 16, 16))
    return ctx, x0.to(DEV), noise.to(DEV), torch.tensor(TIMESTEPS, dtype=torch.int32)


def _fixture_model(tag, precision):
    from diffulab_amd.networks.denoisers import UNetModel

    m = UNetModel(context_embedder=ChannelFirstEmbedder(C_CTX), **CASES[tag])
    m.load_state_dict(synth.generic_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=61))
    return m.set_precision(precision).to(DEV)


@pytest.mark.parametrize("tag", list(CASES))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_context_unet_against_reference_fixture(golden, tag, precision):
    from diffulab_amd import Diffuser
    from oracle import diffusion as od

    g = golden("unet_context")
    m = _fixture_model(tag, precision)
    ctx, x0, noise, ti = _fixture_inputs()
    T = od.GaussianTables(1000)
    xt = od.ddpm_add_noise(T, x0.cpu(), ti, noise.cpu())
    with torch.no_grad():
        pred = m(x=xt.to(DEV), timesteps=ti.to(DEV), context=ctx)["x"]
    gd = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    loss = gd.compute_loss({"x": x0, "context": ctx, "p": 0.0}, timesteps=ti.to(DEV), noise=noise)["loss"]
    loss.backward()
    names, norms = g[f"{tag}_names"].tolist(), g[f"{tag}_grad_norms"]
    named = dict(m.named_parameters())
    e_pred, e_loss = rel(pred, g[f"{tag}_pred"]), abs(loss.item() - float(g[f"{tag}_loss"])) / float(g[f"{tag}_loss"])
    # "d2" (two Transformer layers per block on these random weights) amplifies round-off: the reference's own autocast error there is
    # ~10x that of "d1" (0.29 vs 0.05 median per gradient tensor), and its gradient bars scale with it
    chaotic = tag == "d2"
    if precision == "fp32":
        # (test_unet_fp32_gpu.py asks 2e-5 per gradient tensor of a network without Transformer blocks; here 3e-5 -- 1e-4 for "d2",
        #  whose amplification the paragraph above describes -- with that test's floor: conv biases in front of a GroupNorm have an
        #  exactly-zero gradient, f32 round-off here)
        tol = 1e-4 if chaotic else 3e-5
        assert e_pred < 1e-5 and e_loss < 1e-5, (e_pred, e_loss)
        floor = 1e-6 * norms.max()
        for i, n in enumerate(names):
            got = named[n].grad.double().norm().item()
            if norms[i] <= floor:
                assert got <= 1e-4 * norms.max(), n
            elif f"{tag}_g_{n}" in g:
                assert rel(named[n].grad, g[f"{tag}_g_{n}"]) < tol, n
            else:
                assert abs(got - norms[i]) <= tol * norms[i], n
        return
    # bf16 regime: within 1.5x of the reference's own autocast error per tensor; gradients near zero get the floor of
    # test_small_unet_ddpm_loss_and_grads (conv biases in front of a GroupNorm: exactly zero in exact arithmetic), 1-D gradients
    # (biases / norm gains: signed sums over every token, with heavy cancellation) an absolute 5e-2 on top (1e-1 for "d2"), as there
    assert e_pred <= 1.5 * float(g[f"{tag}_ac_pred_err"]) + 2e-3, (e_pred, float(g[f"{tag}_ac_pred_err"]))
    ac = g[f"{tag}_ac_err"]
    floor = 1e-3 * norms.max()
    for i, n in enumerate(names):
        got = named[n].grad.double().norm().item()
        if norms[i] <= floor:
            assert got <= 30 * floor, n
        elif f"{tag}_g_{n}" in g:
            extra = (1e-1 if chaotic else 5e-2) if named[n].dim() == 1 else 1e-2
            assert rel(named[n].grad, g[f"{tag}_g_{n}"]) <= 1.5 * ac[i] + extra, (n, ac[i])
        else:
            assert abs(got - norms[i]) / norms[i] <= 1.5 * ac[i] + 1e-2, (n, ac[i])


# ------------------------------------------------------------------ at scale: bf16 regime against the port's fp32 regime
@pytest.mark.parametrize("dims", ["config1", "attn16"])
def test_context_unet_bf16_against_fp32_at_scale(dims):
    """configs/model/unet.yaml dims without n_classes, C_ctx = 768, L = 77, ragged masks, B = 4 (every cross-attention on the HIP core:
    Nq = 64 / 16, dh = 256 / 512); "attn16": attention at 16 x 16 (Nq = 256: the f32 fallback of the bf16 regime).
    Bound: prediction 5e-2, loss 2e-2, median per-tensor gradient error 5e-2 and EVERY tensor's within 1e-1 (bf16 activations through
    ~40 stages; measured: median 1.0-1.5e-2, max 3.2e-2)."""
    from diffulab_amd import Diffuser
    from diffulab_amd.networks.denoisers import UNetModel

    kw = dict(image_size=[32, 32], in_channels=1, model_channels=128, out_channels=1, num_res_blocks=2, attention_resolutions=[4, 8, 16],
              num_heads=2, resblock_updown=True, use_scale_shift_norm=True)
    if dims == "attn16":
        kw.update(model_channels=64, channel_mult="1, 2", num_res_blocks=1, attention_resolutions=[2])
    Bn, Lk, cc = 4, 77, 768
    ctx = {"embeddings": synth.normal("ucs.ctx", (Bn, cc, Lk)).to(DEV), "attn_mask": mask_of((77, 30, 5, 1), Lk).to(DEV)}
    x0, noise = synth.normal("ucs.x0", (Bn, 1, 32, 32)).to(DEV), synth.normal("ucs.noise", (Bn, 1, 32, 32)).to(DEV)
    ti = torch.tensor([10, 400, 800, 999], dtype=torch.int32).to(DEV)
    res = {}
    for precision in ("fp32", "bf16"):
        m = UNetModel(context_embedder=ChannelFirstEmbedder(cc), **kw)
        m.load_state_dict(synth.generic_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed=71))
        m = m.set_precision(precision).to(DEV)
        gd = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
        with torch.no_grad():
            xt = gd.diffusion.add_noise(x0, ti, noise)[0]
            pred = m(x=xt, timesteps=ti, context=ctx)["x"].cpu()
        loss = gd.compute_loss({"x": x0, "context": ctx, "p": 0.0}, timesteps=ti, noise=noise)["loss"]
        loss.backward()
        res[precision] = (pred, loss.item(), {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters()})
        del m, gd
        torch.cuda.empty_cache()
    f, b = res["fp32"], res["bf16"]
    norms = {n: g.double().norm().item() for n, g in f[2].items()}
    big = max(norms.values())
    errs = {n: rel(b[2][n], f[2][n]) for n in f[2] if norms[n] > 1e-3 * big}
    worst = max(errs, key=errs.get)
    assert any("cross_attn.norm_context" in n for n in errs) and any("cross_attn.to_kv" in n for n in errs)
    errs = list(errs.values())
    e_pred, e_loss = rel(b[0], f[0]), abs(b[1] - f[1]) / f[1]
    print(f"context UNet {dims}: bf16 vs fp32 prediction {e_pred:.3e} loss {e_loss:.3e} gradients median {np.median(errs):.3e} "
          f"max {max(errs):.3e}")
    assert torch.isfinite(b[0]).all() and all(torch.isfinite(g).all() for g in b[2].values())
    assert e_pred < 5e-2 and e_loss < 2e-2 and float(np.median(errs)) < 5e-2
    assert max(errs) < 1e-1, worst


# ------------------------------------------------------------------ replays
def test_launch_plan_replay_with_changing_contexts():
    """three training steps with DL_LAUNCH_PLAN=1 (eager, recorded, replayed) with different contexts and masks against the same
    steps with DL_LAUNCH_PLAN=0.  The forward has no atomics: the predictions must be bit-identical, which a replay that read a stale
    context would not be.  The backward differs by the order of the f32 atomics left in the bf16 regime's reductions (measured
    0.07-5e-3 relative on the whole gradient arena, eager against eager as well): fixed bound 2e-2, where a skipped launch is O(1)."""
    from diffulab_amd import Diffuser

    steps = []
    for s in range(3):
        lengths = ((20, 7, 1, 0), (3, 20, 12, 5), (0, 1, 19, 20))[s]
        steps.append(({"embeddings": synth.normal(f"ucp.ctx{s}", (B, C_CTX, L)).to(DEV), "attn_mask": mask_of(lengths, L).to(DEV)},
                      synth.normal(f"ucp.x{s}", (B, 3, 16, 16)).to(DEV), synth.normal(f"ucp.n{s}", (B, 3, 16, 16)).to(DEV),
                      torch.tensor([5, 100 * s + 50, 700, 999 - s], dtype=torch.int32).to(DEV)))

    def run(plans):
        os.environ["DL_LAUNCH_PLAN"] = "1" if plans else "0"
        try:
            m = _fixture_model("d1", "bf16")
            gd = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
            out = []
            for ctx, x0, noise, ti in steps:
                m.zero_grad()
                xt = gd.diffusion.add_noise(x0, ti, noise)[0]
                pred = m(x=xt, timesteps=ti, context=ctx)["x"]
                ((pred - noise) ** 2).mean().backward()
                out.append((pred.detach().clone(), m._flat_grad.clone()))
            made = [v for v in m.engine.__dict__.get("_launch_plans", {}).values() if not isinstance(v, (int, bool))]
            return out, made
        finally:
            os.environ.pop("DL_LAUNCH_PLAN", None)

    on, made = run(True)
    off, none = run(False)
    assert len(made) == 1 and made[0].bwd is not None and not none
    for s, ((p1, g1), (p0, g0)) in enumerate(zip(on, off)):
        print(f"step {s}: gradients plan vs eager {rel(g1, g0):.3e}")
        assert torch.equal(p1, p0), s
        assert rel(g1, g0) < 2e-2, s
    assert not torch.equal(on[2][0], on[1][0])  # (different contexts: different predictions)


def test_hipgraph_inference_replay_reads_the_new_context():
    m = _fixture_model("d1", "bf16")
    m.eval()
    _, x0, _, ti = _fixture_inputs()
    ctxs = [{"embeddings": synth.normal(f"ucg.ctx{s}", (B, C_CTX, L)).to(DEV), "attn_mask": mask_of(((20, 7, 1, 0), (5, 20, 2, 9))[s], L).to(DEV)}
            for s in range(2)]
    outs = {}
    for graph in ("1", "0"):
        os.environ["DL_HIPGRAPH"] = graph
        try:
            with torch.inference_mode():
                outs[graph] = [m(x=x0, timesteps=ti.to(DEV), context=c)["x"].clone() for c in ctxs + ctxs]
        finally:
            os.environ.pop("DL_HIPGRAPH", None)
    assert any(v for v in m.__dict__.get("_graphs", {}).values())  # a graph was captured and replayed
    for a, b in zip(outs["1"], outs["0"]):
        assert torch.equal(a, b)
    assert not torch.equal(outs["1"][0], outs["1"][1]) and torch.equal(outs["1"][0], outs["1"][2])


# ------------------------------------------------------------------ training and sampling
def test_training_ema_checkpoint_and_sampling():
    from diffulab_amd import Diffuser
    from diffulab_amd.training.ema import EMA
    from diffulab_amd.training.optim import FusedAdamW

    m = _fixture_model("dflt", "bf16")
    ctx, x0, noise, ti = _fixture_inputs()
    gd = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    opt = FusedAdamW(m.parameters(), lr=3e-4)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        loss = gd.compute_loss({"x": x0, "context": ctx, "p": 0.0}, timesteps=ti.to(DEV), noise=noise)["loss"]
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    ema = EMA(m, beta=0.9, update_after_step=0, update_every=1)
    ema.update()
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    m2 = _fixture_model("dflt", "bf16")
    m2.load_state_dict(sd)
    with torch.no_grad():
        a = m(x=x0, timesteps=ti.to(DEV), context=ctx)["x"]
        b = m2(x=x0, timesteps=ti.to(DEV), context=ctx)["x"]
        c = ema.ema_model(x=x0, timesteps=ti.to(DEV), context=ctx)["x"]
    assert torch.equal(a, b) and torch.isfinite(c).all()
    gs = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    with torch.no_grad():
        out = gs.generate({"x": noise, "context": ctx}, use_tqdm=False)["x"]
    assert out.shape == noise.shape and torch.isfinite(out).all()
    with pytest.raises(AssertionError, match="classifier free"), torch.no_grad():
        Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=4).generate({"x": noise, "context": ctx},
                                                                                                 use_tqdm=False, guidance_scale=2.0)
