"""GPU tests of the gradient with respect to the denoiser's input: `dl_patch_embed_dgrad` element by element against fp64, the input
gradient of the two DiT engines against the oracle (held, in the bf16 regime, to the bf16 regime's own error: the three legs of
tests/test_parity_bf16_gpu.py), and the input-gradient-only backward (no weight-gradient launch, gradient arena untouched).

Bounds: tests/flow_nll_common.py (k = D + 1 roundings on a sum of D products); engines: test_parity_bf16_gpu.py's GRAD_BOUND / FACTOR
and test_fp32_gpu.py's TOL."""

import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import flow_nll_common as fn  # noqa: E402
from oracle import diffusion as od  # noqa: E402
from oracle import dit as odit  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
S2 = dict(input_channels=4, output_channels=4, inner_dim=384, embedding_dim=384, num_heads=6, mlp_ratio=4, patch_size=2, depth=12,
          n_classes=1000, classifier_free=True)
SMALL = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2, depth=2,
             n_classes=10, classifier_free=True)
GRAD_BOUND, FACTOR, TOL = 1e-2, 1.5, 1e-5  # (test_parity_bf16_gpu.py, test_fp32_gpu.py)
RUN_TO_RUN = 1e-4  # two backwards of the same state where f32 atomics order the sums (tests/test_trainer_gpu.py)
GUARD = 64


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,C,H,W,p,D,ld", [(4, 4, 16, 16, 2, 128, 128), (2, 3, 16, 16, 2, 64, 64), (1, 32, 8, 8, 1, 64, 64),
                                            (2, 4, 16, 32, 2, 64, 64), (4, 1, 16, 16, 4, 64, 64), (1, 4, 6, 10, 2, 64, 64),
                                            (1, 4, 16, 16, 2, 1152, 1216), (1, 4, 16, 16, 2, 4096, 4096)])
def test_patch_embed_dgrad_element_by_element(B, C, H, W, p, D, ld, dtype):
    from diffulab_amd import ops

    M = B * (H // p) * (W // p)
    tag = f"ig.{B}.{C}.{H}.{W}.{p}.{D}"
    dtok = synth.normal(tag + ".dtok", (M, ld)).to(dtype)
    w = synth.normal(tag + ".w", (D, C, p, p)) * D**-0.5
    ref, mag = fn.patch_embed_dgrad(dtok.float(), w.reshape(D, -1), B, C, H, W, p)  # (the bf16 values themselves are the operands)
    bound = fn.patch_embed_dgrad_bound(mag, D)
    n = B * C * H * W
    runs = []
    for _ in range(2):
        buf = torch.full((n + 2 * GUARD,), 7.5, device=DEV)
        out = buf[GUARD:GUARD + n].view(B, C, H, W)
        ops.patch_embed_dgrad(dtok.to(DEV), w.to(DEV), out, p)
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == 7.5).all()) and bool((buf[GUARD + n:] == 7.5).all()), "wrote outside the image"
        runs.append(out.clone())
    err = (runs[0].double().cpu() - ref).abs()
    worst = (err / bound).max().item()
    print(f"dl_patch_embed_dgrad {tag} {dtype}: worst error / bound {worst:.3f}")
    assert worst <= 1.0, (tag, worst)
    assert torch.equal(runs[0], runs[1]), "two runs differ"
    # the wrong layouts are outside the bound on these inputs (the bound is live)
    # ((p2 p1) swapped needs p > 1 to differ; (p1 p2 c) against (c p1 p2) needs p > 1 and more than one channel)
    for order in (("swap",) if p > 1 else ()) + (("ppc",) if p > 1 and C > 1 else ()):
        other = fn.patch_embed_dgrad(dtok.float(), w.reshape(D, -1), B, C, H, W, p, order=order)[0]
        assert bool(((other - ref).abs() > bound).any())


# ------------------------------------------------------------------------------------------------------------------ the engines
def _inputs(cfgk, B, H, tag):
    C = cfgk["input_channels"]
    x0, noise = synth.normal(f"{tag}.x0", (B, C, H, H)), synth.normal(f"{tag}.noise", (B, C, H, H))
    t = synth.uniform(f"{tag}.t", (B,), lo=0.05, hi=0.95)
    y = synth.integers(f"{tag}.y", (B,), cfgk["n_classes"])
    return x0, noise, t, y


def _oracle_dz(P, cfg, x0, noise, t, y, autocast):
    z = od.flow_add_noise(x0, t, noise).requires_grad_(True)
    if autocast:
        with odit.bf16_autocast():
            loss = od.flow_loss(odit.dit_forward(P, z, t, y, cfg), x0, noise)
    else:
        loss = od.flow_loss(odit.dit_forward(P, z, t, y, cfg), x0, noise)
    (dz,) = torch.autograd.grad(loss, z)
    return dz


def _model(cfgk, seed, precision):
    from diffulab_amd import MMDiT

    m = MMDiT(simple_dit=True, **cfgk)
    m.load_state_dict(synth.dit_params(odit.param_shapes(odit.DiTConfig(**cfgk)), seed=seed))
    m.set_precision(precision)
    return m.to(DEV)


def _hip_step(m, x0, noise, t, y, x_grad, context=None):
    """flow loss through the model and its backward -> (d loss / d z_t or None, copy of the flat parameter gradient)"""
    from diffulab_amd import ops
    from diffulab_amd.diffuse.modelizations.diffusion import mse_head

    z = ops.flow_add_noise(x0.to(DEV), noise.to(DEV), t.to(DEV))
    z.requires_grad_(x_grad)
    m.zero_grad()
    with (context() if context is not None else torch.enable_grad()):
        pred = m(x=z, timesteps=t, y=y.to(DEV), p=0.0)["x"]
    loss = mse_head(pred, noise.to(DEV), x0.to(DEV), ops.LOSS_FLOW)
    loss.backward()
    torch.cuda.synchronize()
    return (z.grad.detach().clone() if x_grad else None), m._flat_grad.clone()


CASES = [("small", SMALL, 5, 4, 16, "pb.small"), ("s2", S2, 7, 2, 32, "ig.s2")]
_legs_cache: dict = {}


def _legs(name, cfgk, seed, B, H, tag):
    """the two oracle legs of a case, computed once and shared"""
    if name not in _legs_cache:
        cfg = odit.DiTConfig(**cfgk)
        P = synth.dit_params(odit.param_shapes(cfg), seed=seed)
        x0, noise, t, y = _inputs(cfgk, B, H, tag)
        _legs_cache[name] = (_oracle_dz(P, cfg, x0, noise, t, y, False), _oracle_dz(P, cfg, x0, noise, t, y, True))
    return _legs_cache[name]


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("name,cfgk,seed,B,H,tag", CASES, ids=[c[0] for c in CASES])
def test_input_gradient_of_the_engines(name, cfgk, seed, B, H, tag, precision):
    d32, dbf = _legs(name, cfgk, seed, B, H, tag)
    x0, noise, t, y = _inputs(cfgk, B, H, tag)
    m = _model(cfgk, seed, precision)
    dz, g_x = _hip_step(m, x0, noise, t, y, True)
    assert dz.shape == x0.shape and dz.dtype == torch.float32
    e_hip, e_bf = rel(dz, d32), rel(dbf, d32)
    print(f"{name} {precision}: d loss / d z_t rel-L2 hip {e_hip:.3e}, bf16-autocast oracle {e_bf:.3e}")
    if precision == "fp32":
        assert e_hip <= TOL
    else:
        assert e_hip <= max(GRAD_BOUND, FACTOR * e_bf)
        if name == "small":  # the reference's own autocast error on these inputs (tests/golden/dit_input_grad.npz)
            g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dit_input_grad.npz"))
            assert rel(d32, torch.from_numpy(g["dz_fp32"])) <= 1e-6
            assert e_hip <= max(GRAD_BOUND, FACTOR * float(g["autocast_err"]))
    # Parameter gradients: the step with x.requires_grad must match a plain step as closely as two plain steps match each other.  At
    # these small batches some tensors (LayerNorm-affine and modulation sums, the atomic weight gradients) meet through f32 atomics
    # whose order varies from run to run, and two runs of such a tensor are often, not always, bit-equal: "equal in two runs" does not
    # show a tensor to be reproducible (a first version of this test asserted bit equality per tensor on that evidence and failed on
    # one tensor in one of three runs of the suite).  So: the runs alternate, plain / with x / plain / with x; where the WHOLE arena is
    # bit-equal within both pairs -- the step is reproducible here -- it must be bit-equal across them; otherwise every tensor of a
    # step with x lies within 1e-4 relative of a plain step (what tests/test_trainer_gpu.py and tests/test_joint_forms_gpu.py hold two
    # backwards of the same state to), or twice the plain pair's own spread where that is larger.
    _, p1 = _hip_step(m, x0, noise, t, y, False)
    _, x2 = _hip_step(m, x0, noise, t, y, True)
    _, p2 = _hip_step(m, x0, noise, t, y, False)
    if torch.equal(p1, p2) and torch.equal(g_x, x2):
        assert torch.equal(g_x, p1), "the step is bit-reproducible with and without x.requires_grad, but differs between the two"
    lay = m.engine.layout
    for n_ in lay.entries:
        a, b = lay.view(p1, n_), lay.view(p2, n_)
        for c in (lay.view(g_x, n_), lay.view(x2, n_)):
            assert rel(c, a) <= max(RUN_TO_RUN, 2 * rel(b, a)), n_


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_input_gradient_only_backward(precision, monkeypatch):
    from diffulab_amd import ops

    name, cfgk, seed, B, H, tag = CASES[0]
    d32, dbf = _legs(name, cfgk, seed, B, H, tag)
    x0, noise, t, y = _inputs(cfgk, B, H, tag)
    m = _model(cfgk, seed, precision)
    bound = TOL if precision == "fp32" else max(GRAD_BOUND, FACTOR * rel(dbf, d32))
    calls: list[str] = []
    orig = ops._call
    monkeypatch.setattr(ops, "_call", lambda name_, *a: (calls.append(name_), orig(name_, *a))[1])

    def wgrad_like(c: str) -> bool:
        # weight gradients, column sums, folds, the conditioning path, and the native block sequence (which issues its own)
        return any(k in c for k in ("gemm_tn", "wgrad", "colsum", "reduce_rows", "cond_combine_bwd", "silu_bwd", "dit_block_bwd"))

    dz_full, _ = _hip_step(m, x0, noise, t, y, True)
    full = list(calls)
    assert full.count("dl_patch_embed_dgrad") == 1 and any(wgrad_like(c) for c in full)
    calls.clear()
    _hip_step(m, x0, noise, t, y, False)
    plain = list(calls)
    assert "dl_patch_embed_dgrad" not in plain
    without = [c for c in full if c != "dl_patch_embed_dgrad"]
    assert without == plain, "x.requires_grad changed the launch sequence beyond the one data-gradient launch"

    def sentinel_run(context, freeze):
        for q in m.parameters():
            q.requires_grad_(not freeze)
        m.engine  # (flattened)
        m._flat_grad.fill_(-3.25)
        before = m._flat_grad.clone()
        calls.clear()
        z = ops.flow_add_noise(x0.to(DEV), noise.to(DEV), t.to(DEV)).requires_grad_(True)
        from diffulab_amd.diffuse.modelizations.diffusion import mse_head

        with (context() if context is not None else torch.enable_grad()):
            pred = m(x=z, timesteps=t, y=y.to(DEV), p=0.0)["x"]
        mse_head(pred, noise.to(DEV), x0.to(DEV), ops.LOSS_FLOW).backward()
        torch.cuda.synchronize()
        assert torch.equal(m._flat_grad, before), "the gradient arena was written"
        bad = [c for c in calls if wgrad_like(c)]
        assert not bad, bad
        assert calls.count("dl_patch_embed_dgrad") == 1
        assert rel(z.grad, d32) <= bound and rel(z.grad, dz_full) <= bound
        for q in m.parameters():
            q.requires_grad_(True)

    sentinel_run(None, freeze=True)                 # no parameter requires grad
    sentinel_run(m.input_grad_only, freeze=False)   # trainable parameters, forward inside input_grad_only()
    m.zero_grad()
