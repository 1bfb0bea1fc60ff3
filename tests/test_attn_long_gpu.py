"""Long-sequence attention (max(Nq, Nk) > 2048, up to 32768 tokens): dl_attn_fwd_ex / dl_attn_bwd_ex and the square forms
dl_attn_fwd / dl_attn_bwd against fp64 attention on the same bf16 operands.

Accuracy yardstick: the error of the kernels at every new length must stay within 2x the error of the tiled kernels at N = 2048 on
operands drawn from the same distribution (computed here, in the same run).  The output buffers sit inside NaN-poisoned guards that
must come back bit-identical."""

from __future__ import annotations

import functools

import pytest
import torch

from elementwise_bounds import is_poison, poison_

pytestmark = pytest.mark.gpu

DEV = "cuda"
DH = 64
SCALE = DH**-0.5
GUARD = 4096  # poisoned elements in front of and behind every output


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import _lib, ops as _ops

    assert _lib.available(), "libdiffulab_hip.so missing on the GPU box"
    return _ops


def _unit_rms(x):
    return x / x.pow(2).mean(-1, keepdim=True).sqrt()


def make_inputs(B, H, Nq, Nk, seed, peaked=False, masked=False, tail=0):
    """bf16 q, k, v [B, H, N, 64] (unit-RMS q and k: the QK-norm regime; q x4 when peaked), dO token-major [B, Nq, H*64] and a key bias
    [B, Nk] (about 30 % random masked keys plus `tail` masked pad keys at the end) or None"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q = _unit_rms(torch.randn(B, H, Nq, DH, device=DEV, generator=g)) * (4.0 if peaked else 1.0)
    k = _unit_rms(torch.randn(B, H, Nk, DH, device=DEV, generator=g))
    v = torch.randn(B, H, Nk, DH, device=DEV, generator=g)
    do = torch.randn(B, Nq, H * DH, device=DEV, generator=g)
    bias = None
    if masked or tail:
        keep = torch.rand(B, Nk, device=DEV, generator=g) >= (0.3 if masked else 0.0)
        keep[:, 0] = True  # every sample keeps a key
        if tail:
            keep[:, Nk - tail:] = False
        bias = torch.zeros(B, Nk, device=DEV).masked_fill(~keep, float("-inf"))
    bf = lambda t: t.to(torch.bfloat16).contiguous()  # noqa: E731
    return bf(q), bf(k), bf(v), bf(do), bias


def reference(q, k, v, do_tok, bias, chunk_elems=2**26):
    """fp64 attention forward + backward, chunked over the queries: out [B, Nq, H*64], lse [B, H, Nq], dq, dk, dv head-major"""
    B, H, Nq, _ = q.shape
    Nk = k.shape[2]
    q, k, v = q.double(), k.double(), v.double()
    do = do_tok.double().reshape(B, Nq, H, DH).transpose(1, 2)
    out = torch.empty(B, H, Nq, DH, device=DEV, dtype=torch.float64)
    lse = torch.empty(B, H, Nq, device=DEV, dtype=torch.float64)
    dq = torch.empty_like(q)
    dk, dv = torch.zeros_like(k), torch.zeros_like(v)
    c = max(256, chunk_elems // (B * H * Nk))
    for i in range(0, Nq, c):
        qc, doc = q[:, :, i:i + c], do[:, :, i:i + c]
        s = qc @ k.transpose(-1, -2) * SCALE
        if bias is not None:
            s = s + bias.double()[:, None, None, :]
        l = torch.logsumexp(s, -1, keepdim=True)
        p = torch.exp(s - l)
        o = p @ v
        out[:, :, i:i + c], lse[:, :, i:i + c] = o, l[..., 0]
        dp = doc @ v.transpose(-1, -2)
        ds = p * (dp - (o * doc).sum(-1, keepdim=True))
        dq[:, :, i:i + c] = ds @ k * SCALE
        dk += ds.transpose(-1, -2) @ qc * SCALE
        dv += p.transpose(-1, -2) @ doc
        del s, p, dp, ds
    return out.transpose(1, 2).reshape(B, Nq, H * DH), lse, dq, dk, dv


def guarded(shape, dtype):
    """(view, flat buffer): a contiguous tensor of `shape` inside a NaN-poisoned allocation with GUARD elements on either side"""
    n = 1
    for s in shape:
        n *= s
    buf = poison_(torch.empty(n + 2 * GUARD, device=DEV, dtype=dtype))
    return buf[GUARD:GUARD + n].view(shape), buf


def check_guards(buf, what):
    head, tail = buf[:GUARD], buf[-GUARD:]
    assert bool(is_poison(head).all()) and bool(is_poison(tail).all()), f"{what}: a guard element was written"
    assert bool(torch.isfinite(buf[GUARD:-GUARD].float()).all()), f"{what}: unwritten or non-finite elements"


def run(ops, q, k, v, do, bias, square=False):
    """the library's forward + backward into guarded buffers; returns (out, lse, dq, dk, dv) after checking every guard"""
    B, H, Nq, _ = q.shape
    Nk = k.shape[2]
    out, ob = guarded((B, Nq, H * DH), torch.bfloat16)
    lse, lb = guarded((B, H, Nq), torch.float32)
    dq, qb = guarded((B, H, Nq, DH), torch.bfloat16)
    dk, kb = guarded((B, H, Nk, DH), torch.bfloat16)
    dv, vb = guarded((B, H, Nk, DH), torch.bfloat16)
    if square:
        assert bias is None and Nq == Nk
        ops.attn_fwd(q, k, v, out, lse, B, H, Nq, DH, SCALE)
        ops.attn_bwd(q, k, v, out, do, lse, dq, dk, dv, B, H, Nq, DH, SCALE)
    else:
        ops.attn_fwd_ex(q, k, v, out, lse, B, H, Nq, Nk, DH, SCALE, bias)
        ops.attn_bwd_ex(q, k, v, out, do, lse, dq, dk, dv, B, H, Nq, Nk, DH, SCALE, bias)
    torch.cuda.synchronize()
    for buf, what in ((ob, "out"), (lb, "lse"), (qb, "dq"), (kb, "dk"), (vb, "dv")):
        check_guards(buf, what)
    return out, lse, dq, dk, dv


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def errors(got, ref):
    out, lse, dq, dk, dv = got
    r_out, r_lse, r_dq, r_dk, r_dv = ref
    return {"out": rel(out, r_out), "dq": rel(dq, r_dq), "dk": rel(dk, r_dk), "dv": rel(dv, r_dv),
            "lse": float((lse.double() - r_lse).abs().max())}


@functools.lru_cache(maxsize=None)
def _yardstick(peaked, masked):
    """errors of the existing tiled kernels at N = 2048 (B = 1, H = 2) on operands of the same distribution"""
    from diffulab_amd import ops

    q, k, v, do, bias = make_inputs(1, 2, 2048, 2048, seed=7, peaked=peaked, masked=masked)
    e = errors(run(ops, q, k, v, do, bias), reference(q, k, v, do, bias))
    assert e["lse"] < 1e-3, e
    return e


def assert_within_yardstick(e, peaked=False, masked=False):
    y = _yardstick(peaked, masked)
    for name in ("out", "dq", "dk", "dv"):
        assert e[name] <= 2.0 * y[name], f"{name}: rel-L2 {e[name]:.3e} above 2x the 2048-token kernels' {y[name]:.3e} ({e}, {y})"
    assert e["lse"] <= 1e-3, e


@pytest.mark.parametrize("B,H,N", [(2, 2, 2304), (1, 2, 4096), (1, 1, 8192), (1, 1, 32768)])
def test_square_lengths(ops, B, H, N):
    """dl_attn_fwd / dl_attn_bwd (square, no mask) route N > 2048 to the long-sequence kernels"""
    q, k, v, do, _ = make_inputs(B, H, N, N, seed=N)
    e = errors(run(ops, q, k, v, do, None, square=True), reference(q, k, v, do, None))
    assert_within_yardstick(e)


@pytest.mark.parametrize("Nq,Nk", [(256, 4096), (4352, 2560), (2304, 512)])
def test_cross_lengths(ops, Nq, Nk):
    q, k, v, do, _ = make_inputs(2, 2, Nq, Nk, seed=Nq + Nk)
    e = errors(run(ops, q, k, v, do, None), reference(q, k, v, do, None))
    assert_within_yardstick(e)


def test_peaked_scores(ops):
    q, k, v, do, _ = make_inputs(1, 2, 4096, 4096, seed=11, peaked=True)
    e = errors(run(ops, q, k, v, do, None), reference(q, k, v, do, None))
    assert_within_yardstick(e, peaked=True)


def test_key_bias_masked_keys_and_padded_tail(ops):
    """about 30 % masked keys plus a masked pad tail (how the joint engines call it): masked keys get dK = dV = 0 exactly"""
    B, H, N = 2, 2, 4352
    q, k, v, do, bias = make_inputs(B, H, N, N, seed=13, masked=True, tail=200)
    got = run(ops, q, k, v, do, bias)
    e = errors(got, reference(q, k, v, do, bias))
    assert_within_yardstick(e, masked=True)
    masked = torch.isinf(bias)[:, None, :, None].expand(B, H, N, DH)
    for t, what in ((got[3], "dk"), (got[4], "dv")):
        assert float(t.float()[masked].abs().max()) == 0.0, f"{what} of a masked key is not zero"


def test_continuity_at_2048(ops):
    """2304 tokens whose last 256 keys are masked give the first 2048 query rows of the existing kernel at 2048 unpadded tokens"""
    B, H = 1, 2
    q, k, v, do, bias = make_inputs(B, H, 2304, 2304, seed=17, tail=256)
    out, lse, *_ = run(ops, q, k, v, do, bias)
    q0, k0, v0 = (t[:, :, :2048].contiguous() for t in (q, k, v))
    out0 = torch.empty(B, 2048, H * DH, device=DEV, dtype=torch.bfloat16)
    lse0 = torch.empty(B, H, 2048, device=DEV)
    ops.attn_fwd(q0, k0, v0, out0, lse0, B, H, 2048, DH, SCALE)
    y = _yardstick(False, False)
    assert rel(out[:, :2048], out0) <= 2.0 * y["out"], (rel(out[:, :2048], out0), y)
    assert float((lse[:, :, :2048] - lse0).abs().max()) <= 1e-3


def test_backward_is_bit_reproducible(ops):
    B, H, Nq, Nk = 1, 2, 4096, 4352
    q, k, v, do, bias = make_inputs(B, H, Nq, Nk, seed=19, masked=True)
    a = run(ops, q, k, v, do, bias)
    b = run(ops, q, k, v, do, bias)
    for x, y, what in zip(a, b, ("out", "lse", "dq", "dk", "dv")):
        assert torch.equal(x, y), f"{what} differs between two runs"


@pytest.mark.parametrize("Nq,Nk,dh", [(32768 + 256, 32768 + 256, 64), (4096 + 64, 4096 + 64, 64), (4096, 4096, 128)])
def test_refusals_before_launch(ops, Nq, Nk, dh):
    q = torch.zeros(8, device=DEV, dtype=torch.bfloat16)
    lse = torch.zeros(8, device=DEV)
    with pytest.raises(RuntimeError, match="dl_attn_fwd_ex"):
        ops.attn_fwd_ex(q, q, q, q, lse, 1, 1, Nq, Nk, dh, SCALE)
    with pytest.raises(RuntimeError, match="dl_attn_bwd_ex"):
        ops.attn_bwd_ex(q, q, q, q, q, lse, q, q, q, 1, 1, Nq, Nk, dh, SCALE)
    with pytest.raises(RuntimeError, match="dl_attn_fwd"):
        ops.attn_fwd(q, q, q, q, lse, 1, 1, Nq, dh, SCALE)
