"""CPU checks of tests/elementwise_bounds.py: the element-wise bound admits a correct kernel (fp32 accumulation, bf16 round to nearest
even) with every epilogue, and rejects the local corruptions a relative-L2 criterion lets through."""

import pytest
import torch

import elementwise_bounds as eb
from oracle import synth

SHAPES = [(16384, 1152, 384), (300, 1000, 448), (129, 130, 320), (1, 3, 64), (127, 72, 256)]


def _operands(M, N, K):
    a = synth.normal(f"eb.a{M}.{K}", (M, K)).to(torch.bfloat16)
    b = (synth.normal(f"eb.b{N}.{K}", (N, K)) * K**-0.5).to(torch.bfloat16)
    return a, b


def _kernel_like(a, b):
    """what a correct kernel computes: an fp32-accumulated product (f32 out)"""
    return a.float() @ b.float().t()


_CACHE = {}


def _plain(M, N, K):
    if (M, N, K) not in _CACHE:
        a, b = _operands(M, N, K)
        ref, err = eb.gemm_ref(a, b)
        _CACHE[(M, N, K)] = (a, b, _kernel_like(a, b), ref, err)
    return _CACHE[(M, N, K)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_correct_products_pass(M, N, K):
    a, b, acc, ref, err = _plain(M, N, K)
    eb.assert_within(acc.to(torch.bfloat16), ref, eb.store_bf16(ref, err), what="bf16 out")
    eb.assert_within(acc, ref, eb.store_f32(ref, err), what="f32 out")


@pytest.mark.parametrize("M,N,K", SHAPES[1:])
def test_correct_epilogues_pass(M, N, K):
    a, b, acc, ref, err = _plain(M, N, K)
    bias = synth.normal(f"eb.bias{N}", (N,)) * 0.5
    resid = synth.normal(f"eb.res{M}.{N}", (M, N)).to(torch.bfloat16)
    rows = 4
    gate = (synth.normal(f"eb.gate{M}.{N}", ((M + rows - 1) // rows, N)) * 0.5).to(torch.bfloat16)
    g = gate.repeat_interleave(rows, 0)[:M]
    # bias + SiLU + pre_out (f32 arithmetic in the kernel's order; SiLU as the device computes it, through exp2 and a reciprocal)
    v = acc + bias
    r1, e1 = eb.add_bias(ref, err, bias)
    eb.assert_within(v.to(torch.bfloat16), r1, eb.store_bf16(r1, e1), what="pre_out")
    l2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    z = v * (1.0 / (1.0 + torch.exp2((-v) * l2e)))
    r2, e2 = eb.silu(r1, e1)
    eb.assert_within(z.to(torch.bfloat16), r2, eb.store_bf16(r2, e2), what="silu")
    # resid + gate * z, and plain resid + acc (bf16 and f32 out)
    o = resid.float() + g.float() * z
    r3, e3 = eb.gate_resid(r2, e2, resid, g)
    eb.assert_within(o.to(torch.bfloat16), r3, eb.store_bf16(r3, e3), what="gate")
    o = resid.float() + acc
    r4, e4 = eb.gate_resid(ref, err, resid)
    eb.assert_within(o.to(torch.bfloat16), r4, eb.store_bf16(r4, e4), what="resid")
    eb.assert_within(o, r4, eb.store_f32(r4, e4), what="resid f32")
    # conv epilogue: acc + bias + resid
    o = acc + bias + resid.float()
    r5, e5 = eb.add_bias_resid(ref, err, bias, resid)
    eb.assert_within(o.to(torch.bfloat16), r5, eb.store_bf16(r5, e5), what="bias + resid")
    # fused SwiGLU: h = silu(x1) * x3 from two accumulator columns
    h = (acc[:, :1] * (1.0 / (1.0 + torch.exp2(-acc[:, :1] * l2e)))) * acc[:, 1:]
    rh, eh = eb.swiglu(ref[:, :1], err[:, :1], ref[:, 1:], err[:, 1:])
    eb.assert_within(h.to(torch.bfloat16), rh, eb.store_bf16(rh, eh), what="swiglu")


def test_correct_tn_and_conv_pass():
    R, M, N = 2048 + 64, 200, 136
    a = synth.normal("eb.tna", (R, M)).to(torch.bfloat16)
    b = synth.normal("eb.tnb", (R, N)).to(torch.bfloat16)
    init = synth.normal("eb.tnc", (M, N))
    parts = [a[i::4].float().t() @ b[i::4].float() for i in range(4)]  # four split ranges meeting in f32
    out = init + ((parts[0] + parts[1]) + parts[2]) + parts[3]
    ref, err = eb.tn_ref(a, b, init)
    eb.assert_within(out, ref, eb.store_f32(ref, err), what="tn")
    Bn, H, W, Ci, Co = 2, 8, 8, 64, 128
    x = synth.normal("eb.cx", (Bn * H * W, Ci)).to(torch.bfloat16)
    wf = (synth.normal("eb.cw", (Co, 9 * Ci)) * (9 * Ci) ** -0.5).to(torch.bfloat16)
    wconv = wf.float().reshape(Co, 3, 3, Ci).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x.float().reshape(Bn, H, W, Ci).permute(0, 3, 1, 2), wconv, padding=1)
    y = y.permute(0, 2, 3, 1).reshape(Bn * H * W, Co)
    ref, err = eb.conv_ref(x, Bn, H, W, wf)
    eb.assert_within(y.to(torch.bfloat16), ref, eb.store_bf16(ref, err), what="conv")


def _corruptions(acc, ref):
    """(name, corrupted copy) pairs of the correct bf16 output of the f32 accumulator acc"""
    out = acc.to(torch.bfloat16)
    M, N = out.shape
    r0, c0 = (M // 2) // 16 * 16, (N // 2) // 16 * 16
    z16 = out.clone()
    z16[r0:r0 + 16, c0:c0 + 16] = 0
    z8 = out.clone()
    z8[r0:r0 + 8, c0:c0 + 16] = 0
    trunc = (acc.view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)  # exact in bf16: no second rounding
    # one element moved by 2 bf16 ulps (the largest one: the one where a fixed relative slack would hide it best)
    ulp2 = out.clone()
    idx = int(ref.abs().argmax())
    flat = ulp2.view(-1).view(torch.int16)
    flat[idx] = flat[idx] + 2
    return [("zeroed 16x16 fragment", z16), ("zeroed 8x16 fragment", z8), ("truncating store", trunc), ("2 ulps", ulp2)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_corruptions_are_rejected(M, N, K):
    a, b, acc, ref, err = _plain(M, N, K)
    out = acc.to(torch.bfloat16)
    bound = eb.store_bf16(ref, err)
    for name, bad in _corruptions(acc, ref):
        if M < 16 and "fragment" in name:
            continue
        if name == "truncating store" and torch.equal(bad, out):
            continue  # (every value already exact in bf16)
        with pytest.raises(AssertionError, match="outside their bound"):
            eb.assert_within(bad, ref, bound, what=name)


def test_relative_l2_misses_what_the_bound_catches():
    """on the 16384 x 1152 x 384 product the old criterion rel < 4e-3 accepts a zeroed 8x16 fragment and a truncating bf16 store"""
    a, b, acc, ref, err = _plain(16384, 1152, 384)
    out = acc.to(torch.bfloat16)
    assert eb.rel_l2(out, ref) < 4e-3
    bad = dict(_corruptions(acc, ref))
    for name in ("zeroed 8x16 fragment", "truncating store"):
        assert eb.rel_l2(bad[name], ref) < 4e-3, name
        with pytest.raises(AssertionError, match="outside their bound"):
            eb.assert_within(bad[name], ref, eb.store_bf16(ref, err), tile=(256, 384), what=name)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_footprint_checks(dtype):
    M, N = 37, 72
    val = torch.randn(M, N).to(dtype)
    g = eb.Guarded(M, N, dtype, "cpu")
    g.win.copy_(val)
    g.check("clean")
    for name, hit in (("guard column", lambda b, w: b.__setitem__((5, 3), 0)),  # a left guard column of a window row
                      ("right guard column", lambda b, w: b.__setitem__((5, 8 + N), 1.0)),
                      ("guard row", lambda b, w: b.__setitem__((1 + M, 20), 0)),
                      ("row above", lambda b, w: b.__setitem__((0, 20), 2.0))):
        h = eb.Guarded(M, N, dtype, "cpu")
        h.win.copy_(val)
        hit(h.buf, h.win)
        with pytest.raises(AssertionError, match="guard elements written"):
            h.check(name)
    h = eb.Guarded(M, N, dtype, "cpu")
    h.win.copy_(val)
    eb.poison_(h.win[3:4, 7:8])  # one window element never written
    with pytest.raises(AssertionError, match="not finite"):
        h.check("unwritten")
    # += semantics: a window that starts from its initial value
    h = eb.Guarded(M, N, dtype, "cpu", left=0, right=0, ld=N, init=val)
    assert torch.equal(h.win, val)
    h.check("init")


def test_operand_gaps_hold_nan():
    v = torch.randn(5, 64).to(torch.bfloat16)
    op = eb.operand(v, 80, col0=8)
    assert op.stride(0) == 80 and torch.equal(op, v)
    base = op.as_strided((7, 80), (80, 1), op.storage_offset() - 8)
    mask = torch.ones(7, 80, dtype=torch.bool)
    mask[:5, 8:72] = False
    assert bool(eb.is_poison(base)[mask].all()) and bool(torch.isnan(base.float()[mask]).all())


def test_half_ulp():
    x = torch.tensor([1.0, 1.5, 2.0, 3.99, 0.75], dtype=torch.float64)
    assert torch.equal(eb.half_ulp(x, 8), torch.tensor([2**-8, 2**-8, 2**-7, 2**-7, 2**-9], dtype=torch.float64))
    assert torch.equal(eb.half_ulp(x, 24), torch.tensor([2**-24, 2**-24, 2**-23, 2**-23, 2**-25], dtype=torch.float64))
