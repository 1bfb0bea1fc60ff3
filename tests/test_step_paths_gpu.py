"""The optimizer-step, weight-cast and noising kernels of csrc/elementwise.hip, element by element, with write guards.

Every case runs through the C ABI (ops.CastTable: through diffulab_amd.ops, which owns the descriptor table).  A case
  * writes into NaN-poisoned allocations with checked guards on both sides (in-place buffers sit in such allocations too),
  * compares every read-only input (gradients, coefficient, device scalars, t, tables, sources) bit for bit afterwards,
  * judges every output element against the fp64 reference within its bound, or bit for bit where the kernel only moves or rounds
    data (tests/step_bounds.py; tests/test_step_bounds_host.py shows on these same inputs what the bounds admit and reject).
Sizes are the smallest that reach each code path: tail only / body only / both, every alignment phase of the scalar forms, and one
size past the 2048 x 256 thread cap of ew_grid for every grid-stride loop.  The closing tests print the worst ratio per kernel and
assert that every extern "C" entry point of the file was called.
"""

from __future__ import annotations

import functools
import os
import re

import pytest
import torch

import elementwise_bounds as eb
import f32_bounds as fb
import step_bounds as sb

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024  # poisoned elements on each side of a dense buffer
CALLED: set[str] = set()
WORST: dict[str, tuple[float, str]] = {}
# entry points of elementwise.hip this module does not drive: the error / version / device / stream plumbing, the lab switch, and
# dl_sgd_step*, whose write-guard and alignment-phase tests live in tests/test_sgd_gpu.py
EXCLUDED = {"dl_last_error", "dl_version", "dl_device_info", "dl_lab_set_wg_cap", "dl_stream_create_masked",
            "dl_stream_create_low_priority", "dl_stream_destroy", "dl_sgd_step", "dl_sgd_step_dev"}


# ------------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    return _lib.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def call(L, name, *args):
    CALLED.add(name)
    return L.call(name, *args)


class Flat:
    """a dense tensor between two runs of GUARD poisoned elements, `shift` elements off the allocation's 16-byte grid.
    init None: an output, it starts poisoned; else it starts from `init` (a CPU tensor, kept for `unchanged`)"""

    def __init__(self, shape, init=None, shift=0, dtype=F32):
        n = 1
        for s in shape:
            n *= s
        self.buf = eb.poison_(torch.empty(n + 2 * GUARD + shift, dtype=dtype, device=DEV))
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        self.t = self.buf[self.lo:self.hi].view(*shape)
        self.init = init
        if init is not None:
            assert init.dtype == dtype and init.numel() == n
            self.t.copy_(init.reshape(shape))

    def ptr(self):
        return self.t.data_ptr()

    def guards(self, what):
        assert bool(eb.is_poison(self.buf[:self.lo]).all()) and bool(eb.is_poison(self.buf[self.hi:]).all()), f"{what}: guard written"

    def unchanged(self, what):
        """a read-only input: guards intact, contents bit-identical to what was put there"""
        self.guards(what)
        a, b = self.t.reshape(-1), self.init.reshape(-1).to(DEV)
        iv = (lambda t: t.view(torch.int16)) if self.t.element_size() == 2 else (lambda t: t.view(torch.int32))
        assert bool(torch.equal(iv(a), iv(b))), f"{what}: a read-only input was written"


def window(rows, ld, dtype=BF16):
    """a [rows, ld] destination whose rows are the allocation's rows (the kernel owns every column), guard rows above and below"""
    return eb.Guarded(rows, ld, dtype, DEV, left=0, right=0, ld=ld)


def guards_intact(G, what):
    hit = G.mask & ~eb.is_poison(G.buf)
    assert not bool(hit.any()), f"{what}: {int(hit.sum())} guard elements written"


def note(kernel: str, ratio: float, cid: str):
    if ratio > WORST.get(kernel, (-1.0, ""))[0]:
        WORST[kernel] = (ratio, cid)


def settle(kernel: str, cid: str, got: dict, ref: dict):
    """every output element inside its bound; keeps the worst ratio per kernel and output for the report"""
    ratios = fb.judge(got, ref)
    print(f"{cid}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        note(f"{kernel}.{k}", v, cid)
    for k, (r, bound) in ref.items():
        eb.assert_within(got[k].reshape(1, -1), r.reshape(1, -1), bound.reshape(1, -1), what=f"{cid}: {k}")
    assert all(v <= 1.0 for v in ratios.values()), (cid, ratios)


def same_bits(a, b) -> bool:
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ------------------------------------------------------------------------------------------------------------------ AdamW
FORMS = ("plain", "clip", "dev", "dev_clip")
HYPERS = {h[0]: h[1:] for h in sb.ADAMW_HYPERS}
BIG_HYPERS = ("default-step1", "visible-gs0.5", "visible-coef0.37")  # the sets that also run past the thread cap


@functools.lru_cache(maxsize=8)
def adamw_inputs(n, seed):
    return sb.adamw_inputs(n, seed)


def scalars(hp: str, form: str):
    lr, betas, eps, wd, step, gs, coef = HYPERS[hp]
    return sb.adamw_scalars(lr, betas, eps, wd, step, gs, coef if "clip" in form else None)


def run_adamw(L, form, S, inputs, shift=0, what=""):
    """one step through the entry point of `form`; -> (p, m, v) device tensors after guard and read-only checks"""
    p0, g0, m0, v0 = inputs
    n = p0.numel()
    P, M, V, G = (Flat((n,), init=t, shift=shift) for t in (p0, m0, v0, g0))
    ro = [(G, "g")]
    base = (P.ptr(), G.ptr(), M.ptr(), V.ptr(), n)
    host = (S["lr"], S["b1"], S["b2"], S["eps"], S["wd"], S["bc1"], S["bc2"], S["grad_scale"])
    if "clip" in form:
        C = Flat((1,), init=torch.tensor([S["coef"]], dtype=F32), shift=shift)
        ro.append((C, "coef"))
    if form.startswith("dev"):
        H = Flat((8,), init=sb.adamw_hyper(S), shift=shift)
        ro.append((H, "hyper"))
    if form == "plain":
        call(L, "dl_adamw_step", *base, *host, _s())
    elif form == "clip":
        call(L, "dl_adamw_step_clip", *base, *host, C.ptr(), _s())
    elif form == "dev":
        call(L, "dl_adamw_step_dev", *base, H.ptr(), _s())
    else:
        call(L, "dl_adamw_step_dev_clip", *base, H.ptr(), C.ptr(), _s())
    torch.cuda.synchronize()
    for F, name in ((P, "p"), (M, "m"), (V, "v")):
        F.guards(f"{what}: {name}")
    for F, name in ro:
        F.unchanged(f"{what}: {name}")
    return P.t, M.t, V.t


def check_adamw(L, form, hp, n, shift=0):
    S = scalars(hp, form)
    inputs = adamw_inputs(n, n)
    cid = f"adamw-{form}-{hp}-n{n}" + (f"-shift{shift}" if shift else "")
    p, m, v = run_adamw(L, form, S, inputs, shift, cid)
    ref = sb.adamw_ref(*(t.to(DEV) for t in inputs), S)
    settle(f"adamw_{'dev_' if form.startswith('dev') else ''}k", cid, {"p": p, "m": m, "v": v}, ref)


@pytest.mark.parametrize("hp", list(HYPERS))
@pytest.mark.parametrize("form", FORMS)
def test_adamw_against_fp64(lib, form, hp):
    """every form against fp64 (not against its sibling) at the sizes that are tail only, body only and both"""
    dev = form.startswith("dev")
    for i, n in enumerate(sb.ADAMW_SMALL_N):
        check_adamw(lib, form, hp, n, shift=i % 4 if dev else 0)  # the dev forms: buffers 0, 4, 8 and 12 bytes past a 16-byte boundary
    if dev:
        for shift in (1, 2, 3):
            check_adamw(lib, form, hp, 1027, shift=shift)
    if hp in BIG_HYPERS:
        check_adamw(lib, form, hp, sb.ADAMW_DEV_BIG_N if dev else sb.ADAMW_PLAIN_BIG_N, shift=3 if dev else 0)


def test_adamw_plain_forms_refuse_unaligned_buffers(lib):
    S = scalars("default-step1", "clip")
    t = torch.zeros(16, device=DEV)
    c = torch.ones(1, device=DEV)
    host = (S["lr"], S["b1"], S["b2"], S["eps"], S["wd"], S["bc1"], S["bc2"], S["grad_scale"])
    with pytest.raises(RuntimeError):
        call(lib, "dl_adamw_step", t.data_ptr() + 4, t.data_ptr(), t.data_ptr(), t.data_ptr(), 8, *host, _s())
    with pytest.raises(RuntimeError):
        call(lib, "dl_adamw_step_clip", t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr() + 8, 8, *host, c.data_ptr(), _s())
    assert bool((t == 0).all())


@pytest.mark.parametrize("hp", ("default-step1", "visible-coef0.37"))
def test_adamw_position_independence(lib, hp):
    """one (p, g, m, v) quadruple replicated over an n = 4 k + 3 buffer: every element of the float4 body, of the tail and of the
    device-scalar kernel (at every alignment phase) comes back with the same bits, in all four forms"""
    n = 1027
    quads = adamw_inputs(8, 99)
    for j in range(8):
        inputs = tuple(t[j].repeat(n) for t in quads)
        for clip in (False, True):
            plain, dev = ("clip", "dev_clip") if clip else ("plain", "dev")
            S = scalars(hp, plain)
            a = run_adamw(lib, plain, S, inputs, 0, f"position-{plain}")
            for name, t in zip("pmv", a):
                bits = t.view(torch.int32)
                assert bool((bits == bits[0]).all()), f"{plain}, quadruple {j}: {name} depends on the element's position " \
                    f"(body {bits[0].item():#x}, tail {bits[-1].item():#x})"
            for shift in (0, 1, 2, 3):
                b = run_adamw(lib, dev, S, inputs, shift, f"position-{dev}")
                for name, x, y in zip("pmv", a, b):
                    assert same_bits(x, y), f"{dev} (shift {shift}) and {plain}, quadruple {j}: {name} differs"


@pytest.mark.parametrize("n", (1027, sb.ADAMW_PLAIN_BIG_N))
def test_adamw_plain_and_dev_forms_agree_bit_for_bit(lib, n):
    """the claim FusedAdamW (eager / graph mode) and FusedMuon rest on: on random data the launch-scalar forms and the device-scalar
    forms write the same bits, past the thread cap too"""
    inputs = adamw_inputs(n, n)
    for hp, pair in (("default-step1", ("plain", "dev")), ("visible-coef0.37", ("clip", "dev_clip"))):
        S = scalars(hp, pair[0])
        a = run_adamw(lib, pair[0], S, inputs, 0, f"agree-{pair[0]}-n{n}")
        b = run_adamw(lib, pair[1], S, inputs, 1, f"agree-{pair[1]}-n{n}")
        for name, x, y in zip("pmv", a, b):
            assert same_bits(x, y), f"{pair[0]} vs {pair[1]}, n = {n}: {name} differs in {int((x != y).sum())} elements"


# ------------------------------------------------------------------------------------------------------------------ noising
def run_flow(L, x, e, t, what):
    B, chw = x.shape
    X, E, Tt, Z = Flat((B, chw), init=x), Flat((B, chw), init=e), Flat((B,), init=t), Flat((B, chw))
    call(L, "dl_flow_add_noise", X.ptr(), E.ptr(), Tt.ptr(), Z.ptr(), B, chw, _s())
    torch.cuda.synchronize()
    Z.guards(what)
    for F, name in ((X, "x"), (E, "noise"), (Tt, "t")):
        F.unchanged(f"{what}: {name}")
    return Z.t


@pytest.mark.parametrize("shape", sb.FLOW_VEC_SHAPES + sb.FLOW_SCALAR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_flow_add_noise(lib, shape):
    B, chw = shape
    x, e = sb.noise_inputs(B, chw)
    t = sb.sample_times(B)
    cid = f"flow-{'vec' if chw % 4 == 0 else 'scalar'}-{B}x{chw}"
    z = run_flow(lib, x, e, t, cid)
    settle("flow_add_noise_k", cid, {"z": z}, sb.flow_ref(x.to(DEV), e.to(DEV), t.to(DEV)))


def test_flow_float4_and_scalar_forms_agree_bit_for_bit(lib):
    """the same values through the float4 form (3 samples of 1024) and, one element per sample, through the scalar form"""
    B, chw = 3, 1024
    x, e = sb.noise_inputs(B, chw)
    t = sb.sample_times(B)
    zv = run_flow(lib, x, e, t, "flow-bits-vec")
    zs = run_flow(lib, x.reshape(-1, 1), e.reshape(-1, 1), t.repeat_interleave(chw), "flow-bits-scalar")
    assert same_bits(zv.reshape(-1), zs.reshape(-1)), f"{int((zv.reshape(-1) != zs.reshape(-1)).sum())} elements differ between the forms"


@pytest.mark.parametrize("T", (8, 1000))
@pytest.mark.parametrize("shape", sb.FLOW_SCALAR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_ddpm_add_noise(lib, shape, T):
    B, chw = shape
    x, e = sb.noise_inputs(B, chw)
    t = sb.sample_steps(B, T)
    sab, ab = sb.ddpm_tables(T)
    X, E, Tt, SA, AB, O = Flat((B, chw), init=x), Flat((B, chw), init=e), Flat((B,), init=t, dtype=torch.int32), Flat((T,), init=sab), \
        Flat((T,), init=ab), Flat((B, chw))
    cid = f"ddpm-T{T}-{B}x{chw}"
    call(lib, "dl_ddpm_add_noise", X.ptr(), E.ptr(), Tt.ptr(), SA.ptr(), AB.ptr(), O.ptr(), B, chw, _s())
    torch.cuda.synchronize()
    O.guards(cid)
    for F, name in ((X, "x"), (E, "noise"), (Tt, "t"), (SA, "sqrt_ab"), (AB, "ab")):
        F.unchanged(f"{cid}: {name}")
    settle("ddpm_add_noise_k", cid, {"xt": O.t}, sb.ddpm_ref(x.to(DEV), e.to(DEV), t.to(DEV), sab.to(DEV), ab.to(DEV)))


@pytest.mark.parametrize("beta", sb.EMA_BETAS)
@pytest.mark.parametrize("n", sb.EMA_N)
def test_ema_update(lib, n, beta):
    ema0, p = (t[0] for t in sb.noise_inputs(1, n, seed=n))  # a non-zero EMA
    Em, P = Flat((n,), init=ema0, shift=1), Flat((n,), init=p, shift=2)
    cid = f"ema-n{n}-beta{beta}"
    call(lib, "dl_ema_update", Em.ptr(), P.ptr(), beta, n, _s())
    torch.cuda.synchronize()
    Em.guards(cid)
    P.unchanged(f"{cid}: p")
    settle("ema_k", cid, {"ema": Em.t}, sb.ema_ref(ema0.to(DEV), p.to(DEV), beta))


# ------------------------------------------------------------------------------------------------------------------ casts
def cast_1d_sources():
    return (("patterns", sb.f32_patterns()), ("one", sb.from_bits32(torch.tensor([0x3F818000]))),
            ("loop", sb.weight_input(1, sb.EW_CAP + 77).reshape(-1)))


@pytest.mark.parametrize("which", ("patterns", "one", "loop"))
def test_cast_f32_to_bf16(lib, which):
    """f2bf on every pattern class: ties on even and odd mantissas, carries into the exponent and to infinity, +-0, subnormals, inf,
    NaN.  Run over a poisoned destination and over one filled with 1.0: an element left unwritten shows in at least one of them
    (the poison is itself a NaN, which a NaN source may legitimately produce)"""
    src = dict(cast_1d_sources())[which]
    n = src.numel()
    S = Flat((n,), init=src, shift=1)
    for fill in (None, torch.ones(n, dtype=BF16)):
        D = Flat((n,), init=fill, shift=3, dtype=BF16)
        call(lib, "dl_cast_f32_to_bf16", S.ptr(), D.ptr(), n, _s())
        torch.cuda.synchronize()
        D.guards(f"cast_f32_to_bf16-{which}")
        bad = sb.cast_mismatch(D.t, S.t)
        assert bad == 0, f"cast_f32_to_bf16-{which}: {bad} of {n} elements are not the round-to-nearest-even of their source"
    S.unchanged(f"cast_f32_to_bf16-{which}: src")
    note("cast_f2b_k", 0.0, which)


@pytest.mark.parametrize("which", ("patterns", "one", "loop"))
def test_cast_bf16_to_f32(lib, which):
    """a shift: bit-exact for all 65 536 patterns, NaN payloads included (no result has the poison's low half)"""
    src = {"patterns": sb.bf16_patterns(), "one": sb.from_bits16(torch.tensor([0xC049])),
           "loop": sb.from_bits16(torch.arange(sb.EW_CAP + 77) * 40503)}[which]
    n = src.numel()
    S, D = Flat((n,), init=src, shift=1, dtype=BF16), Flat((n,), shift=1)
    call(lib, "dl_cast_bf16_to_f32", S.ptr(), D.ptr(), n, _s())
    torch.cuda.synchronize()
    D.guards(f"cast_bf16_to_f32-{which}")
    S.unchanged(f"cast_bf16_to_f32-{which}: src")
    assert bool(torch.equal(sb.bits32(D.t), sb.bf16_to_f32_bits(S.t))), f"cast_bf16_to_f32-{which}: not the source shifted left by 16"
    note("cast_b2f_k", 0.0, which)


@pytest.mark.parametrize("which", ("patterns", "1x4", "loop"))
def test_cast2d_f32_to_bf16(lib, which):
    """pack2bf on the pattern table, as a window of wider rows on both sides; one float4; more float4s than the thread cap"""
    if which == "patterns":
        src, ld_s, ld_d = sb.f32_patterns().reshape(384, 1024), 1032, 1040
    elif which == "1x4":
        src, ld_s, ld_d = sb.from_bits32(torch.tensor([[0x3F808000, 0x3F818000, 0xBF80C000, 0x7F7FFFFF]])), 8, 12
    else:
        src, ld_s, ld_d = sb.weight_input(2052, 1024), 1028, 1032  # 2052 * 1024 / 4 = 525 312 > 524 288
    rows, cols = src.shape
    s = eb.operand(src.to(DEV), ld_s, col0=4)  # past its row and below its last row the kernel would read NaN
    for fill in (None, torch.ones(rows, cols, dtype=BF16)):
        D = eb.Guarded(rows, cols, BF16, DEV, left=8, ld=ld_d, init=fill)
        call(lib, "dl_cast2d_f32_to_bf16", s.data_ptr(), s.stride(0), D.win.data_ptr(), D.win.stride(0), rows, cols, _s())
        torch.cuda.synchronize()
        guards_intact(D, f"cast2d-{which}")
        bad = sb.cast_mismatch(D.win, s)
        assert bad == 0, f"cast2d-{which}: {bad} of {rows * cols} elements are not the round-to-nearest-even of their source"
    assert bool(torch.equal(sb.bits32(s), sb.bits32(src).to(DEV)))
    note("cast2d_f2b_k", 0.0, which)


def test_cast2d_refuses_what_it_cannot_vectorise(lib):
    s, d = torch.zeros(4, 8, device=DEV), torch.zeros(4, 8, dtype=BF16, device=DEV)
    for (ld_s, ld_d, cols, off) in ((8, 8, 3, 0), (6, 8, 4, 0), (8, 6, 4, 0), (8, 8, 4, 4)):
        with pytest.raises(RuntimeError):
            call(lib, "dl_cast2d_f32_to_bf16", s.data_ptr() + off, ld_s, d.data_ptr(), ld_d, 2, cols, _s())


# ------------------------------------------------------------------------------------------------------------------ layouts
def run_cast_weight(L, S, R, C, ld_dst, ld_t, what):
    """dl_cast_weight of the source Flat S into fresh guarded windows (ld None: that destination is not asked for)"""
    Dp = window(R, ld_dst) if ld_dst is not None else None
    Dt = window(C, ld_t) if ld_t is not None else None
    call(L, "dl_cast_weight", S.ptr(), R, C, Dp.win.data_ptr() if Dp else None, ld_dst or 0, Dt.win.data_ptr() if Dt else None,
         ld_t or 0, _s())
    torch.cuda.synchronize()
    for G in (Dp, Dt):
        if G is not None:
            guards_intact(G, what)
    return Dp, Dt


def expect_bits(G, want, what):
    """no poison left inside [rows, ld), padding columns exactly +0, every element the rounding of its source: all of it is `want`"""
    got = sb.bits16(G.win)
    assert not bool((got == eb.BF16_POISON).any()), f"{what}: {int((got == eb.BF16_POISON).sum())} elements inside [rows, ld) unwritten"
    bad = got != want.to(DEV)
    if bool(bad.any()):
        r, c = (int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, first [{r}, {c}] = {int(got[r, c]):#06x}, "
                             f"expected {int(want[r, c]):#06x}; 32 x 32 tile ({r // 32}, {c // 32})")


@pytest.mark.parametrize("shape", sb.CAST_WEIGHT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cast_weight(lib, shape):
    R, C = shape
    src = sb.weight_input(R, C)
    S = Flat((R, C), init=src, shift=1)
    for (pd, pt) in sb.CAST_WEIGHT_PADS:
        for want_p, want_t in ((True, False), (False, True), (True, True)):
            ld_dst, ld_t = (C + pd if want_p else None), (R + pt if want_t else None)
            cid = f"cast_weight-{R}x{C}-ld{ld_dst}-ldt{ld_t}"
            Dp, Dt = run_cast_weight(lib, S, R, C, ld_dst, ld_t, cid)
            if Dp is not None:
                expect_bits(Dp, sb.plain_bits(src, ld_dst), cid + ": dst")
            if Dt is not None:
                expect_bits(Dt, sb.transposed_bits(src, ld_t), cid + ": dstT")
    S.unchanged(f"cast_weight-{R}x{C}: src")
    note("cast_weight_k", 0.0, f"{R}x{C}")


def test_cast_weight_refusals(lib):
    s, d = torch.zeros(8, 8, device=DEV), torch.zeros(8, 8, dtype=BF16, device=DEV)
    for args in ((8, 8, None, 0, None, 0), (8, 8, d.data_ptr(), 7, None, 0), (8, 8, None, 0, d.data_ptr(), 7), (0, 8, d.data_ptr(), 8, None, 0)):
        with pytest.raises(RuntimeError):
            call(lib, "dl_cast_weight", s.data_ptr(), *args, _s())


def run_cast_swiglu(L, S, F, C, ld, what):
    D = window(2 * F, ld)
    call(L, "dl_cast_weight_swiglu", S.ptr(), F, C, D.win.data_ptr(), ld, _s())
    torch.cuda.synchronize()
    guards_intact(D, what)
    return D


@pytest.mark.parametrize("shape", sb.SWIGLU_SHAPES, ids=lambda s: f"F{s[0]}-C{s[1]}-ld{s[2]}")
def test_cast_weight_swiglu(lib, shape):
    F, C, ld = shape
    src = sb.weight_input(2 * F, C)
    S = Flat((2 * F, C), init=src, shift=1)
    cid = f"cast_weight_swiglu-F{F}-C{C}-ld{ld}"
    expect_bits(run_cast_swiglu(lib, S, F, C, ld, cid), sb.swiglu_bits(src, ld), cid)
    S.unchanged(cid + ": src")
    note("cast_weight_swiglu_k", 0.0, cid)


def test_cast_weight_swiglu_refuses_ragged_groups(lib):
    s, d = torch.zeros(48, 8, device=DEV), eb.poison_(torch.empty(64, 8, dtype=BF16, device=DEV))
    with pytest.raises(RuntimeError):
        call(lib, "dl_cast_weight_swiglu", s.data_ptr(), 24, 8, d.data_ptr(), 8, _s())
    with pytest.raises(RuntimeError):
        call(lib, "dl_cast_weight_swiglu", s.data_ptr(), 16, 8, d.data_ptr(), 7, _s())
    torch.cuda.synchronize()
    assert bool(eb.is_poison(d).all())


# ------------------------------------------------------------------------------------------------------------------ ops.CastTable
def build_table(spec):
    """-> (sources, entries for ops.CastTable, [(R, C, src, {kind: (Guarded, ld)})])"""
    srcs, entries, rows = [], [], []
    for i, (R, C, ld_dst, ld_t, ld_g) in enumerate(spec):
        src = sb.weight_input(R, C, seed=i)
        S = Flat((R, C), init=src, shift=i % 4)
        dests = {}
        if ld_dst is not None:
            dests["dst"] = (window(R, ld_dst), ld_dst)
        if ld_t is not None:
            dests["dst_t"] = (window(C, ld_t), ld_t)
        if ld_g is not None:
            dests["dst_swiglu"] = (window(R, ld_g), ld_g)
        srcs.append(S)
        entries.append((S.t,) + tuple(dests[k][0].win if k in dests else None for k in ("dst", "dst_t", "dst_swiglu")))
        rows.append((R, C, src, dests))
    return srcs, entries, rows


@pytest.mark.parametrize("spec", (sb.CAST_TABLE[4:5], sb.CAST_TABLE), ids=("one-entry", "seven-entries"))
def test_cast_table(lib, spec):
    """dl_cast_weights_batched through ops.CastTable: every destination of every entry is the reference, bit for bit what the
    single-matrix entry points write for the same source, and the same again after a second run"""
    from diffulab_amd import ops

    srcs, entries, rows = build_table(spec)
    tab = ops.CastTable(entries)
    assert tab.n == len(spec)
    desc0 = tab.dev.clone()
    snaps = []
    for run in range(2):
        tab.run()
        CALLED.add("dl_cast_weights_batched")
        torch.cuda.synchronize()
        snap = []
        for i, (R, C, src, dests) in enumerate(rows):
            for kind, (G, ld) in dests.items():
                cid = f"cast_table[{i}] {R}x{C} {kind} ld {ld}, run {run}"
                guards_intact(G, cid)
                want = {"dst": sb.plain_bits, "dst_t": sb.transposed_bits, "dst_swiglu": sb.swiglu_bits}[kind](src, ld)
                expect_bits(G, want, cid)
                snap.append(sb.bits16(G.win).clone())
        snaps.append(snap)
    assert all(bool(torch.equal(a, b)) for a, b in zip(*snaps)), "the second run of the table wrote other bits"
    assert bool(torch.equal(tab.dev, desc0)), "the descriptor table was written"
    for i, (S, (R, C, src, dests)) in enumerate(zip(srcs, rows)):
        S.unchanged(f"cast_table[{i}]: src")
        single = {}
        if "dst" in dests or "dst_t" in dests:
            single["dst"], single["dst_t"] = run_cast_weight(lib, S, R, C, dests["dst"][1] if "dst" in dests else None,
                                                             dests["dst_t"][1] if "dst_t" in dests else None, f"cast_table[{i}] single")
        if "dst_swiglu" in dests:
            single["dst_swiglu"] = run_cast_swiglu(lib, S, R // 2, C, dests["dst_swiglu"][1], f"cast_table[{i}] single swiglu")
        for kind, (G, ld) in dests.items():
            assert bool(torch.equal(sb.bits16(G.win), sb.bits16(single[kind].win))), \
                f"cast_table[{i}] {kind}: the table and the single-matrix entry point wrote different bits"
    note("cast_weights_batched_k", 0.0, f"{len(spec)} entries")


def test_cast_table_refuses_ragged_swiglu_rows(lib):
    from diffulab_amd import ops

    src = torch.zeros(48, 8, device=DEV)
    dst = eb.poison_(torch.empty(64, 8, dtype=BF16, device=DEV))
    with pytest.raises(ValueError):
        ops.CastTable([(src, None, None, dst[:48])])
    torch.cuda.synchronize()
    assert bool(eb.is_poison(dst).all())


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_every_entry_point_of_elementwise_hip_is_exercised():
    """runs after the tables (module order): every extern "C" name of csrc/elementwise.hip was called here or is excluded by name"""
    print("\nworst |diff| / bound: " + "; ".join(f"{k} {r:.3f} ({cid})" for k, (r, cid) in sorted(WORST.items())))
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "elementwise.hip")).read()
    names = set(re.findall(r'^extern "C"[^\n]*?\b(dl_\w+)\s*\(', text, flags=re.M))
    assert {"dl_adamw_step", "dl_cast_weights_batched", "dl_flow_add_noise", "dl_sgd_step"} <= names, sorted(names)
    assert EXCLUDED <= names, f"excluded names the file no longer defines: {sorted(EXCLUDED - names)}"
    missing = names - EXCLUDED - CALLED
    assert not missing, f"entry points of elementwise.hip no test of this module called: {sorted(missing)}"
    assert all(r <= 1.0 for r, _ in WORST.values())
