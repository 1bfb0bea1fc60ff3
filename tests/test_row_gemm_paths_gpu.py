"""The row-complete GEMMs (csrc/gemm_ln.hip, csrc/gemm_rows_body.h) element by element against fp64, THROUGH THE C ABI, with write
guards; and the two other producers of the QK statistics, dl_gemm_nt_ssq and dl_gemm_nt_ssq_stationary.

Every case of the tables in tests/row_gemm_bounds.py (D = 384, M = 256 B; B = 8: one tile per workgroup, B = 9: a ragged walk, B = 20
under dl_lab_set_wg_cap(8): walks of 3 and 2 tiles; K from one k-step to 1536; every form of the three entry points)
  * reads A and W at lda = K + 8 with NaN in the gaps and below the last row (the patch-embedding form with K < A's width), its
    modulation rows out of a poisoned [B, 6 D] buffer, every other operand out of an allocation with NaN on both sides,
  * writes every output into a poisoned buffer with guards on both sides, which must come back bit for bit; outputs a form does not
    request are allocated all the same and must come back untouched; q / k rows outside [n_off, n_off + N) keep their poison,
  * is compared element by element with the staged fp64 references and bounds of tests/row_gemm_bounds.py; a failure names the
    workgroup, tile, position in the walk, wave and epilogue step that own the worst element,
  * runs twice and must give the same bits on every output.
The column sums of the backward are written with `=`: their windows start as NaN, so an accumulating kernel fails them.

Worst |out - ref| / bound per mode and output, measured on the MI355X over all cases of the tables (78 tests, 3 s):
    forward   t 0.98   x 1.00   xm 1.00   mean 0.0012   rstd 0.0032
    backward  dx 0.91 (exact product: 1.00)   dt 1.00   dscale 0.21   dshift 0.19   dw 0.18   db 0.19   dgate 0.0015
              exact product, i.e. without the propagated term: dscale 0.0017, dshift 0.0, dw 0.0016, db 0.0005
    QK        qkv 0.96   q 0.99   k 0.99   rrms 0.0032
    ssq       dl_gemm_nt_ssq C 1.00, ssq 0.0081;  dl_gemm_nt_ssq_stationary C 1.00, ssq 0.0071
The bf16 outputs sit at their half ulp: a one-ulp error anywhere in them fails.  The f32 row statistics (mean, rstd, rrms, ssq) and
the f32 column sums (dgate; dscale / dshift / dw / db in the exact-product case) are far below 1: their bounds cannot see a one-ulp
f32 error.  The dominating term is row_bounds' worst-case summation term C * n * 2^-24 of the summed magnitudes (n = 384 columns or
256 rows, any order), where the device adds 8 terms in a lane and then a six-level wave tree, or 32 rows and then 8 slots.  These
bounds see what is structural -- a missing row or slot, a stale operand, a wrong index (tests/test_row_gemm_bounds_host.py rejects
each of them) -- not the last bits.  dscale / dshift / dw / db with random operands reach 0.05 .. 0.21: there the half bf16 ulp of the
unstored d, summed in absolute value over the 256 rows, dominates (the rounding errors themselves add up like a random walk).
"""

from __future__ import annotations

import pytest
import torch

import elementwise_bounds as eb
import row_bounds as rwb
import row_gemm_bounds as rb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
D, BM = rb.D, rb.BM
INVALID, UNSUPPORTED = -1, -3
RATIOS: dict = {}  # (mode, form, exact) -> {output: worst ratio}


@pytest.fixture(scope="module")
def L():
    from diffulab_amd import _lib

    return _lib.lib()


@pytest.fixture
def wg_cap(L):
    """sets the thread's workgroup cap; 0 (no cap) again afterwards"""
    yield lambda n: L.cdll.dl_lab_set_wg_cap(int(n))
    L.cdll.dl_lab_set_wg_cap(0)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _in(v):
    """an operand between two runs of NaN"""
    return None if v is None else rwb.Dense(tuple(v.shape), v.dtype, init=v).t


def _mod(c, names):
    """the modulation rows as views of one poisoned [B, 6 D] buffer (the adaLN output's layout): ld = 6 D"""
    buf = eb.poison_(torch.empty(c["B"], 6 * D, dtype=BF, device=DEV))
    out = {}
    for i, nm in enumerate(names):
        if c.get(nm) is not None:
            out[nm] = buf[:, i * D:(i + 1) * D]
            out[nm].copy_(c[nm])
        else:
            out[nm] = None
    return out


_SETUPS: dict = {}


def _setup(mode, key, exact=False):
    """the case on the device and its operand buffers, built once and left unchanged"""
    k = (mode, key, exact)
    if k not in _SETUPS:
        make = {"fwd": rb.fwd_case, "bwd": rb.bwd_case, "qk": rb.qk_case}[mode]
        c = rb.to(make(*key[:-1], exact=exact), DEV)
        io = dict(A=eb.operand(c["A"], c["A"].shape[1] + 8), W=eb.operand(c["W"], c["W"].shape[1] + 8))
        if mode == "fwd":
            io.update(_mod(c, ("scale", "shift", "gate")), resid=_in(c["resid"]), ln_w=_in(c["ln_w"]), ln_b=_in(c["ln_b"]))
        elif mode == "bwd":
            io.update(_mod(c, ("scale", "-", "gate")), x=_in(c["x"]), dres=_in(c["dres"]), gate_t=_in(c["gate_t"]), ln_w=_in(c["ln_w"]),
                      ln_b=_in(c["ln_b"]), mean=_in(c["mean"]), rstd=_in(c["rstd"]))
        else:
            cos, sin = c["cos"], c["sin"]
            if c["rot"] == 0:  # nothing rotates: the tables must not be read
                cos, sin = eb.poison_(cos.clone()), eb.poison_(sin.clone())
            io.update(sq=_in(c["sq"]), sk=_in(c["sk"]), cos=_in(cos), sin=_in(sin))
        _SETUPS[k] = (c, io)
    return _SETUPS[k]


def _untouched(o, what):
    assert bool(eb.is_poison(o.buf).all()), f"{what}: written although the call did not ask for it"


def _same_bits(a: dict, b: dict, what):
    for nm in a:
        ia, ib = (v.buf.view(torch.int16 if v.buf.dtype == BF else torch.int32) for v in (a[nm], b[nm]))
        assert torch.equal(ia, ib), f"{what}: {nm} differs between two runs"


def _record(c, ratios):
    slot = RATIOS.setdefault((c["mode"], c["form"], c["exact"]), {})
    for nm, v in ratios.items():
        slot[nm] = max(slot.get(nm, 0.0), v)
    print(c["mode"], c["form"], f"B={c['B']} K={c['K']}", "exact" if c["exact"] else "", {k: round(v, 4) for k, v in ratios.items()})


# ------------------------------------------------------------------------------------------------------------------ forward
def fwd_outs(c):
    M = c["M"]
    return dict(t=rwb.Dense((M, D), BF), x=rwb.Dense((M, D), BF), xm=rwb.Dense((M, D), BF), mean=rwb.Dense((M,), F32), rstd=rwb.Dense((M,), F32))


def fwd_call(L, c, io, o, **over):
    a = dict(A=_p(io["A"]), lda=io["A"].stride(0), W=_p(io["W"]), ldw=io["W"].stride(0), M=c["M"], K=c["K"], resid=_p(io["resid"]),
             gate=_p(io["gate"]), ld_gate=6 * D, ln_w=_p(io["ln_w"]), ln_b=_p(io["ln_b"]), scale=_p(io["scale"]), shift=_p(io["shift"]),
             ld_mod=6 * D, rows_per_mod=BM, eps=c["eps"], t_out=_p(o["t"].t) if c["t_out"] else None, x_out=_p(o["x"].t),
             xm_out=_p(o["xm"].t), mean=_p(o["mean"].t), rstd=_p(o["rstd"].t), D=D, stream=_s())
    for k, v in over.items():
        a[k] = v(a[k]) if callable(v) else v
    rc = L.cdll.dl_ln_modulate_gemm_fwd(*a.values())
    torch.cuda.synchronize()
    return rc


def fwd_run(L, c, io, what):
    o = fwd_outs(c)
    rc = fwd_call(L, c, io, o)
    assert rc == 0, L.cdll.dl_last_error().decode()
    for nm, b in o.items():
        if nm == "t" and not c["t_out"]:
            _untouched(b, what + " t")
        else:
            b.check(f"{what} {nm}")
    return o


def _fwd_test(L, wg_cap, key, exact=False):
    c, io = _setup("fwd", key, exact)
    cap = key[-1]
    wg_cap(cap)
    what = f"fwd {key}"
    o, o2 = fwd_run(L, c, io, what), fwd_run(L, c, io, what)
    _same_bits(o, o2, what)
    got = dict(t=o["t"].t if c["t_out"] else None, x=o["x"].t, xm=o["xm"].t, mean=o["mean"].t, rstd=o["rstd"].t)
    _record(c, rb.check_fwd(c, got, rb.locator(c["M"], 1, c["K"], _n_cu(), cap)))


@pytest.mark.parametrize("key", rb.FWD_CASES, ids=lambda k: f"B{k[0]}-K{k[1]}-{k[2]}-cap{k[3]}")
def test_ln_modulate_gemm_fwd(L, wg_cap, key):
    _fwd_test(L, wg_cap, key)


def test_ln_modulate_gemm_fwd_exact_product(L, wg_cap):
    _fwd_test(L, wg_cap, rb.FWD_EXACT, exact=True)


# ------------------------------------------------------------------------------------------------------------------ backward
def bwd_outs(c):
    M, B = c["M"], c["B"]
    return dict(dx=rwb.Dense((M, D), BF), dt=rwb.Dense((M, D), BF), dwb=rwb.Dense((B, 2, D), F32), dmod=eb.Guarded(B, 3 * D, F32, DEV))


def bwd_call(L, c, io, o, **over):
    gated, win = c["gate_t"] is not None, o["dmod"].win
    a = dict(A=_p(io["A"]), lda=io["A"].stride(0), Wt=_p(io["W"]), ldw=io["W"].stride(0), M=c["M"], K=c["K"], x=_p(io["x"]), ln_w=_p(io["ln_w"]),
             ln_b=_p(io["ln_b"]), scale=_p(io["scale"]), ld_mod=6 * D, rows_per_mod=BM, mean=_p(io["mean"]), rstd=_p(io["rstd"]),
             dres=_p(io["dres"]), dx=_p(o["dx"].t), dscale=_p(win[:, :D]), dshift=_p(win[:, D:2 * D]), ld_dmod=o["dmod"].buf.stride(0),
             dwb=_p(o["dwb"].t) if c["dwb"] else None, gate_t=_p(io["gate_t"]), gate=_p(io["gate"]), ld_gate=6 * D,
             dt=_p(o["dt"].t) if gated else None, dgate=_p(win[:, 2 * D:]) if gated else None, D=D, stream=_s())
    for k, v in over.items():
        a[k] = v(a[k]) if callable(v) else v
    rc = L.cdll.dl_ln_modulate_gemm_bwd(*a.values())
    torch.cuda.synchronize()
    return rc


def bwd_run(L, c, io, what):
    o = bwd_outs(c)
    rc = bwd_call(L, c, io, o)
    assert rc == 0, L.cdll.dl_last_error().decode()
    gated, dm = c["gate_t"] is not None, o["dmod"]
    o["dx"].check(what + " dx")
    o["dt"].check(what + " dt") if gated else _untouched(o["dt"], what + " dt")
    o["dwb"].check(what + " dwb") if c["dwb"] else _untouched(o["dwb"], what + " dwb")
    hit = dm.mask & ~eb.is_poison(dm.buf)
    assert not bool(hit.any()), what + ": guard of the modulation-gradient rows written"
    # written with `=` over NaN: an accumulating kernel leaves NaN here
    assert bool(torch.isfinite(dm.win[:, :(3 if gated else 2) * D]).all()), what + ": dscale / dshift / dgate unwritten or accumulated"
    if not gated:
        assert bool(eb.is_poison(dm.win[:, 2 * D:]).all()), what + ": dgate written without the gate backward"
    return o


def _bwd_test(L, wg_cap, key, exact=False):
    c, io = _setup("bwd", key, exact)
    cap = key[-1]
    wg_cap(cap)
    what = f"bwd {key}"
    o, o2 = bwd_run(L, c, io, what), bwd_run(L, c, io, what)
    _same_bits(o, o2, what)
    gated, win = c["gate_t"] is not None, o["dmod"].win
    got = dict(dx=o["dx"].t, dscale=win[:, :D], dshift=win[:, D:2 * D], dwb=o["dwb"].t if c["dwb"] else None, dt=o["dt"].t if gated else None,
               dgate=win[:, 2 * D:] if gated else None)
    _record(c, rb.check_bwd(c, got, rb.locator(c["M"], 1, c["K"], _n_cu(), cap)))


@pytest.mark.parametrize("key", rb.BWD_CASES, ids=lambda k: f"B{k[0]}-K{k[1]}-{k[2]}-cap{k[3]}")
def test_ln_modulate_gemm_bwd(L, wg_cap, key):
    _bwd_test(L, wg_cap, key)


def test_ln_modulate_gemm_bwd_exact_product(L, wg_cap):
    """the GEMM term is zero: the epilogue is judged at the row kernels' own bounds, without the propagated term"""
    _bwd_test(L, wg_cap, rb.BWD_EXACT, exact=True)


# ------------------------------------------------------------------------------------------------------------------ QK
def qk_outs(c):
    shape = (c["B"], c["H"], c["n_dst"], c["dh"])
    return dict(qkv=rwb.Dense((c["M"], 3 * D), BF), q=rwb.Dense(shape, BF), k=rwb.Dense(shape, BF), rrms=rwb.Dense((c["M"], 2), F32))


def qk_call(L, c, io, o, **over):
    a = dict(A=_p(io["A"]), lda=io["A"].stride(0), Wqkv=_p(io["W"]), ldw=io["W"].stride(0), B=c["B"], N=c["N"], H=c["H"], dh=c["dh"],
             rot=c["rot"], eps=c["eps"], scale_q=_p(io["sq"]), scale_k=_p(io["sk"]), cos=_p(io["cos"]), sin=_p(io["sin"]), qkv=_p(o["qkv"].t),
             q=_p(o["q"].t), k=_p(o["k"].t), rrms=_p(o["rrms"].t), n_dst=c["n_dst"], n_off=c["n_off"], stream=_s())
    for k, v in over.items():
        a[k] = v(a[k]) if callable(v) else v
    rc = L.cdll.dl_gemm_nt_qk_norm_rope(*a.values())
    torch.cuda.synchronize()
    return rc


def qk_run(L, c, io, what):
    o = qk_outs(c)
    rc = qk_call(L, c, io, o)
    assert rc == 0, L.cdll.dl_last_error().decode()
    o["qkv"].check(what + " qkv")
    o["rrms"].check(what + " rrms")
    o["q"].check(what + " q", finite=False)  # (the window and the poison around it: rb.check_qk)
    o["k"].check(what + " k", finite=False)
    return o


def _qk_test(L, wg_cap, key, exact=False):
    c, io = _setup("qk", key, exact)
    cap = key[-1]
    wg_cap(cap)
    what = f"qk {key}"
    o, o2 = qk_run(L, c, io, what), qk_run(L, c, io, what)
    _same_bits(o, o2, what)
    _record(c, rb.check_qk(c, {k: v.t for k, v in o.items()}, rb.locator(c["M"], 3, c["K"], _n_cu(), cap)))


@pytest.mark.parametrize("key", rb.QK_CASES, ids=lambda k: f"B{k[0]}-N{k[1]}-H{k[2]}-rot{k[4]}-off{k[5]}-cap{k[7]}")
def test_gemm_nt_qk_norm_rope(L, wg_cap, key):
    _qk_test(L, wg_cap, key)


def test_gemm_nt_qk_norm_rope_exact_product(L, wg_cap):
    _qk_test(L, wg_cap, rb.QK_EXACT, exact=True)


# ------------------------------------------------------------------------------------------------------------------ refusals
def _off(nbytes):
    return lambda p: p + nbytes


FWD_REFUSALS = [("D", 512, UNSUPPORTED), ("M", 7 * BM, UNSUPPORTED), ("K", 96, UNSUPPORTED), ("rows_per_mod", 128, UNSUPPORTED),
                ("ld_mod", 6 * D + 4, INVALID), ("resid", None, INVALID), ("x_out", None, INVALID)] + [
    (nm, _off(4 if nm.startswith("ln_") else 2), INVALID) for nm in ("A", "W", "resid", "gate", "scale", "shift", "t_out", "x_out", "xm_out", "ln_w", "ln_b")]
BWD_REFUSALS = [("D", 512, UNSUPPORTED), ("M", 7 * BM, UNSUPPORTED), ("K", 96, UNSUPPORTED), ("rows_per_mod", 128, UNSUPPORTED),
                ("ld_mod", 6 * D + 4, INVALID)] + [
    (nm, _off(4 if nm.startswith("ln_") else 2), INVALID) for nm in ("A", "Wt", "x", "scale", "dres", "dx", "gate_t", "gate", "dt", "ln_w")]
QK_REFUSALS = [("H", 8, UNSUPPORTED), ("B", 7, UNSUPPORTED), ("rot", 72, UNSUPPORTED), ("n_dst", 255 + 77, INVALID), ("n_off", -8, INVALID)] + [
    (nm, _off(4 if nm in ("scale_q", "scale_k", "cos", "sin") else 2), INVALID) for nm in ("A", "Wqkv", "qkv", "q", "k", "scale_q", "scale_k", "cos", "sin")]


def _rid(v):
    return v if isinstance(v, str) else ("misaligned" if callable(v) else str(v))


def _refused(L, rc, want, o, name):
    assert rc == want, (rc, L.cdll.dl_last_error().decode())
    assert name in L.cdll.dl_last_error().decode()
    for nm, b in o.items():
        assert bool(eb.is_poison(b.buf).all()), f"a refused call wrote to {nm}"


@pytest.mark.parametrize("arg,value,want", FWD_REFUSALS, ids=_rid)
def test_fwd_refusals_write_nothing(L, arg, value, want):
    """(the base call is the smallest block form, which passes in test_ln_modulate_gemm_fwd's table at K = 384)"""
    c, io = _setup("fwd", (8, 64, "block", 0))
    o = fwd_outs(c)
    _refused(L, fwd_call(L, c, io, o, **{arg: value}), want, o, "dl_ln_modulate_gemm_fwd")


@pytest.mark.parametrize("arg,value,want", BWD_REFUSALS, ids=_rid)
def test_bwd_refusals_write_nothing(L, arg, value, want):
    c, io = _setup("bwd", (8, 64, "full", 0))
    o = bwd_outs(c)
    _refused(L, bwd_call(L, c, io, o, **{arg: value}), want, o, "dl_ln_modulate_gemm_bwd")


@pytest.mark.parametrize("arg,value,want", QK_REFUSALS, ids=_rid)
def test_qk_refusals_write_nothing(L, arg, value, want):
    c, io = _setup("qk", (8, 256, 6, 64, 64, 77, 356, 0))
    o = qk_outs(c)
    _refused(L, qk_call(L, c, io, o, **{arg: value}), want, o, "dl_gemm_nt_qk_norm_rope")


# ------------------------------------------------------------------------------------------------------------------ dl_gemm_nt_ssq
def _ssq_window(M, tiles, init=None):
    """ssq [M, tiles] is dense (its row stride is ssq_tiles): guard rows above and below"""
    return eb.Guarded(M, tiles, F32, DEV, left=0, right=0, top=16, bottom=16, ld=tiles, init=init)


def _ssq_operands(M, N, K, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = (torch.randn(M, K, generator=g, device=DEV)).to(BF)
    w = (torch.randn(N, K, generator=g, device=DEV) * K**-0.5).to(BF)
    return eb.operand(a, K + 8), eb.operand(w, K + 8)


# dl_gemm_nt_ssq wants (M / 256) * (N / 384) >= 64 tiles (gemm.hip): 8 x 8 tiles at the smallest M, and the qkv shape N = 3 D at its own
@pytest.mark.parametrize("M,N,K,tiles", [(2048, 3072, 128, 2), (5632, 1152, 384, 2), (2048, 3072, 64, 8)])
def test_gemm_nt_ssq_against_fp64(L, M, N, K, tiles):
    a, w = _ssq_operands(M, N, K, 7)
    runs = []
    for _ in range(2):
        Cw = eb.Guarded(M, N, BF, DEV)
        S = _ssq_window(M, tiles, init=torch.zeros(M, tiles, device=DEV))  # (atomic adds: the caller zero-fills)
        L.call("dl_gemm_nt_ssq", _p(a), a.stride(0), _p(w), w.stride(0), _p(Cw.win), Cw.buf.stride(0), M, N, K, _p(S.win), tiles, _s())
        torch.cuda.synchronize()
        Cw.check("C")
        S.check("ssq")
        runs.append((Cw, S))
    assert torch.equal(runs[0][0].buf.view(torch.int16), runs[1][0].buf.view(torch.int16))
    r = rb.check_ssq(a, w, runs[0][0].win, runs[0][1].win, tiles, f"dl_gemm_nt_ssq {M}x{N}x{K}")
    _record(dict(mode="ssq", form="tiles", exact=False, B=M // BM, K=K), r)
    # fewer than 64 tiles: declined, nothing written
    Cw, S = eb.Guarded(M - 256, N, BF, DEV), _ssq_window(M - 256, tiles)
    rc = L.cdll.dl_gemm_nt_ssq(_p(a), a.stride(0), _p(w), w.stride(0), _p(Cw.win), Cw.buf.stride(0), M - 256, N, K, _p(S.win), tiles, _s())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and bool(eb.is_poison(Cw.buf).all()) and bool(eb.is_poison(S.buf).all())


# the stationary form: whole 256-row panels, N % 128 == 0, K <= 512; max_workgroups > 0 sizes the grid (st_grid, gemm_stationary.hip)
@pytest.mark.parametrize("M,N,K,tiles,wgs", [(256, 128, 64, 1, 1), (256, 1152, 384, 2, 1), (768, 512, 192, 2, 2), (512, 1152, 512, 3, 2)])
def test_gemm_nt_ssq_stationary_against_fp64(L, M, N, K, tiles, wgs):
    a, w = _ssq_operands(M, N, K, 9)
    runs = []
    for _ in range(2):
        Cw = eb.Guarded(M, N, BF, DEV)
        S = _ssq_window(M, tiles)  # plain stores: over NaN
        rc = L.cdll.dl_gemm_nt_ssq_stationary(_p(a), a.stride(0), _p(w), w.stride(0), _p(Cw.win), Cw.buf.stride(0), M, N, K, _p(S.win),
                                              tiles, wgs, _s())
        torch.cuda.synchronize()
        assert rc == 0, L.cdll.dl_last_error().decode()
        Cw.check("C")
        S.check("ssq")
        runs.append((Cw, S))
    assert torch.equal(runs[0][0].buf.view(torch.int16), runs[1][0].buf.view(torch.int16))
    assert torch.equal(runs[0][1].buf.view(torch.int32), runs[1][1].buf.view(torch.int32))
    r = rb.check_ssq(a, w, runs[0][0].win, runs[0][1].win, tiles, f"dl_gemm_nt_ssq_stationary {M}x{N}x{K}")
    _record(dict(mode="ssq", form="stationary", exact=False, B=M // BM, K=K), r)


# ------------------------------------------------------------------------------------------------------------------ closing
def test_every_mode_and_form_was_reached_within_its_bound():
    want = {("fwd", f, False) for f in rb.FWD_FORMS} | {("bwd", f, False) for f in rb.BWD_FORMS} | {
        ("qk", f"N{k[1]} H{k[2]} rot{k[4]} off{k[5]}", False) for k in rb.QK_CASES} | {
        ("fwd", "block", True), ("bwd", "full", True), ("qk", "N256 H6 rot64 off77", True), ("ssq", "tiles", False), ("ssq", "stationary", False)}
    for k in sorted(RATIOS):
        print(k, {n: round(v, 4) for n, v in RATIOS[k].items()})
    assert want <= set(RATIOS), sorted(want - set(RATIOS))
    outs = {"fwd": {"t", "x", "xm", "mean", "rstd"}, "bwd": {"dx", "dscale", "dshift", "dw", "db", "dt", "dgate"},
            "qk": {"qkv", "rrms", "q", "k"}, "ssq": {"C", "ssq"}}
    for mode, names in outs.items():
        seen = set().union(*(RATIOS[k] for k in RATIOS if k[0] == mode))
        assert seen == names, (mode, seen ^ names)
    worst = {k: max(v.values()) for k, v in RATIOS.items()}
    assert all(v <= 1.0 for v in worst.values()), worst
