"""Every fp32-regime kernel of csrc/f32.hip, element by element, with write guards.

Tables of cases drive every dl_f32_* entry point through the C ABI (and the four attention composites of diffulab_amd.ops).  A case
  * asserts the kernel form it was built to reach where the entry point has more than one (dl_lab_last_f32_path, csrc/f32_paths.h),
  * compares every element of every output with the fp64 reference within its bound, or bit for bit where the kernel only moves data
    (tests/f32_bounds.py; test_f32_bounds_host.py shows what the bounds admit and reject),
  * writes into poisoned allocations with guards around the window (leading dimension above the width wherever the entry point takes
    one) and reads operands from allocations that end in NaN, so a read past a row or past the last row shows.
The last tests assert that every path code was reached, that PATHS mirrors the header and that every dl_f32_* entry point was called.
"""

from __future__ import annotations

import ctypes
import os
import re
import zlib

import pytest
import torch

import elementwise_bounds as eb
import f32_bounds as fb

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024  # poisoned elements on each side of a dense output

# mirror of enum DlF32Path (diffulab_amd/csrc/f32_paths.h), by name: index = code
PATHS = ["DL_F32_PATH_NONE", "F32_GEMM_SCALAR", "F32_GEMM_VEC", "F32_GEMM_SCALAR_SPLITK", "F32_GEMM_VEC_SPLITK", "F32_SOFTMAX_FWD_VEC",
         "F32_SOFTMAX_FWD_ANY", "F32_SOFTMAX_BWD_VEC", "F32_SOFTMAX_BWD_ANY", "F32_SOFTMAX_KEYMASK"]
REACHED: set[str] = set()
CALLED: set[str] = set()
WORST: dict[str, tuple[float, str]] = {}


# ------------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    L = _lib.lib()
    L.cdll.dl_lab_last_f32_path.restype = ctypes.c_int
    return L


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def call(L, name, *args):
    CALLED.add(name)
    return L.call(name, *args)


def path(L):
    code = L.cdll.dl_lab_last_f32_path()
    name = PATHS[code] if 0 <= code < len(PATHS) else f"<{code}>"
    REACHED.add(name)
    return name


def gen_for(cid: str):
    g = torch.Generator(device=DEV)
    g.manual_seed(zlib.crc32(cid.encode()))
    return g


class Flat:
    """a dense tensor between two runs of GUARD poisoned elements, `shift` floats off the 16-byte grid (init None: starts poisoned)"""

    def __init__(self, shape, init=None, shift=0, dtype=F32):
        n = 1
        for s in shape:
            n *= s
        self.buf = eb.poison_(torch.empty(n + 2 * GUARD + shift, dtype=dtype, device=DEV))
        self.t = self.buf[GUARD + shift:GUARD + shift + n].view(*shape)
        self.lo, self.hi = GUARD + shift, GUARD + shift + n
        if init is not None:
            self.t.copy_(init)

    def check(self, what, finite=True):
        assert bool(eb.is_poison(self.buf[:self.lo]).all()) and bool(eb.is_poison(self.buf[self.hi:]).all()), f"{what}: guard written"
        if finite:
            assert bool(torch.isfinite(self.t.float()).all()), f"{what}: unwritten or non-finite elements"


def win(rows, cols, pad=8, init=None):
    """an output window with guard columns on both sides (ld = 8 + cols + pad rounded to 8: rows stay 16-byte aligned)"""
    return eb.Guarded(rows, cols, F32, DEV, left=8, right=pad, init=init)


def opnd(t, pad=4, col0=0):
    """a 2-D operand with leading dimension cols + pad inside a poisoned allocation that ends in NaN rows"""
    return eb.operand(t.contiguous(), t.shape[1] + pad + col0, col0=col0)


def dense(t):
    """a dense operand of any shape followed by NaN rows"""
    t = t.contiguous()
    return eb.operand(t.reshape(-1, t.shape[-1]), t.shape[-1]).view(t.shape)


def settle(cid, got: dict, ref: dict, guards=()):
    """guards intact, then every output inside its bound (or bit-identical); keeps the worst ratio per output for the report"""
    torch.cuda.synchronize()
    for g, what in guards:
        g.check(f"{cid}: {what}")
    ratios = fb.judge(got, ref)
    print(f"{cid}: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    for k, v in ratios.items():
        key = f"{cid.split('-')[0]}.{k}"
        if v > WORST.get(key, (-1.0, ""))[0]:
            WORST[key] = (v, cid)
    for k, (r, bound) in ref.items():
        if bound is None:
            assert ratios[k] == 0.0, f"{cid}: {k} is not bit-identical to the reference"
        else:
            g2, r2, b2 = (t.reshape(-1, t.shape[-1]) for t in (got[k], r, bound))
            eb.assert_within(g2, r2, b2, what=f"{cid}: {k}")
    assert all(v <= 1.0 for v in ratios.values()), (cid, ratios)


# ------------------------------------------------------------------------------------------------------------------ GEMM
def _gemm_cases():
    cs = []
    for (M, N, K) in ((1, 1, 1), (128, 128, 16), (129, 127, 17), (132, 124, 20), (260, 36, 1028)):
        for ta in (0, 1):
            for tb in (0, 1):
                cs.append(dict(M=M, N=N, K=K, ta=ta, tb=tb))
    al = dict(M=132, N=124, K=20)
    cs += [dict(al, ta=0, tb=0, pad=3), dict(al, ta=1, tb=1, pad=3), dict(al, ta=0, tb=0, pad=3, off=1),
           dict(al, ta=1, tb=0, pad=3, off=1)]  # (pad 3 + offset 1: ld % 4 == 0, only the base is off the 16-byte grid)
    # epilogue, direct and through the fold
    for extra in (dict(), dict(K=1040, scratch="ample")):
        base = dict(al, ta=0, tb=0, **extra)
        cs += [dict(base, alpha=0.37), dict(base, bias=1), dict(base, bias=1, silu=1, pre=1), dict(base, acc=1, alpha=-1.5, bias=1)]
    # split-K: last split shorter (1040 = 3 x 272 + 224), scalar + split (2050), exactly two images, below two images
    for ta, tb in ((0, 0), (1, 1), (0, 1), (1, 0)):
        cs.append(dict(M=260, N=36, K=1040, ta=ta, tb=tb, scratch="ample"))
    cs += [dict(M=260, N=36, K=2050, ta=0, tb=0, scratch="ample"), dict(M=260, N=36, K=2050, ta=1, tb=1, scratch="ample", acc=1),
           dict(M=132, N=124, K=1040, ta=0, tb=0, scratch="two"), dict(M=129, N=127, K=2050, ta=0, tb=1, scratch="two", bias=1),
           dict(M=132, N=124, K=1040, ta=0, tb=0, scratch="one"), dict(M=132, N=124, K=1040, ta=1, tb=1)]
    for c in cs:
        c["id"] = "gemm-" + "-".join(f"{k}{v}" for k, v in c.items())
    return cs


GEMM_CASES = _gemm_cases()


def _gemm_desc(A, B, C, lda, ldb, ldc, M, N, K, ta, tb, batch=(1, 1), sa=(0, 0), sb=(0, 0), sc=(0, 0), alpha=1.0, bias=None, act=0,
               pre=None, acc=0, scratch=None, scratch_floats=0):
    from diffulab_amd.ops import _F32Gemm

    return _F32Gemm(_p(A), _p(B), _p(C), lda, ldb, ldc, M, N, K, ta, tb, batch[0], batch[1], sa[0], sa[1], sb[0], sb[1], sc[0], sc[1],
                    float(alpha), _p(bias), act, _p(pre), acc, _p(scratch), scratch_floats)


def run_gemm(L, c):
    M, N, K, ta, tb = c["M"], c["N"], c["K"], c["ta"], c["tb"]
    pad, off = c.get("pad", 4), c.get("off", 0)
    g = gen_for(c["id"])
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    a, b = n(M, K), n(N, K)
    A = opnd(a.t() if ta else a, pad=pad, col0=off)
    B = opnd(b.t() if tb else b, pad=pad, col0=off)
    bias = n(N) if c.get("bias") else None
    c0 = n(M, N) if c.get("acc") else None
    alpha = c.get("alpha", 1.0)
    Cw = win(M, N, init=c0)
    Pw = win(M, N) if c.get("pre") else None
    mode = c.get("scratch")
    floats = {"ample": 64 * M * N, "two": 2 * M * N, "one": 2 * M * N - 1, None: 0}[mode]
    scr = Flat((floats,)) if mode else None
    d = _gemm_desc(A, B, Cw.win, A.stride(0), B.stride(0), Cw.win.stride(0), M, N, K, ta, tb, alpha=alpha, bias=dense(bias[None])[0]
                   if bias is not None else None, act=1 if c.get("silu") else 0, pre=Pw.win if Pw else None, acc=int(bool(c.get("acc"))),
                   scratch=scr.t if scr else None, scratch_floats=floats)
    call(L, "dl_f32_gemm", ctypes.addressof(d), _s())
    vec = (pad + off) % 4 == 0 and off == 0 and (M if ta else K) % 4 == 0 and (N if tb else K) % 4 == 0
    tiles = -(-M // 128) * -(-N // 128)
    split = mode in ("ample", "two") and tiles < 768 and K >= 1024
    want = ("F32_GEMM_VEC" if vec else "F32_GEMM_SCALAR") + ("_SPLITK" if split else "")
    got_path = path(L)
    assert got_path == want, f"{c['id']}: took {got_path}, expected {want}"
    ref = fb.gemm_ref(a, b, alpha, bias, bool(c.get("silu")), c0, bool(c.get("pre")))
    got = {"C": Cw.win}
    guards = [(Cw, "C")]
    if Pw:
        got["pre_out"] = Pw.win
        guards.append((Pw, "pre_out"))
    torch.cuda.synchronize()
    if scr:
        scr.check(f"{c['id']}: scratch", finite=False)
    settle(c["id"], got, ref, guards)
    return Cw.win.clone()


@pytest.mark.parametrize("case", GEMM_CASES, ids=[c["id"] for c in GEMM_CASES])
def test_gemm(lib, case):
    first = run_gemm(lib, case)
    if case.get("scratch"):
        assert fb.same_bits(first, run_gemm(lib, case)), f"{case['id']}: two runs differ"


def test_gemm_batched_pre_out(lib):
    """two-level batch with batch strides on A, B, C and pre_out (SiLU after it)"""
    b1, b2, M, N, K = 2, 3, 37, 20, 12
    g = gen_for("gemm-batched")
    a, b, bias = (torch.randn(s, generator=g, device=DEV) for s in ((b1, b2, M, K), (b1, b2, N, K), (N,)))
    A, B = dense(a), dense(b)
    Cw, Pw = Flat((b1, b2, M, N)), Flat((b1, b2, M, N))
    d = _gemm_desc(A, B, Cw.t, K, K, N, M, N, K, 0, 0, batch=(b1, b2), sa=(b2 * M * K, M * K), sb=(b2 * N * K, N * K),
                   sc=(b2 * M * N, M * N), bias=bias, act=1, pre=Pw.t)
    call(lib, "dl_f32_gemm", ctypes.addressof(d), _s())
    assert path(lib) == "F32_GEMM_VEC"
    for i in range(b1):
        for j in range(b2):
            settle(f"gemm-batched-{i}{j}", {"C": Cw.t[i, j], "pre_out": Pw.t[i, j]}, fb.gemm_ref(a[i, j], b[i, j], 1.0, bias, True, None, True),
                   [(Cw, "C"), (Pw, "pre_out")])


# ------------------------------------------------------------------------------------------------------------------ LayerNorm + modulate
# flags: w affine, g gated residual (t / gate / x_out; the gate backward), r dres, p dwb partials
def _ln_cases():
    cs = []
    flags = ["wgrp", "", "wr", "g", "wp", "gr", "wg"]
    for i, D in enumerate((4, 252, 256, 260, 384, 1020, 1024)):
        cs.append(dict(D=D, rpm=13, G=3, cls=fb.ROW_CLASSES[i % 3], f=flags[i]))
    cs += [dict(D=260, rpm=1, G=5, cls="offset32", f="wgrp"), dict(D=1024, rpm=13, G=3, cls="const", f="wgrp"),
           dict(D=64, rpm=4100, G=4, cls="scaled", f="w", fwd_only=1), dict(D=260, rpm=13, G=3, cls="const", f="")]
    for c in cs:
        c["id"] = f"ln-D{c['D']}-r{c['rpm']}x{c['G']}-{c['cls']}-{c['f'] or 'plain'}"
    return cs


LN_CASES = _ln_cases()


@pytest.mark.parametrize("case", LN_CASES, ids=[c["id"] for c in LN_CASES])
def test_ln_modulate(lib, case):
    c, L = case, lib
    D, rpm, G, f = c["D"], c["rpm"], c["G"], c["f"]
    M = rpm * G
    g = gen_for(c["id"])
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    x = dense(fb.row_input(c["cls"], M, D, g, DEV))
    w, b = (dense((1.0 + 0.2 * n(1, D)))[0], dense(0.2 * n(1, D))[0]) if "w" in f else (None, None)
    mod = eb.operand(0.3 * n(G, 6 * D), 6 * D)  # ld_mod = 6 D: the six slices of one modulation row
    shift, scale, gate = mod[:, 0:D], mod[:, D:2 * D], mod[:, 2 * D:3 * D]
    t = dense(n(M, D)) if "g" in f else None
    outw, mean, rstd = Flat((M, D)), Flat((M,)), Flat((M,))
    xo = Flat((M, D)) if t is not None else None
    call(L, "dl_f32_ln_modulate_fwd", _p(x), _p(w), _p(b), _p(scale), _p(shift), 6 * D, rpm, fb.LN_EPS, _p(outw.t), _p(mean.t), _p(rstd.t),
         _p(t), _p(gate if t is not None else None), 6 * D, _p(xo.t if xo else None), M, D, _s())
    ref = fb.ln_fwd_ref(x, w, b, scale, shift, rpm, fb.LN_EPS, t, gate if t is not None else None)
    got = {"out": outw.t, "mean": mean.t, "rstd": rstd.t}
    guards = [(outw, "out"), (mean, "mean"), (rstd, "rstd")]
    if xo:
        got["x_out"] = xo.t
        guards.append((xo, "x_out"))
    settle(c["id"] + "-fwd", got, ref, guards)
    if c.get("fwd_only"):
        return
    xin = dense(xo.t.clone()) if xo else x
    dout = dense(n(M, D))
    dres = dense(n(M, D)) if "r" in f else None
    dx = Flat((M, D))
    dmod = win(G, 3 * D)  # dshift | dscale | dgate as column windows of one guarded allocation, ld_dmod > 3 D
    dshift, dscale, dgate = dmod.win[:, 0:D], dmod.win[:, D:2 * D], dmod.win[:, 2 * D:3 * D]
    if t is None:
        dgate.zero_()
    dwb = Flat((G, 2, D)) if "p" in f else None
    dt = Flat((M, D)) if t is not None else None
    call(L, "dl_f32_ln_modulate_bwd", _p(dout), _p(xin), _p(w), _p(b), _p(scale), 6 * D, rpm, _p(mean.t), _p(rstd.t), _p(dres), _p(dx.t),
         _p(dscale), _p(dshift), dmod.win.stride(0), _p(dwb.t if dwb else None), _p(t), _p(gate if t is not None else None), 6 * D,
         _p(dt.t if dt else None), _p(dgate if t is not None else None), M, D, _s())
    ref = fb.ln_bwd_ref(dout, xin, w, b, scale, rpm, mean.t, rstd.t, dres, dwb is not None, t, gate if t is not None else None)
    got = {"dx": dx.t, "dscale": dscale, "dshift": dshift}
    guards = [(dx, "dx"), (dmod, "dmod")]
    for name, o in (("dwb", dwb), ("dt", dt)):
        if o:
            got[name] = o.t
            guards.append((o, name))
    if t is not None:
        got["dgate"] = dgate
    settle(c["id"] + "-bwd", got, ref, guards)


def test_ln_modulate_refuses_wide_rows(lib):
    D, M = 1028, 2
    z = torch.zeros(M, D, device=DEV)
    v = torch.zeros(M, device=DEV)
    with pytest.raises(RuntimeError):
        call(lib, "dl_f32_ln_modulate_fwd", _p(z), None, None, _p(z), _p(z), D, 1, 1e-6, _p(z.clone()), _p(v), _p(v.clone()), None, None, 0,
             None, M, D, _s())
    with pytest.raises(RuntimeError):
        call(lib, "dl_f32_ln_modulate_bwd", _p(z), _p(z), None, None, _p(z), D, 1, _p(v), _p(v), None, _p(z.clone()), _p(z.clone()),
             _p(z.clone()), D, None, None, None, 0, None, None, M, D, _s())


# ------------------------------------------------------------------------------------------------------------------ QK-RMSNorm + RoPE
def _qk_cases():
    cs = []
    for i, (H, dh) in enumerate(((1, 4), (2, 64), (6, 64), (16, 64), (3, 84))):
        for j, rot in enumerate(sorted({0, (dh // 2 + 3) // 4 * 4, dh})):
            cs.append(dict(H=H, dh=dh, rot=rot, pos=(i + j) % 2, wide=(i + j) % 2 == 0))
    for c in cs:
        c["id"] = f"qk-H{c['H']}-dh{c['dh']}-rot{c['rot']}-pos{c['pos']}-w{int(c['wide'])}"
    return cs


QK_CASES = _qk_cases()


@pytest.mark.parametrize("case", QK_CASES, ids=[c["id"] for c in QK_CASES])
def test_qk_norm_rope(lib, case):
    c, L = case, lib
    H, dh, rot, B, N = c["H"], c["dh"], c["rot"], 2, 13
    D, M = H * dh, 2 * 13
    g = gen_for(c["id"])
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    qkv = eb.operand(n(M, 3 * D) * (0.5 + torch.rand(1, 3 * D, generator=g, device=DEV)), 3 * D + 8)
    sq, sk = dense(1.0 + 0.2 * n(1, D))[0], dense(1.0 + 0.2 * n(1, D))[0]
    T = 19  # rows of the rotary table
    cs, sn = fb.rope_tables(T, rot, g, DEV)
    cs, sn = (dense(cs), dense(sn)) if rot else (None, None)
    if c["pos"]:  # repeats and out-of-order rows
        pos = torch.randint(0, T, (M,), generator=g, device=DEV, dtype=torch.int32)
        pos[1], pos[2] = pos[0], T - 1
        tok = pos.long()
    else:
        pos, tok = None, torch.arange(M, device=DEV) % N
    qk, rr = Flat((M, 2 * D)), Flat((M, 2))
    call(L, "dl_f32_qk_norm_rope_fwd", _p(qkv), 3 * D + 8, _p(sq), _p(sk), _p(cs), _p(sn), _p(qk.t), _p(rr.t), B, N, H, dh, rot, fb.QK_EPS,
         _p(pos), _s())
    settle(c["id"] + "-fwd", {"qk": qk.t, "rrms": rr.t}, fb.qk_fwd_ref(qkv, sq, sk, cs, sn, tok, H, dh, rot, fb.QK_EPS), [(qk, "qk"), (rr, "rrms")])
    dqk = dense(n(M, 2 * D))
    ld_d = (3 * D if c["wide"] else 2 * D) + 4  # wide: the V columns and the pad stay poison
    dq = eb.Guarded(M, 2 * D, F32, DEV, left=0, ld=ld_d)
    part = Flat((B, 2, D))
    call(L, "dl_f32_qk_norm_rope_bwd", _p(dqk), _p(qkv), 3 * D + 8, _p(sq), _p(sk), _p(cs), _p(sn), _p(rr.t), _p(dq.win), ld_d, _p(part.t), B,
         N, H, dh, rot, _p(pos), _s())
    ref = fb.qk_bwd_ref(dqk, qkv, sq, sk, cs, sn, tok, rr.t, B, N, H, dh, rot)
    settle(c["id"] + "-bwd", {"dqk_in": dq.win, "dscale": part.t}, ref, [(dq, "dqkv"), (part, "dscale")])


# ------------------------------------------------------------------------------------------------------------------ softmax
def _scores(rows, cols, g):
    s = 3.0 * torch.randn(rows, cols, generator=g, device=DEV)
    if rows >= 3:
        s[0, cols // 2] += 80.0                      # a spike
        s[1, ::3] = float("-inf")                    # some -inf (never the whole row: column 1 % cols stays)
        s[1, 1 % cols] = 0.5
        s[2] = -1.0e4                                # far below zero throughout
    return s


SOFTMAX_CASES = [dict(rows=7, cols=c, shift=0) for c in (1, 3, 4, 9, 25, 252, 256, 260, 4092, 4096, 4100)] + \
                [dict(rows=7, cols=256, shift=1), dict(rows=65540, cols=4, shift=0)]


@pytest.mark.parametrize("case", SOFTMAX_CASES, ids=[f"softmax-r{c['rows']}-c{c['cols']}-s{c['shift']}" for c in SOFTMAX_CASES])
def test_softmax(lib, case):
    rows, cols, shift = case["rows"], case["cols"], case["shift"]
    cid = f"softmax-r{rows}-c{cols}-s{shift}"
    g = gen_for(cid)
    s = _scores(rows, cols, g)
    vec = cols % 4 == 0 and cols <= 4096 and shift == 0
    sw = Flat((rows, cols), init=s, shift=shift)
    call(lib, "dl_f32_softmax_fwd", _p(sw.t), rows, cols, _s())
    assert path(lib) == ("F32_SOFTMAX_FWD_VEC" if vec else "F32_SOFTMAX_FWD_ANY"), cid
    settle(cid + "-fwd", {"p": sw.t}, fb.softmax_fwd_ref(s, vec), [(sw, "s")])
    p = dense(torch.softmax(s.double(), -1).float()) if shift == 0 else Flat((rows, cols), init=torch.softmax(s.double(), -1).float(), shift=1).t
    dp = torch.randn(rows, cols, generator=g, device=DEV)
    dw = Flat((rows, cols), init=dp, shift=shift)
    call(lib, "dl_f32_softmax_bwd", _p(p), _p(dw.t), rows, cols, _s())
    assert path(lib) == ("F32_SOFTMAX_BWD_VEC" if vec else "F32_SOFTMAX_BWD_ANY"), cid
    settle(cid + "-bwd", {"ds": dw.t}, fb.softmax_bwd_ref(p, dp, vec), [(dw, "dp")])


def test_softmax_keymask(lib):
    B, rps, cols = 3, 5, 77
    g = gen_for("keymask")
    s = 3.0 * torch.randn(B * rps, cols, generator=g, device=DEV)
    bias = torch.zeros(B, cols, device=DEV)
    bias[0] = float("-inf")            # fully masked: exact zeros
    bias[1, 40:] = float("-inf")       # partly masked
    for kb in (bias, None):
        sw = Flat((B * rps, cols), init=s)
        call(lib, "dl_f32_softmax_keymask_fwd", _p(sw.t), _p(dense(kb) if kb is not None else None), B, rps, cols, _s())
        assert path(lib) == "F32_SOFTMAX_KEYMASK"
        ref = fb.softmax_fwd_ref(s, False, kb.repeat_interleave(rps, 0) if kb is not None else None)
        settle(f"keymask-{'bias' if kb is not None else 'nobias'}", {"p": sw.t}, ref, [(sw, "s")])
        if kb is not None:
            assert fb.same_bits(sw.t[:rps], torch.zeros(rps, cols, device=DEV)), "a fully masked row is not exact zeros"
            assert bool((sw.t[rps:2 * rps, 40:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ attention composites
def _autograd_attention(q, k, v, dout, B, Nq, L, H, dh, key_bias):
    Q, K_, V_ = (fb._heads(t.double(), B, n, H, dh).clone().requires_grad_(True) for t, n in ((q, Nq), (k, L), (v, L)))
    S = (Q @ K_.transpose(-1, -2)) * fb.f32c(float(dh) ** -0.5)
    if key_bias is not None:
        S = S + key_bias.double()[:, None, None, :]
    O = torch.softmax(S, -1) @ V_
    (O * fb._heads(dout.double(), B, Nq, H, dh)).sum().backward()
    back = lambda t, n: t.permute(0, 2, 1, 3).reshape(B * n, H * dh)  # noqa: E731
    return {"out": back(O.detach(), Nq), "dq": back(Q.grad, Nq), "dk": back(K_.grad, L), "dv": back(V_.grad, L)}


@pytest.mark.parametrize("n,cross", [(9, 0), (25, 0), (64, 0), (9, 1), (25, 1), (64, 1)])
def test_attention_composites(lib, n, cross):
    from diffulab_amd import ops

    B, H, dh = 2, 2, 16
    Nq, L = n, (77 if cross else n)
    cid = f"{'xattn' if cross else 'attn'}-n{n}"
    g = gen_for(cid)
    r = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    q, dout = opnd(r(B * Nq, H * dh)), opnd(r(B * Nq, H * dh))
    k, v = opnd(r(B * L, H * dh)), opnd(r(B * L, H * dh))
    kb = None
    if cross:
        kb = torch.zeros(B, L, device=DEV)
        kb[0, 50:] = float("-inf")
        kb[1, ::2] = float("-inf")
    o, dq = win(B * Nq, H * dh), win(B * Nq, H * dh)
    dk, dv = win(B * L, H * dh), win(B * L, H * dh)
    probs, dP = Flat((B, H, Nq, L)), Flat((B, H, Nq, L))
    if cross:
        ops.f32_xattn_fwd(q, k, v, dense(kb), o.win, probs.t, B, Nq, L, H, dh)
        ops.f32_xattn_bwd(q, k, v, dout, probs.t, dP.t, dq.win, dk.win, dv.win, B, Nq, L, H, dh)
    else:
        ops.f32_attn_fwd(q, k, v, o.win, probs.t, B, n, H, dh)
        ops.f32_attn_bwd(q, k, v, dout, probs.t, dP.t, dq.win, dk.win, dv.win, B, n, H, dh)
    CALLED.update({"dl_f32_gemm", "dl_f32_softmax_bwd", "dl_f32_softmax_keymask_fwd" if cross else "dl_f32_softmax_fwd"})
    ref = fb.attn_ref(q, k, v, dout, B, Nq, L, H, dh, kb)
    ag = _autograd_attention(q, k, v, dout, B, Nq, L, H, dh, kb)
    for name, t in ag.items():  # the composed reference is fp64 attention under autograd
        assert float((ref[name][0] - t).abs().max()) < 1e-11, (cid, name)
    dP.check(f"{cid}: dP")
    settle(cid, {"out": o.win, "probs": probs.t, "dq": dq.win, "dk": dk.win, "dv": dv.win}, ref,
           [(o, "out"), (dq, "dq"), (dk, "dk"), (dv, "dv"), (probs, "probs")])


# ------------------------------------------------------------------------------------------------------------------ token routing, gates, DDT
@pytest.mark.parametrize("D", [4, 260, 1024])
@pytest.mark.parametrize("k", [1, 5, 13])
def test_token_routing(lib, D, k):
    B, N = 2, 13
    cid = f"route-D{D}-k{k}"
    g = gen_for(cid)
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    idx = torch.stack([torch.randperm(N, generator=g, device=DEV)[:k] for _ in range(B)]).to(torch.int32).contiguous()
    # gather: a bytewise row copy (dl_gather_tokens over 2 D two-byte columns)
    src = opnd(n(B * N, D))
    gw = win(B * k, D)
    lib.call("dl_gather_tokens", _p(src), 2 * src.stride(0), _p(idx), None, _p(gw.win), 2 * gw.win.stride(0), B, N, k, 2 * D, _s())
    want = src.reshape(B, N, D).gather(1, idx.long()[:, :, None].expand(B, k, D)).reshape(B * k, D)
    settle(cid + "-gather", {"dst": gw.win}, {"dst": fb.bits(want)}, [(gw, "dst")])
    # scatter-add into non-zero rows
    s_src, d0 = opnd(n(B * k, D)), n(B * N, D)
    dw = win(B * N, D, init=d0)
    call(lib, "dl_f32_scatter_tokens_add", _p(s_src), s_src.stride(0), _p(idx), _p(dw.win), dw.win.stride(0), B, N, k, D, _s())
    settle(cid + "-scatter", {"dst": dw.win}, fb.scatter_add_ref(s_src, idx, d0, B, N, k), [(dw, "dst")])
    # restore
    inv = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    inv.scatter_(1, idx.long(), torch.arange(k, dtype=torch.int32, device=DEV)[None].expand(B, k))
    xd, mask = opnd(n(B * k, D)), dense(n(1, D))[0]
    rw = win(B * N, D)
    call(lib, "dl_f32_restore_tokens", _p(xd), xd.stride(0), _p(inv), _p(mask), _p(rw.win), rw.win.stride(0), B, N, k, D, _s())
    settle(cid + "-restore", {"out": rw.win}, fb.restore_ref(xd.contiguous(), inv, mask, B, N, k), [(rw, "out")])


@pytest.mark.parametrize("C", [4, 260, 1024])
@pytest.mark.parametrize("pick", ["none", "one", "all", "some"])
def test_masked_colsum(lib, C, pick):
    R, slabs = 45, 3  # 15 rows per slab: not a multiple of the four row lanes
    cid = f"colsum-C{C}-{pick}"
    g = gen_for(cid)
    x = opnd(torch.randn(R, C, generator=g, device=DEV) + 1.0, pad=3)
    sel = torch.zeros(R, dtype=torch.int32, device=DEV)
    if pick == "one":
        sel[17] = -1
    elif pick == "all":
        sel[:] = -1
    elif pick == "some":
        sel[torch.rand(R, generator=g, device=DEV) < 0.5] = -1
    pw = Flat((slabs, C))
    call(lib, "dl_f32_masked_colsum_partials", _p(x), x.stride(0), _p(sel), _p(pw.t), slabs, R, C, _s())
    settle(cid, {"part": pw.t}, fb.colsum_ref(x, sel, slabs), [(pw, "part")])


@pytest.mark.parametrize("D", [4, 260, 1024])
@pytest.mark.parametrize("rpm,G", [(1, 5), (13, 2)])
def test_gates_and_ddt(lib, D, rpm, G):
    M = rpm * G
    cid = f"gate-D{D}-r{rpm}x{G}"
    g = gen_for(cid)
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    x, t, dout = dense(n(M, D)), dense(n(M, D)), dense(n(M, D))
    gate = opnd(n(G, D))
    ow = win(M, D)
    call(lib, "dl_f32_gated_residual_fwd", _p(x), _p(t), _p(gate), gate.stride(0), rpm, _p(ow.win), ow.win.stride(0), M, D, _s())
    settle(cid + "-fwd", {"out": ow.win}, fb.gated_residual_ref(x, t, gate, rpm), [(ow, "out")])
    dt, dg = Flat((M, D)), win(G, D)
    call(lib, "dl_f32_gate_bwd", _p(dout), _p(t), _p(gate), gate.stride(0), rpm, _p(dt.t), _p(dg.win), dg.win.stride(0), M, D, _s())
    settle(cid + "-bwd", {"dt": dt.t, "dgate": dg.win}, fb.gate_bwd_ref(dout, t, gate, rpm), [(dt, "dt"), (dg, "dgate")])
    # DDT conditioning: B = G samples of N = rpm tokens; arguments out to +-30 and an exact 0
    enc, temb = opnd(2.0 * n(M, D)), win(G, D, init=2.0 * n(G, D))
    enc[0, 0], enc[0, 1], enc[0, 2] = 30.0, -30.0, 0.0
    temb.win[0, :3] = 0.0
    cw = Flat((M, D))
    call(lib, "dl_f32_ddt_cond_fwd", _p(enc), enc.stride(0), _p(temb.win), temb.win.stride(0), G, rpm, D, _p(cw.t), _s())
    settle(cid + "-ddt_fwd", {"out": cw.t}, fb.ddt_fwd_ref(enc, temb.win, rpm), [(cw, "out")])
    de, dtm = Flat((M, D)), win(G, D)
    assert dtm.win.stride(0) == temb.win.stride(0)  # dtemb shares ld_t
    call(lib, "dl_f32_ddt_cond_bwd", _p(dout), _p(enc), enc.stride(0), _p(temb.win), temb.win.stride(0), G, rpm, D, _p(de.t), _p(dtm.win), _s())
    settle(cid + "-ddt_bwd", {"denc": de.t, "dtemb": dtm.win}, fb.ddt_bwd_ref(dout, enc, temb.win, rpm), [(de, "denc"), (dtm, "dtemb")])


# ------------------------------------------------------------------------------------------------------------------ elementwise
def _edge(t):
    """arguments of +-30 and an exact 0 among the values of a 2-D tensor (or view)"""
    t[0, 0], t[1, 0], t[2, 0] = 30.0, -30.0, 0.0
    return t


@pytest.mark.parametrize("F", [4, 96, 100, 3])
def test_elementwise(lib, F):
    M = 7
    cid = f"ew-F{F}"
    g = gen_for(cid)
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    u = 2.0 * n(M, 2 * F)
    _edge(u[:, :F])
    _edge(u[:, F:])
    u[3, :min(3, F)] = torch.tensor([-30.0, 0.0, 30.0], device=DEV)[:min(3, F)]
    u, dh = dense(u), dense(n(M, F))
    h, du = Flat((M, F)), Flat((M, 2 * F))
    call(lib, "dl_f32_geglu_fwd", _p(u), _p(h.t), M, F, _s())
    settle(cid + "-geglu_fwd", {"h": h.t}, fb.geglu_fwd_ref(u, F), [(h, "h")])
    call(lib, "dl_f32_geglu_bwd", _p(dh), _p(u), _p(du.t), M, F, _s())
    settle(cid + "-geglu_bwd", {"du": du.t}, fb.geglu_bwd_ref(dh, u, F), [(du, "du")])
    if F % 4 == 0:  # SwiGLU takes F % 4 == 0 only
        h, du = Flat((M, F)), Flat((M, 2 * F))
        call(lib, "dl_f32_swiglu_fwd", _p(u), _p(h.t), M, F, _s())
        settle(cid + "-swiglu_fwd", {"h": h.t}, fb.swiglu_fwd_ref(u, F), [(h, "h")])
        call(lib, "dl_f32_swiglu_bwd", _p(dh), _p(u), _p(du.t), M, F, _s())
        settle(cid + "-swiglu_bwd", {"du": du.t}, fb.swiglu_bwd_ref(dh, u, F), [(du, "du")])
    else:
        with pytest.raises(RuntimeError):
            call(lib, "dl_f32_swiglu_fwd", _p(u), _p(h.t), M, F, _s())
        with pytest.raises(RuntimeError):
            call(lib, "dl_f32_swiglu_bwd", _p(dh), _p(u), _p(du.t), M, F, _s())
    a, b = dense(_edge(4.0 * n(M, F))), dense(n(M, F))
    o = Flat((M, F))
    call(lib, "dl_f32_add", _p(a), _p(b), _p(o.t), M * F, _s())
    settle(cid + "-add", {"out": o.t}, fb.add_ref(a, b), [(o, "out")])
    o = Flat((M, F))
    call(lib, "dl_f32_silu_bwd", _p(b), _p(a), _p(o.t), M * F, _s())
    settle(cid + "-silu_bwd", {"dx": o.t}, fb.silu_bwd_ref(b, a), [(o, "dx")])


@pytest.mark.parametrize("p", [1, 2, 4])
@pytest.mark.parametrize("order", [0, 1])
def test_patchify(lib, p, order):
    B, C, H, W = 2, 3, 8, 12
    F = C * p * p
    cid = f"patchify-p{p}-o{order}"
    x = dense(torch.randn(B, C, H, W, generator=gen_for(cid), device=DEV))
    tok = Flat((B * (H // p) * (W // p), F + 5))
    call(lib, "dl_f32_patchify", _p(x), _p(tok.t), B, C, H, W, p, F + 5, order, _s())  # ld = F + 5: five zeroed columns
    settle(cid, {"tok": tok.t}, fb.patchify_ref(x, p, F + 5, order == 0), [(tok, "tok")])


def test_patch_orders_match_header():
    text = open(os.path.join(ROOT, "include", "diffulab_hip.h")).read()
    assert re.search(r"DL_PATCH_CPP\s*=?\s*0", text) and re.search(r"DL_PATCH_PPC\s*=?\s*1", text)


@pytest.mark.parametrize("dim", [2, 64, 65])
def test_timestep_embedding(lib, dim):
    t = torch.tensor([0.0, 0.5, 999.0, 250.25, 1000.0], device=DEV)
    o = Flat((t.numel(), dim))
    call(lib, "dl_f32_timestep_embedding", _p(dense(t[None])[0]), _p(o.t), t.numel(), dim, 10000.0, _s())
    settle(f"temb-dim{dim}", {"emb": o.t}, fb.timestep_ref(t, dim, 10000.0), [(o, "emb")])


@pytest.mark.parametrize("E", [4, 100, 259])
def test_cond_combine(lib, E):
    B, n_cls = 7, 5  # class 4 = the null class of classifier-free guidance; labels repeat
    cid = f"cond-E{E}"
    g = gen_for(cid)
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    idx = torch.tensor([1, 4, 1, 0, 4, 1, 3], device=DEV)
    e, table = dense(_edge(3.0 * n(B, E))), dense(n(n_cls, E))
    emb, act = Flat((B, E)), Flat((B, E))
    call(lib, "dl_f32_cond_combine_fwd", _p(e), _p(table), _p(idx), _p(emb.t), _p(act.t), B, E, _s())
    settle(cid + "-fwd", {"emb": emb.t, "act": act.t}, fb.cond_fwd_ref(e, table, idx), [(emb, "emb"), (act, "act")])
    emb2, act2 = Flat((B, E)), Flat((B, E))
    call(lib, "dl_f32_cond_combine_fwd", _p(e), None, None, _p(emb2.t), _p(act2.t), B, E, _s())
    settle(cid + "-fwd-notable", {"emb": emb2.t, "act": act2.t}, fb.cond_fwd_ref(e, None, None), [(emb2, "emb"), (act2, "act")])
    dact, dt0 = dense(n(B, E)), n(n_cls, E)
    demb, dtab = Flat((B, E)), Flat((n_cls, E), init=dt0)
    call(lib, "dl_f32_cond_combine_bwd", _p(dact), _p(emb.t), _p(idx), _p(demb.t), _p(dtab.t), B, E, _s())
    settle(cid + "-bwd", {"demb": demb.t, "dtable": dtab.t}, fb.cond_bwd_ref(dact, emb.t, idx, dt0), [(demb, "demb"), (dtab, "dtable")])
    assert fb.same_bits(dtab.t[2], dt0[2]), "the row of an absent class changed"


# ------------------------------------------------------------------------------------------------------------------ UNet
IMG = [(1, 1, 1, 1), (2, 1, 5, 3), (2, 5, 1, 3), (2, 6, 10, 5), (3, 4, 4, 48)]


@pytest.mark.parametrize("B,H,W,C", IMG)
def test_unet_data_movement(lib, B, H, W, C):
    cid = f"img-{B}x{H}x{W}x{C}"
    g = gen_for(cid)
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    P = B * H * W
    x = opnd(n(P, C), pad=3)  # ldx > C
    cols = Flat((P, C * 9))
    call(lib, "dl_f32_im2col3x3", _p(x), x.stride(0), _p(cols.t), B, H, W, C, _s())
    settle(cid + "-im2col", {"cols": cols.t}, fb.im2col_ref(x.contiguous(), B, H, W, C), [(cols, "cols")])
    dcols = dense(n(P, C * 9))
    dx = win(P, C, pad=3)  # ld_dx > C
    call(lib, "dl_f32_col2im3x3", _p(dcols), _p(dx.win), dx.win.stride(0), B, H, W, C, _s())
    settle(cid + "-col2im", {"dx": dx.win}, fb.col2im_ref(dcols, B, H, W, C), [(dx, "dx")])
    # resample: Hs x Ws = H x W is the small resolution
    big, small = dense(n(4 * P, C)), dense(n(P, C))
    for mode, src, scale in ((0, big, 0.25), (0, big, 1.0), (1, small, 0.25), (1, small, 1.0), (2, big, 1.0), (3, small, 1.0)):
        o = Flat((P if mode in (0, 2) else 4 * P, C))
        call(lib, "dl_f32_resample2x2", _p(src), _p(o.t), B, H, W, C, scale, mode, _s())
        settle(f"{cid}-resample{mode}-s{scale}", {"out": o.t}, fb.resample_ref(src, B, H, W, C, scale, mode), [(o, "out")])
    # layout converts and the strided copy
    nchw = dense(n(B, C, H * W))
    rows = win(P, C, pad=3)
    call(lib, "dl_f32_nchw_to_nhwc", _p(nchw), _p(rows.win), B, C, H * W, rows.win.stride(0), _s())
    settle(cid + "-to_nhwc", {"o": rows.win}, {"o": fb.bits(nchw.permute(0, 2, 1).reshape(P, C))}, [(rows, "rows")])
    back = Flat((B, C, H * W))
    call(lib, "dl_f32_nhwc_to_nchw", _p(x), _p(back.t), B, C, H * W, x.stride(0), _s())
    settle(cid + "-to_nchw", {"o": back.t}, {"o": fb.bits(x.reshape(B, H * W, C).permute(0, 2, 1))}, [(back, "nchw")])
    cw = win(P, C, pad=5)
    call(lib, "dl_f32_copy2d", _p(x), x.stride(0), _p(cw.win), cw.win.stride(0), P, C, _s())
    settle(cid + "-copy2d", {"o": cw.win}, {"o": fb.bits(x.contiguous())}, [(cw, "dst")])
    # additive conditioning and its pixel sum
    xr, e = dense(n(P, C)), opnd(n(B, C), pad=3)
    o = Flat((P, C))
    call(lib, "dl_f32_rowbias_add", _p(xr), _p(e), e.stride(0), _p(o.t), B, H * W, C, _s())
    settle(cid + "-rowbias_add", {"out": o.t}, fb.rowbias_add_ref(xr, e, B, H * W, C), [(o, "out")])
    de = win(B, C, pad=3)
    call(lib, "dl_f32_rowbias_bwd", _p(xr), _p(de.win), de.win.stride(0), B, H * W, C, _s())
    settle(cid + "-rowbias_bwd", {"de": de.win}, fb.rowbias_bwd_ref(xr, B, H * W, C), [(de, "de")])


GN_SHAPES = [(1, 32, 32), (77, 96, 8), (16, 512, 2), (64, 36, 3), (5, 64, 32)]


def _gn_cases():
    cs = []
    for i, (HW, C, G) in enumerate(GN_SHAPES):
        for flags in range(8):  # bit 0 FiLM, bit 1 SiLU, bit 2 dres
            cls = ("scaled", "offset32", "const")[(i + flags) % 3]
            cs.append(dict(HW=HW, C=C, G=G, flags=flags, cls=cls, id=f"gn-HW{HW}-C{C}-G{G}-{cls}-f{flags}"))
    return cs


GN_CASES = _gn_cases()


@pytest.mark.parametrize("case", GN_CASES, ids=[c["id"] for c in GN_CASES])
def test_groupnorm(lib, case):
    import groupnorm_bounds as gb

    c = case
    B, HW, C, G = 2, c["HW"], c["C"], c["G"]
    film, silu, use_dres = bool(c["flags"] & 1), bool(c["flags"] & 2), bool(c["flags"] & 4)
    g = gen_for(c["id"])
    n = lambda *s: torch.randn(s, generator=g, device=DEV)  # noqa: E731
    x = dense(gb.make_x(c["cls"], B, HW, C, G, g, DEV).float().reshape(B * HW, C))  # (bf16 values: exact in f32)
    st = Flat((B, G, 2))
    call(lib, "dl_f32_gn_stats", _p(x), _p(st.t), B, HW, C, G, fb.GN_EPS, _s())
    settle(c["id"] + "-stats", {"stats": st.t}, fb.gn_stats_ref(x, B, HW, C, G, fb.GN_EPS), [(st, "stats")])
    w, b = dense(1.0 + 0.2 * n(1, C))[0], dense(0.2 * n(1, C))[0]
    fs = fh = None
    ldf = 0
    if film:
        fbuf = eb.operand(0.3 * n(B, 2 * C + 3), 2 * C + 3)
        fs, fh, ldf = fbuf[:, :C], fbuf[:, C + 3:], 2 * C + 3
    o = Flat((B * HW, C))
    call(lib, "dl_f32_gn_apply_fwd", _p(x), _p(st.t), _p(w), _p(b), _p(fs), _p(fh), ldf, int(silu), _p(o.t), B, HW, C, G, _s())
    settle(c["id"] + "-apply", {"out": o.t}, fb.gn_apply_ref(x, st.t, w, b, fs, fh, silu, B, HW, C, G), [(o, "out")])
    dout, dres = dense(n(B * HW, C)), (dense(n(B * HW, C)) if use_dres else None)
    dx, dw, db = Flat((B * HW, C)), Flat((B, C)), Flat((B, C))
    dfw = eb.Guarded(B, 2 * C + 3, F32, DEV, left=0, ld=2 * C + 3) if film else None
    dfs, dfh = (dfw.win[:, :C], dfw.win[:, C + 3:]) if film else (None, None)
    if film:
        dfw.win[:, C:C + 3] = 0.0  # (the three columns between the halves: never written, checked below)
    call(lib, "dl_f32_gn_bwd", _p(dout), _p(x), _p(st.t), _p(w), _p(b), _p(fs), _p(fh), ldf, int(silu), _p(dres), _p(dx.t), _p(dw.t), _p(db.t),
         _p(dfs), _p(dfh), B, HW, C, G, _s())
    ref = fb.gn_bwd_ref(dout, x, st.t, w, b, fs, fh, silu, dres, B, HW, C, G)
    got = {"dx": dx.t, "dw": dw.t, "db": db.t}
    guards = [(dx, "dx"), (dw, "dw"), (db, "db")]
    if film:
        got.update(dfs=dfs, dfh=dfh)
        guards.append((dfw, "dfilm"))
    settle(c["id"] + "-bwd", got, ref, guards)
    if film:
        assert bool((dfw.win[:, C:C + 3] == 0).all()), "columns between the FiLM gradient halves written"


def test_groupnorm_bwd_refuses_wide_groups(lib):
    B, HW, C, G = 1, 2, 257, 1
    z, st = torch.zeros(B * HW, C, device=DEV), torch.zeros(B, G, 2, device=DEV)
    w = torch.ones(C, device=DEV)
    with pytest.raises(RuntimeError):
        call(lib, "dl_f32_gn_bwd", _p(z), _p(z), _p(st), _p(w), _p(w), None, None, 0, 0, None, _p(z.clone()), _p(torch.zeros(B, C, device=DEV)),
             _p(torch.zeros(B, C, device=DEV)), None, None, B, HW, C, G, _s())


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_path_enum_mirror():
    """PATHS mirrors enum DlF32Path by name and order"""
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "f32_paths.h")).read()
    body = text[text.index("enum DlF32Path"):text.index("DL_F32_PATH_COUNT")]
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", body.split("{", 1)[1], flags=re.M)
    assert names == PATHS


def test_every_f32_path_code_is_reached():
    """runs after the tables (module order): every DlF32Path code was taken"""
    print("\nworst |diff| / bound: " + "; ".join(f"{o} {r:.3f} ({cid})" for o, (r, cid) in sorted(WORST.items())))
    missing = set(PATHS[1:]) - REACHED
    assert not missing, f"f32 path codes no case reached: {sorted(missing)}"


def test_every_f32_entry_point_is_exercised():
    """every dl_f32_* declaration of the header was called by this module, and the coverage list says where"""
    from diffulab_amd import _lib

    names = {k for k in _lib.parse_header() if k.startswith("dl_f32_")}
    assert names == set(fb.COVERAGE), sorted(names ^ set(fb.COVERAGE))
    assert not names - CALLED, f"entry points no test called: {sorted(names - CALLED)}"
    for name, tests in fb.COVERAGE.items():
        for t in tests:
            assert t in globals(), (name, t)
