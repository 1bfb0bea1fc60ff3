"""Every attention kernel up to 2048 tokens, element by element, with write guards.

The DiT family (dl_attn_fwd / _sv / _ex, dl_attn_bwd / _sv / _tok / _ex, dl_attn_fwd_qkn) and the UNet's small and cross attention
(dl_attn_small_*, dl_attn_cross_*) pick among 14 kernels by shape, CU count and head width.  One table of cases drives them; every case
  * checks that the entry point launched the expected kernel (dl_lab_last_attn_path, csrc/attn_paths.h; where the choice depends on
    the CU count the expectation is computed from dl_device_info),
  * compares every output element -- out, lse, dq, dk, dv, the fused-norm forward's q_out / k_out / rrms, the UNet kernels' probs
    and ds -- with an fp64 reference within a bound derived from what the kernel computes (tests/attention_bounds.py; the host test
    test_attention_bounds_host.py shows what those bounds admit and reject),
  * runs on operands in poisoned allocations (NaN in the leading-dimension gaps, after the last head / token row, and in the thirds
    of a qkv row the entry point must not read) and writes into windows of poisoned allocations whose guard rows and columns must come
    back bit-identical,
  * asserts exact zeros in dk / dv (and probs) of masked keys, keeps the older whole-chain relative-L2 check against the fp64 autograd
    gradient at the older thresholds, and runs twice: every output bit-identical between the two runs.
The last test asserts that the table reached every attention path code except the three long-sequence ones, which
tests/test_attn_long_gpu.py owns.
"""

from __future__ import annotations

import ctypes
import os
import re
import zlib
from dataclasses import dataclass, field

import pytest
import torch

import attention_bounds as ab
import elementwise_bounds as eb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DH = 64

# mirror of enum DlAttnPath (diffulab_amd/csrc/attn_paths.h), by name: index = code
PATHS = ["DL_ATTN_PATH_NONE", "ATTN_FWD_RESIDENT", "ATTN_FWD_TILED", "ATTN_FWD_QKN_CHAIN", "ATTN_FWD_QKN_PIPE", "ATTN_BWD_RESIDENT",
         "ATTN_BWD_TILED", "ATTN_SMALL_FWD_MFMA", "ATTN_SMALL_FWD_VALU", "ATTN_SMALL_BWD_MFMA", "ATTN_SMALL_BWD_VALU",
         "ATTN_CROSS_FWD_MFMA", "ATTN_CROSS_FWD_VALU", "ATTN_CROSS_BWD_MFMA", "ATTN_CROSS_BWD_VALU", "ATTN_FWD_LONG_BIAS",
         "ATTN_FWD_LONG_NOBIAS", "ATTN_BWD_LONG"]
LONG = {"ATTN_FWD_LONG_BIAS", "ATTN_FWD_LONG_NOBIAS", "ATTN_BWD_LONG"}  # tests/test_attn_long_gpu.py
DISTS = ("normal", "unit_rms", "peaked")


@dataclass
class Case:
    kind: str  # resident | tiled | qkn | small | cross
    dims: tuple
    dist: str = "normal"
    var: str = ""  # resident: hm | sv | tok;  tiled: sq | ex;  qkn: train | infer;  small / cross: -
    bias: str = "none"  # tiled: none | rand30 | tail | chunk | last;  cross: none | rand30 | single
    extra: dict = field(default_factory=dict)

    @property
    def id(self):
        dims = "x".join(str(d) for d in self.dims)
        return "-".join(x for x in (self.kind, self.var, dims, self.dist, "" if self.bias == "none" else self.bias) if x)


def _cases():
    cs = []
    # ---- resident kernels (B or a CU-count token, H, N): B * H in {1, CUs, 3 CUs + 1}, H in {1, 6, 16}, every N on every layout
    for i, N in enumerate((64, 128, 192, 256)):
        for j, var in enumerate(("hm", "sv", "tok")):
            cs.append(Case("resident", (2, (1, 6, 16)[(i + j) % 3], N), DISTS[(i + j) % 3], var))
    for N, H in ((128, 1), (192, 16), (128, 16), (192, 1)):
        cs.append(Case("resident", (3, H, N), "peaked", "tok"))
        cs.append(Case("resident", (3, H, N), "unit_rms", "sv"))
    cs.append(Case("resident", (1, 1, 64), "peaked", "hm"))
    cs.append(Case("resident", (1, 1, 256), "peaked", "hm"))
    cs.append(Case("resident", ("cu", 1, 256), "normal", "hm"))
    cs.append(Case("resident", ("3cu+1", 1, 256), "unit_rms", "sv"))
    cs.append(Case("resident", ("3cu+1", 1, 64), "normal", "tok"))
    # ---- tiled kernels (B, H, Nq, Nk): the square entry points for N > 256, and _ex with every bias variant
    for N, dist in ((512, "normal"), (768, "peaked"), (1280, "unit_rms"), (2048, "normal")):
        cs.append(Case("tiled", (2 if N < 2048 else 1, 2, N, N), dist, "sq"))
    for N in (1536, 1792):
        cs.append(Case("tiled", (1, 2, N, N), "peaked", "sq"))
    shapes = ((512, 512), (256, 2048), (2048, 256), (1792, 768), (1280, 1280))
    for i, bias in enumerate(("none", "rand30", "tail", "chunk", "last")):
        for j, (Nq, Nk) in enumerate(shapes):
            if bias == "chunk" and Nk == 256:
                continue  # (a 256-key chunk masked entirely would leave the sample without a key)
            cs.append(Case("tiled", (2, 2, Nq, Nk), DISTS[(i + j) % 3], "ex", bias))
    cs.append(Case("tiled", (1, 3, 2048, 2048), "peaked", "ex", "rand30"))
    cs.append(Case("tiled", ("cu", 1, 512, 512), "normal", "ex", "tail"))
    # ---- fused-norm forward (B, H, N, rot): chain and pipelined (N = 256 from 3 CUs of items: 130 samples x 6 heads end a
    #      workgroup's run of items inside a sample), training and inference forms
    for N in (64, 192, 256):
        for k, rot in enumerate((0, 32, 64)):
            cs.append(Case("qkn", (3, 6, N, rot), DISTS[k], "train" if (N // 64 + k) % 2 else "infer"))
    cs.append(Case("qkn", (2, 1, 256, 64), "peaked", "train"))
    cs.append(Case("qkn", (130, 6, 256, 64), "unit_rms", "train"))
    cs.append(Case("qkn", (131, 6, 256, 32), "normal", "infer"))
    cs.append(Case("qkn", (98, 8, 256, 0), "normal", "train"))
    # ---- UNet small attention (B, H, n, dh)
    for n in (1, 2, 16, 33, 63, 64):
        for dh in (8, 64, 128, 512):
            cs.append(Case("small", (2, 1 if dh == 512 else 3, n, dh), DISTS[(n + dh // 8) % 3]))
    cs.append(Case("small", (2, 2, 33, 72), "normal"))  # dh % 64 != 0: VALU
    cs.append(Case("small", (2, 2, 64, 320), "peaked"))
    # ---- UNet cross attention (B, H, Nq, L, dh)
    for i, Nq in enumerate((16, 64, 65, 256)):
        for j, L in enumerate((1, 77, 511, 512)):
            bias = ("none", "rand30", "single")[(i + j) % 3] if L > 1 else "none"
            dh = (64, 256, 72, 128)[(i + j) % 4]
            cs.append(Case("cross", (2, 2, Nq, L, dh), DISTS[(i + 2 * j) % 3], bias=bias))
    cs.append(Case("cross", (2, 1, 64, 512, 512), "normal", bias="rand30"))
    cs.append(Case("cross", (2, 4, 64, 77, 8), "normal", bias="single"))
    cs.append(Case("cross", (2, 2, 65, 77, 64), "peaked", bias="rand30"))
    return cs


CASES = _cases()
REACHED: set[str] = set()
WORST: dict[str, dict[str, tuple[float, str]]] = {}


# ------------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    L = _lib.lib()
    L.cdll.dl_lab_last_attn_path.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def n_cu(lib):
    cu, lds, hbm = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    arch = ctypes.create_string_buffer(64)
    lib.call("dl_device_info", 0, ctypes.byref(cu), ctypes.byref(lds), ctypes.byref(hbm), arch, 64)
    return cu.value


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _path(L):
    code = L.cdll.dl_lab_last_attn_path()
    name = PATHS[code] if 0 <= code < len(PATHS) else f"<{code}>"
    REACHED.add(name)
    return name


def _resolve(b, n_cu):
    return {"cu": n_cu, "3cu+1": 3 * n_cu + 1}.get(b, b)


class Rand:
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV)
        self.g.manual_seed(seed)

    def n(self, *shape):
        return torch.randn(shape, generator=self.g, device=DEV)

    def u(self, *shape):
        return torch.rand(shape, generator=self.g, device=DEV)


def _qkvdo(r, G, Nq, Nk, dh, dist):
    """q [G, Nq, dh], k / v [G, Nk, dh], dO [G, Nq, dh] (bf16 values) of one input distribution"""
    q, k, v, do = r.n(G, Nq, dh), r.n(G, Nk, dh), r.n(G, Nk, dh), r.n(G, Nq, dh)
    if dist == "unit_rms":  # the QK-norm regime
        q, k = (t / t.square().mean(-1, keepdim=True).sqrt() for t in (q, k))
    if dist == "peaked":  # q x 4 and a planted dominant key in a late key block: the online-softmax rescale fires late
        q = q * 4 * (64 / dh) ** 0.5
        k[:, max(Nk - 40, 0)] = q[:, min(7, Nq - 1)] / 4
    return q.to(BF), k.to(BF), v.to(BF), do.to(BF)


def _key_bias(r, kind, B, Nk):
    """f32 [B, Nk] additive key bias (0 keep / -inf masked) inside a poisoned allocation; no sample fully masked"""
    if kind == "none":
        return None
    keep = torch.ones(B, Nk, dtype=torch.bool, device=DEV)
    if kind == "rand30":
        keep = r.u(B, Nk) > 0.3
        keep[:, Nk // 2] = True
    elif kind == "tail":
        keep[:, Nk - 37 - 64 * (Nk > 256):] = False  # a masked tail that is not a multiple of 64
        keep[1:, Nk - 5:] = False
        keep[1:, :Nk - 5] = True
    elif kind == "chunk":  # one 256-key chunk masked entirely: the first one (every key so far masked) or the second
        for b in range(B):
            c0 = 256 * (b % 2)
            keep[b, c0:c0 + 256] = False
    elif kind == "last":  # sample 0 keeps only key Nk - 1, the others 70 % of their keys
        keep = r.u(B, Nk) > 0.3
        keep[:, 0] = True
        keep[0] = False
        keep[0, Nk - 1] = True
    elif kind == "single":  # sample 0 keeps a single key in the middle
        keep = r.u(B, Nk) > 0.3
        keep[:, 0] = True
        keep[0] = False
        keep[0, Nk // 2] = True
    assert bool(keep.any(1).all())
    buf = eb.poison_(torch.empty(B * Nk + 16, device=DEV))
    bias = buf[8:8 + B * Nk].view(B, Nk)
    bias.copy_(torch.zeros(B, Nk, device=DEV).masked_fill(~keep, float("-inf")))
    return bias


def _rows(values2d, guard_rows=2):
    """dense [rows, cols] operand (the ABI fixes the stride) with poisoned rows after the last one"""
    return eb.operand(values2d.contiguous(), values2d.shape[1], guard_rows=guard_rows)


def _dense(rows, cols, dtype, top=2, bottom=2):
    """dense [rows, cols] output window (the ABI fixes the stride): poisoned guard rows before and after"""
    return eb.Guarded(rows, cols, dtype, DEV, left=0, right=0, ld=cols, top=top, bottom=bottom)


def _hm(t, B, H):
    """token-major [B * N, H * dh] -> head-major [B * H, N, dh]"""
    N = t.shape[0] // B
    return t.reshape(B, N, H, -1).permute(0, 2, 1, 3).reshape(B * H, N, -1)


def _tok(t, B, H):
    """head-major [B * H, N, dh] -> token-major [B * N, H * dh]"""
    N, dh = t.shape[1], t.shape[2]
    return t.reshape(B, H, N, dh).permute(0, 2, 1, 3).reshape(B * N, H * dh)


class Checker:
    """collects a case's outputs: footprint now, bounds now, bits for the second run"""

    def __init__(self, case, family):
        self.case, self.family, self.bits = case, family, []

    def guard(self, g, what):
        g.check(f"{self.case.id} {what}")
        self.bits.append(g.win.clone())

    def within(self, got, ref, bound, what, H=1, rows="query"):
        r = ab.check(got, ref, bound, f"{self.case.id} {what}", H=H, rows=rows)
        w = WORST.setdefault(self.family, {})
        if r > w.get(what, (-1.0, ""))[0]:
            w[what] = (r, self.case.id)


def _rel_chain(c, outs, refs, tols):
    for (name, got), ref, tol in zip(outs, refs, tols):
        rel = eb.rel_l2(got, ref)
        assert rel < tol, f"{c.id}: {name} relative L2 {rel:.3e} against the fp64 gradient (threshold {tol})"


# ------------------------------------------------------------------------------------------------------------------ runners
def run_resident(L, c, r, n_cu, ck):
    B, H, N = _resolve(c.dims[0], n_cu), c.dims[1], c.dims[2]
    G, D, scale = B * H, H * DH, DH**-0.5
    q, k, v, do = _qkvdo(r, G, N, N, DH, c.dist)
    qd, kd = _rows(q.reshape(G * N, DH)), _rows(k.reshape(G * N, DH))
    dod = _rows(_tok(do, B, H))
    out, lse = _dense(B * N, D, BF), _dense(G, N, torch.float32, top=1, bottom=1)
    if c.var == "hm":
        vd = _rows(v.reshape(G * N, DH))
        L.call("dl_attn_fwd", _p(qd), _p(kd), _p(vd), _p(out.win), _p(lse.win), B, H, N, DH, scale, _s())
    else:  # V inside qkv rows whose q / k thirds hold NaN; sv: the pitch is free (3 D + pad), tok: 3 D
        pitch = 3 * D + (16 if c.var == "sv" else 0)
        qkv = eb.poison_(torch.empty(B * N + 2, pitch, dtype=BF, device=DEV))
        qkv[:B * N, 2 * D:3 * D] = _tok(v, B, H)
        vd = qkv[:, 2 * D:]
        L.call("dl_attn_fwd_sv", _p(qd), _p(kd), _p(vd), N * pitch, DH, pitch, _p(out.win), _p(lse.win), B, H, N, DH, scale, _s())
    assert _path(L) == "ATTN_FWD_RESIDENT", (c.id, _path(L))
    torch.cuda.synchronize()
    ck.guard(out, "out"), ck.guard(lse, "lse")
    r_out, b_out, r_lse, b_lse = ab.attn_fwd(q, k, v, scale)
    o_hm = _hm(out.win, B, H)
    ck.within(o_hm, r_out, b_out, "out", H)
    ck.within(lse.win.reshape(G, N), r_lse, b_lse, "lse", H)
    # backward, on the forward's own out and lse
    thirds = None
    if c.var == "hm":
        dq, dk, dv = (_dense(G * N, DH, BF) for _ in range(3))
        L.call("dl_attn_bwd", _p(qd), _p(kd), _p(vd), _p(out.win), _p(dod), _p(lse.win), _p(dq.win), _p(dk.win), _p(dv.win), B, H, N, DH,
               scale, _s())
        g = [dq.win.reshape(G, N, DH), dk.win.reshape(G, N, DH), dv.win.reshape(G, N, DH)]
        guards = [(dq, "dq"), (dk, "dk"), (dv, "dv")]
    elif c.var == "sv":  # dV into the v third of dqkv rows (pitch 3 D + pad): guard columns over the q / k thirds and the pad
        dq, dk = (_dense(G * N, DH, BF) for _ in range(2))
        dv = eb.Guarded(B * N, D, BF, DEV, left=2 * D, right=16, ld=3 * D + 16)
        pd = dv.buf.stride(0)
        L.call("dl_attn_bwd_sv", _p(qd), _p(kd), _p(vd), N * pitch, DH, pitch, _p(out.win), _p(dod), _p(lse.win), _p(dq.win), _p(dk.win),
               _p(dv.win), N * pd, DH, pd, B, H, N, DH, scale, _s())
        g = [dq.win.reshape(G, N, DH), dk.win.reshape(G, N, DH), _hm(dv.win, B, H)]
        guards = [(dq, "dq"), (dk, "dk"), (dv, "dv")]
    else:  # token-major dqkv rows [B * N, 3 D], all three thirds written: guard rows before and after
        thirds = _dense(B * N, 3 * D, BF)
        L.call("dl_attn_bwd_tok", _p(qd), _p(kd), _p(qkv), _p(out.win), _p(dod), _p(lse.win), _p(thirds.win), B, H, N, DH, scale, _s())
        g = [_hm(thirds.win[:, i * D:(i + 1) * D], B, H) for i in range(3)]
        guards = [(thirds, "dqkv")]
    assert _path(L) == "ATTN_BWD_RESIDENT", (c.id, _path(L))
    torch.cuda.synchronize()
    for gd, what in guards:
        ck.guard(gd, what)
    refs = ab.attn_bwd(q, k, v, do, o_hm, lse.win.reshape(G, N), scale)
    for i, what in enumerate(("dq", "dk", "dv")):
        ck.within(g[i], refs[2 * i], refs[2 * i + 1], what, H, rows="query" if what == "dq" else "key")
    if G <= 64:
        _rel_chain(c, list(zip(("dq", "dk", "dv"), g)), ab.attn_grad_fp64(q, k, v, do, scale), (8e-3, 8e-3, 8e-3))
        assert eb.rel_l2(o_hm, r_out) < 5e-3


def run_tiled(L, c, r, n_cu, ck):
    B, H, Nq, Nk = _resolve(c.dims[0], n_cu), *c.dims[1:]
    G, D, scale = B * H, H * DH, DH**-0.5
    q, k, v, do = _qkvdo(r, G, Nq, Nk, DH, c.dist)
    bias = _key_bias(r, c.bias, B, Nk)
    bias_g = None if bias is None else bias.repeat_interleave(H, 0)
    qd, kd, vd = _rows(q.reshape(G * Nq, DH)), _rows(k.reshape(G * Nk, DH)), _rows(v.reshape(G * Nk, DH))
    dod = _rows(_tok(do, B, H))
    out, lse = _dense(B * Nq, D, BF), _dense(G, Nq, torch.float32, top=1, bottom=1)
    dq, dk, dv = _dense(G * Nq, DH, BF), _dense(G * Nk, DH, BF), _dense(G * Nk, DH, BF)
    if c.var == "sq":
        L.call("dl_attn_fwd", _p(qd), _p(kd), _p(vd), _p(out.win), _p(lse.win), B, H, Nq, DH, scale, _s())
    else:
        L.call("dl_attn_fwd_ex", _p(qd), _p(kd), _p(vd), _p(out.win), _p(lse.win), B, H, Nq, Nk, DH, scale, _p(bias), _s())
    assert _path(L) == "ATTN_FWD_TILED", (c.id, _path(L))
    if c.var == "sq":
        L.call("dl_attn_bwd", _p(qd), _p(kd), _p(vd), _p(out.win), _p(dod), _p(lse.win), _p(dq.win), _p(dk.win), _p(dv.win), B, H, Nq, DH,
               scale, _s())
    else:
        L.call("dl_attn_bwd_ex", _p(qd), _p(kd), _p(vd), _p(out.win), _p(dod), _p(lse.win), _p(dq.win), _p(dk.win), _p(dv.win), B, H, Nq, Nk,
               DH, scale, _p(bias), _s())
    assert _path(L) == "ATTN_BWD_TILED", (c.id, _path(L))
    torch.cuda.synchronize()
    for gd, what in ((out, "out"), (lse, "lse"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        ck.guard(gd, what)
    r_out, b_out, r_lse, b_lse = ab.attn_fwd(q, k, v, scale, bias_g)
    o_hm = _hm(out.win, B, H)
    ck.within(o_hm, r_out, b_out, "out", H)
    ck.within(lse.win.reshape(G, Nq), r_lse, b_lse, "lse", H)
    g = [dq.win.reshape(G, Nq, DH), dk.win.reshape(G, Nk, DH), dv.win.reshape(G, Nk, DH)]
    refs = ab.attn_bwd(q, k, v, do, o_hm, lse.win.reshape(G, Nq), scale, bias_g)
    for i, what in enumerate(("dq", "dk", "dv")):
        ck.within(g[i], refs[2 * i], refs[2 * i + 1], what, H, rows="query" if what == "dq" else "key")
    if bias is not None:  # masked keys: exact zeros
        masked = torch.isinf(bias_g)
        assert float(g[1][masked].float().abs().max()) == 0.0 and float(g[2][masked].float().abs().max()) == 0.0, f"{c.id}: masked dk / dv"
    if G <= 8:
        # (a sample with a single kept key has P = 1 there: its true dq and dk are exactly zero, and what the kernel returns for it is
        # the rounding of the forward's bf16 out seen through delta -- inside the element-wise bounds above, but without a scale for a
        # relative measure, so the whole-tensor criterion is taken over the samples that keep more than one key)
        sel = torch.ones(G, dtype=torch.bool, device=DEV) if bias is None else (~torch.isinf(bias_g)).sum(1) > 1
        true = [t[sel] for t in ab.attn_grad_fp64(q, k, v, do, scale, bias_g)]
        _rel_chain(c, [(n, t[sel]) for n, t in zip(("dq", "dk", "dv"), g)], true, (8e-3, 8e-3, 8e-3))
        assert eb.rel_l2(o_hm, r_out) < 5e-3


def run_qkn(L, c, r, n_cu, ck):
    B, H, N, rot = c.dims
    G, D, M, scale, eps = B * H, H * DH, B * N, DH**-0.5, 1e-6
    x = r.n(M, 3 * D)
    if c.dist == "peaked":
        x[:, :D] *= 4
    qkv = _rows(x.to(BF))  # the ABI fixes the pitch (3 D): poisoned rows after the last token
    ssq = torch.stack([qkv[:, :D].float().square().sum(1), qkv[:, D:2 * D].float().square().sum(1)], 1).contiguous()
    sq, sk = (1 + 0.1 * r.n(D)).contiguous(), (1 + 0.1 * r.n(D)).contiguous()
    cos = sin = None
    if rot:  # tables exactly [N, rot / 2] inside a poisoned allocation
        ang = r.u(N, rot // 2) * 6.0
        tb = eb.poison_(torch.empty(2, N * (rot // 2) + 16, device=DEV))
        cos, sin = tb[0, 8:8 + N * (rot // 2)].view(N, rot // 2), tb[1, 8:8 + N * (rot // 2)].view(N, rot // 2)
        cos.copy_(ang.cos()), sin.copy_(ang.sin())
    want = "ATTN_FWD_QKN_PIPE" if N == 256 and D <= 2048 and G >= 3 * n_cu else "ATTN_FWD_QKN_CHAIN"

    def launch(train):
        out, lse = _dense(M, D, BF), _dense(G, N, torch.float32, top=1, bottom=1)
        qo = ko = rr = None
        if train:
            qo, ko, rr = _dense(G * N, DH, BF), _dense(G * N, DH, BF), _dense(M, 2, torch.float32, top=4, bottom=4)
        L.call("dl_attn_fwd_qkn", _p(qkv), _p(ssq), _p(sq), _p(sk), _p(cos), _p(sin), eps, rot, _p(qo.win) if train else None,
               _p(ko.win) if train else None, _p(rr.win) if train else None, _p(out.win), _p(lse.win), B, H, N, DH, scale, _s())
        assert _path(L) == want, (c.id, _path(L), want)
        torch.cuda.synchronize()
        return out, lse, qo, ko, rr

    out, lse, qo, ko, rr = launch(True)
    for gd, what in ((out, "out"), (lse, "lse"), (qo, "q_out"), (ko, "k_out"), (rr, "rrms")):
        ck.guard(gd, what)
    for i, (gd, sc, what) in enumerate(((qo, sq, "q_out"), (ko, sk, "k_out"))):
        y, by, rref, br = ab.qk_norm_rope(qkv[:, i * D:(i + 1) * D], ssq[:, i], sc, cos, sin, N, H, rot, eps)
        ck.within(gd.win.reshape(G, N, DH), _hm(y, B, H), _hm(by, B, H), what, H)
        ck.within(rr.win[:, i].reshape(B, N), rref.reshape(B, N), br.reshape(B, N), "rrms")
    v = _hm(qkv[:, 2 * D:], B, H)
    r_out, b_out, r_lse, b_lse = ab.attn_fwd(qo.win.reshape(G, N, DH), ko.win.reshape(G, N, DH), v, scale)
    ck.within(_hm(out.win, B, H), r_out, b_out, "out", H)
    ck.within(lse.win.reshape(G, N), r_lse, b_lse, "lse", H)
    if c.var == "infer":  # q_out = k_out = rrms = NULL: out and lse bit for bit the training form's
        out2, lse2, *_ = launch(False)
        ck.guard(out2, "out (inference)"), ck.guard(lse2, "lse (inference)")
        assert torch.equal(out2.win, out.win) and torch.equal(lse2.win, lse.win), f"{c.id}: inference form differs from the training form"


def _unet_operands(r, c, B, H, Nq, L, dh):
    G, W = B * H, H * dh
    q, k, v, do = _qkvdo(r, G, Nq, L, dh, c.dist)
    ldq, ldkv, ldo = W + 16, W + 24, W + 8  # larger than H * dh: the gaps hold NaN
    qd = eb.operand(_tok(q, B, H), ldq, col0=8)
    kd, vd = eb.operand(_tok(k, B, H), ldkv, col0=8), eb.operand(_tok(v, B, H), ldkv, col0=16)
    dod = eb.operand(_tok(do, B, H), ldo)
    return q, k, v, do, qd, kd, vd, dod, ldq, ldkv, ldo


def run_small(L, c, r, n_cu, ck):
    B, H, n, dh = c.dims
    G, W = B * H, H * dh
    scale = ab.f32(dh**-0.5)
    mfma = dh % 64 == 0 and dh <= 512
    q, k, v, do, qd, kd, vd, dod, ldq, ldkv, ldo = _unet_operands(r, c, B, H, n, n, dh)
    out = eb.Guarded(B * n, W, BF, DEV, left=0, ld=ldo)
    probs = _dense(G * n, n, torch.float32, top=8, bottom=8)
    L.call("dl_attn_small_fwd", _p(qd), _p(kd), _p(vd), ldq, ldkv, _p(out.win), ldo, _p(probs.win), B, n, H, dh, scale, _s())
    assert _path(L) == ("ATTN_SMALL_FWD_MFMA" if mfma else "ATTN_SMALL_FWD_VALU"), (c.id, _path(L))
    dq = eb.Guarded(B * n, W, BF, DEV, left=8, ld=ldq)
    dk, dv = eb.Guarded(B * n, W, BF, DEV, left=8, ld=ldkv), eb.Guarded(B * n, W, BF, DEV, left=16, ld=ldkv)
    L.call("dl_attn_small_bwd", _p(qd), _p(kd), _p(vd), ldq, ldkv, _p(dod), ldo, _p(probs.win), _p(dq.win), _p(dk.win), _p(dv.win), B, n, H,
           dh, scale, _s())
    assert _path(L) == ("ATTN_SMALL_BWD_MFMA" if mfma else "ATTN_SMALL_BWD_VALU"), (c.id, _path(L))
    torch.cuda.synchronize()
    _unet_checks(c, ck, B, H, n, n, q, k, v, do, None, scale, mfma, out, probs, None, dq, dk, dv)


def run_cross(L, c, r, n_cu, ck):
    B, H, Nq, Lk, dh = c.dims
    G, W = B * H, H * dh
    scale = ab.f32(dh**-0.5)
    mfma = dh % 64 == 0 and dh <= 512 and Nq <= 64
    q, k, v, do, qd, kd, vd, dod, ldq, ldkv, ldo = _unet_operands(r, c, B, H, Nq, Lk, dh)
    bias = _key_bias(r, c.bias, B, Lk)
    out = eb.Guarded(B * Nq, W, BF, DEV, left=0, ld=ldo)
    probs, ds = _dense(G * Nq, Lk, torch.float32, top=8, bottom=8), _dense(G * Nq, Lk, torch.float32, top=8, bottom=8)
    L.call("dl_attn_cross_fwd", _p(qd), _p(kd), _p(vd), ldq, ldkv, _p(bias), _p(out.win), ldo, _p(probs.win), B, Nq, Lk, H, dh, scale, _s())
    assert _path(L) == ("ATTN_CROSS_FWD_MFMA" if mfma else "ATTN_CROSS_FWD_VALU"), (c.id, _path(L))
    dq = eb.Guarded(B * Nq, W, BF, DEV, left=8, ld=ldq)
    dk, dv = eb.Guarded(B * Lk, W, BF, DEV, left=8, ld=ldkv), eb.Guarded(B * Lk, W, BF, DEV, left=16, ld=ldkv)
    L.call("dl_attn_cross_bwd", _p(qd), _p(kd), _p(vd), ldq, ldkv, _p(bias), _p(dod), ldo, _p(probs.win), _p(ds.win), _p(dq.win), _p(dk.win),
           _p(dv.win), B, Nq, Lk, H, dh, scale, _s())
    assert _path(L) == ("ATTN_CROSS_BWD_MFMA" if mfma else "ATTN_CROSS_BWD_VALU"), (c.id, _path(L))
    torch.cuda.synchronize()
    _unet_checks(c, ck, B, H, Nq, Lk, q, k, v, do, bias, scale, mfma, out, probs, ds, dq, dk, dv)


def _unet_checks(c, ck, B, H, Nq, Lk, q, k, v, do, bias, scale, mfma, out, probs, ds, dq, dk, dv):
    G = B * H
    for gd, what in ((out, "out"), (probs, "probs"), (ds, "ds"), (dq, "dq"), (dk, "dk"), (dv, "dv")):
        if gd is not None:
            ck.guard(gd, what)
    bias_g = None if bias is None else bias.repeat_interleave(H, 0)
    rp, bp, ro, bo = ab.probs_fwd(q, k, v, scale, bias_g, bf16_p=mfma)
    pk = probs.win.reshape(G, Nq, Lk)
    ck.within(pk, rp, bp, "probs", H)
    ck.within(_hm(out.win, B, H), ro, bo, "out", H)
    rs, bs, rq, bq, rk, bk, rv, bv = ab.probs_bwd(q, k, v, do, pk, scale, bf16_p=mfma)
    if ds is not None:
        ck.within(ds.win.reshape(G, Nq, Lk), rs, bs, "ds", H)
    g = [_hm(dq.win, B, H), _hm(dk.win, B, H), _hm(dv.win, B, H)]
    for got, ref, bound, what in ((g[0], rq, bq, "dq"), (g[1], rk, bk, "dk"), (g[2], rv, bv, "dv")):
        ck.within(got, ref, bound, what, H, rows="query" if what == "dq" else "key")
    if bias is not None:  # masked keys: probability, dk and dv exactly zero
        masked = torch.isinf(bias_g)
        assert float(pk[masked[:, None, :].expand_as(pk)].abs().max()) == 0.0, f"{c.id}: masked probs"
        assert float(g[1][masked].float().abs().max()) == 0.0 and float(g[2][masked].float().abs().max()) == 0.0, f"{c.id}: masked dk / dv"
    if Lk > 1:
        _rel_chain(c, list(zip(("dq", "dk", "dv"), g)), ab.attn_grad_fp64(q, k, v, do, scale, bias_g), (1e-2, 1e-2, 1e-2))


RUN = {"resident": run_resident, "tiled": run_tiled, "qkn": run_qkn, "small": run_small, "cross": run_cross}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_attn_path(lib, n_cu, case):
    seed = zlib.crc32(case.id.encode())
    first, second = Checker(case, case.kind), Checker(case, case.kind)
    RUN[case.kind](lib, case, Rand(seed), n_cu, first)
    RUN[case.kind](lib, case, Rand(seed), n_cu, second)  # the same inputs again: every output bit for bit
    assert len(first.bits) == len(second.bits)
    for i, (a, b) in enumerate(zip(first.bits, second.bits)):
        assert torch.equal(eb._int_view(a), eb._int_view(b)), f"{case.id}: output {i} differs between two runs"


def _buffers(B, H, N, dh):
    bf = [torch.zeros(B * H * N * dh + 64, dtype=BF, device=DEV) for _ in range(9)]
    return bf, torch.zeros(B * H * N + 64, device=DEV)


def test_refusals(lib):
    """shapes outside the envelope are refused before any launch, with a message that names the limit"""
    (q, k, v, o, do, dq, dk, dv, _), lse = _buffers(1, 1, 512, 128)
    sc = 0.125
    with pytest.raises(RuntimeError, match=r"dl_attn_fwd: N=320 must be a multiple of 64 up to 256, or a multiple of 256 up to 32768"):
        lib.call("dl_attn_fwd", _p(q), _p(k), _p(v), _p(o), _p(lse), 1, 1, 320, 64, sc, _s())
    with pytest.raises(RuntimeError, match=r"dl_attn_bwd: N=320 must be a multiple of 64 up to 256, or a multiple of 256 up to 32768"):
        lib.call("dl_attn_bwd", _p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(dq), _p(dk), _p(dv), 1, 1, 320, 64, sc, _s())
    with pytest.raises(RuntimeError, match=r"dl_attn_fwd: head_dim 128 unsupported \(64 only\)"):
        lib.call("dl_attn_fwd", _p(q), _p(k), _p(v), _p(o), _p(lse), 1, 1, 256, 128, sc, _s())
    with pytest.raises(RuntimeError, match=r"dl_attn_bwd_ex: head_dim 128 unsupported \(64 only\)"):
        lib.call("dl_attn_bwd_ex", _p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(dq), _p(dk), _p(dv), 1, 1, 256, 256, 128, sc, None, _s())
    with pytest.raises(RuntimeError, match=r"dl_attn_fwd_ex: Nq=64 Nk=256 must be multiples of 256 up to 32768"):
        lib.call("dl_attn_fwd_ex", _p(q), _p(k), _p(v), _p(o), _p(lse), 1, 1, 64, 256, 64, sc, None, _s())
    with pytest.raises(RuntimeError, match=r"dl_attn_bwd_ex: Nq=64 Nk=256 must be multiples of 256 up to 32768"):
        lib.call("dl_attn_bwd_ex", _p(q), _p(k), _p(v), _p(o), _p(do), _p(lse), _p(dq), _p(dk), _p(dv), 1, 1, 64, 256, 64, sc, None, _s())


def test_path_enum_mirror():
    """PATHS mirrors enum DlAttnPath by name and order"""
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "attn_paths.h")).read()
    body = text[text.index("enum DlAttnPath"):text.index("DL_ATTN_PATH_COUNT")]
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", body.split("{", 1)[1], flags=re.M)
    assert names == PATHS


def test_every_attention_path_code_is_reached(n_cu):
    """runs after the table (module order): every path code except the long-sequence ones (tests/test_attn_long_gpu.py) was taken"""
    for fam, outs in sorted(WORST.items()):
        print(f"\nworst |diff| / bound, {fam}: " + "; ".join(f"{o} {r:.3f} ({cid})" for o, (r, cid) in sorted(outs.items())))
    missing = set(PATHS[1:]) - LONG - REACHED
    assert not missing, f"attention path codes no case reached: {sorted(missing)} (device with {n_cu} CUs)"
    assert not (REACHED & LONG), f"the table is meant to stay below 2048 tokens: {sorted(REACHED & LONG)}"
    print(f"\nreached all {len(PATHS) - 1 - len(LONG)} attention path codes below the long-sequence kernels: {sorted(REACHED)}")
