"""Every bf16-regime token, embedding and layout kernel, element by element, with write guards.

Tables of cases drive the entry points of bf16_aux_bounds.ENTRY_POINTS through the C ABI (the descriptor tables through
diffulab_amd.ops, so their host-side arithmetic is under test too).  A case
  * asserts the kernel form it was built to reach where the entry point has more than one (dl_lab_last_aux_path, csrc/aux_paths.h),
  * compares every element of every output with the fp64 reference within its bound, or bit for bit where the kernel only moves data
    (tests/bf16_aux_bounds.py; test_bf16_aux_bounds_host.py shows what the bounds admit and reject),
  * writes into poisoned allocations with guards around the window and reads operands from allocations whose gaps hold NaN.
The last tests assert that every path code was reached, that PATHS mirrors the header and that every entry point was called.
"""

from __future__ import annotations

import ctypes
import os
import re

import pytest
import torch

import bf16_aux_bounds as ab
import elementwise_bounds as eb
import f32_bounds as fb
from test_f32_paths_gpu import Flat, _p, _s, gen_for

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, BF = torch.float32, torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mirror of enum DlAuxPath (diffulab_amd/csrc/aux_paths.h), by name: index = code
PATHS = ["DL_AUX_PATH_NONE", "AUX_IM2COL_VEC", "AUX_IM2COL_SCALAR", "AUX_CAST_CONV_TILED", "AUX_CAST_CONV_DIRECT", "AUX_FOLD_TILED",
         "AUX_FOLD_DIRECT", "AUX_RESAMPLE_VEC_PAIR", "AUX_RESAMPLE_VEC_SINGLE", "AUX_RESAMPLE_SCALAR", "AUX_COLSUM_BF16_VEC",
         "AUX_COLSUM_BF16_SCALAR", "AUX_COLSUM_F32", "AUX_COLSUM_BATCHED", "AUX_COLSUM_BATCHED_FALLBACK"]
REACHED: set[str] = set()
CALLED: set[str] = set()
WORST: dict[str, tuple[float, str]] = {}


# ------------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    L = _lib.lib()
    L.cdll.dl_lab_last_aux_path.restype = ctypes.c_int
    return L


def call(L, name, *args):
    CALLED.add(name)
    return L.call(name, *args)


def path(L):
    code = L.cdll.dl_lab_last_aux_path()
    name = PATHS[code] if 0 <= code < len(PATHS) else f"<{code}>"
    REACHED.add(name)
    return name


def win(rows, cols, dtype=BF, pad=8, init=None):
    """an output window with 8 guard columns on the left and `pad` on the right (rows stay 16-byte aligned), guard rows around"""
    return eb.Guarded(rows, cols, dtype, DEV, left=8, right=pad, init=init)


def opnd(t, pad=8):
    """a 2-D operand with leading dimension cols + pad inside a poisoned allocation that ends in NaN rows"""
    return eb.operand(t.contiguous(), t.shape[1] + pad)


def dense(t):
    t = t.contiguous()
    return eb.operand(t.reshape(-1, t.shape[-1]), t.shape[-1]).view(t.shape)


def rnd(g, *s, dtype=BF, scale=1.0):
    return (scale * torch.randn(s, generator=g, device=DEV)).to(dtype)


def settle(cid, got: dict, ref: dict, guards=()):
    """guards intact, then every output inside its bound (or bit-identical); keeps the worst ratio per output for the report"""
    torch.cuda.synchronize()
    for g, what in guards:
        g.check(f"{cid}: {what}")
    ratios = ab.judge(got, ref)
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


# ------------------------------------------------------------------------------------------------------------------ tokens.hip
def _routing(g, B, N, k):
    idx = torch.stack([torch.randperm(N, generator=g, device=DEV)[:k] for _ in range(B)]).to(torch.int32).contiguous()
    inv = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    inv.scatter_(1, idx.long(), torch.arange(k, dtype=torch.int32, device=DEV)[None].expand(B, k).contiguous())
    return idx, inv


@pytest.mark.parametrize("D", [8, 72, 384])
@pytest.mark.parametrize("N,k", [(1, 1), (5, 1), (5, 5), (64, 1), (64, 64)])
def test_token_routing(lib, D, N, k):
    B = 3
    cid = f"route-D{D}-N{N}-k{k}"
    g = gen_for(cid)
    idx, inv = _routing(g, B, N, k)
    src = opnd(rnd(g, B * N, D))
    for keep in (None, torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)):
        gw = win(B * k, D)
        call(lib, "dl_gather_tokens", _p(src), src.stride(0), _p(idx), _p(keep), _p(gw.win), gw.win.stride(0), B, N, k, D, _s())
        settle(f"{cid}-gather{'-keep' if keep is not None else ''}", {"dst": gw.win}, ab.gather_ref(src.contiguous(), idx, keep, B, N, k), [(gw, "dst")])
    s_src, d0 = opnd(rnd(g, B * k, D)), rnd(g, B * N, D)
    dw = win(B * N, D, init=d0)
    call(lib, "dl_scatter_tokens_add", _p(s_src), s_src.stride(0), _p(idx), _p(dw.win), dw.win.stride(0), B, N, k, D, _s())
    settle(cid + "-scatter", {"dst": dw.win}, ab.scatter_add_ref(s_src.contiguous(), idx, d0, B, N, k), [(dw, "dst")])
    xd, mask = opnd(rnd(g, B * k, D)), dense(torch.randn(1, D, generator=g, device=DEV))[0]
    rw = win(B * N, D)
    call(lib, "dl_restore_tokens", _p(xd), xd.stride(0), _p(inv), _p(mask), _p(rw.win), rw.win.stride(0), B, N, k, D, _s())
    settle(cid + "-restore", {"out": rw.win}, ab.restore_ref(xd.contiguous(), inv, mask, B, N, k), [(rw, "out")])


def test_row_grid_second_trip(lib):
    """4200 rows x 4096 columns: 2,150,400 chunks, past the 8192 x 256 threads of row_grid, for each of its six kernels"""
    B, N, k, D = 1, 4200, 4200, 4096
    g = gen_for("route-big")
    idx, _ = _routing(g, B, N, k)
    src = dense(rnd(g, B * N, D))
    gw = Flat((B * k, D), dtype=BF)
    call(lib, "dl_gather_tokens", _p(src), D, _p(idx), None, _p(gw.t), D, B, N, k, D, _s())
    settle("route-big-gather", {"dst": gw.t}, ab.gather_ref(src, idx, None, B, N, k), [(gw, "dst")])
    d0 = rnd(g, B * N, D)
    dw = Flat((B * N, D), init=d0, dtype=BF)
    call(lib, "dl_scatter_tokens_add", _p(src), D, _p(idx), _p(dw.t), D, B, N, k, D, _s())
    settle("route-big-scatter", {"dst": dw.t}, ab.scatter_add_ref(src, idx, d0, B, N, k), [(dw, "dst")])
    inv = torch.full((B, N), -1, dtype=torch.int32, device=DEV)
    inv[0, idx[0, :k // 2].long()] = torch.arange(k // 2, dtype=torch.int32, device=DEV)  # half of the rows get the mask token
    mask = dense(torch.randn(1, D, generator=g, device=DEV))[0]
    rw = Flat((B * N, D), dtype=BF)
    call(lib, "dl_restore_tokens", _p(src), D, _p(inv), _p(mask), _p(rw.t), D, B, N, k, D, _s())
    settle("route-big-restore", {"out": rw.t}, ab.restore_ref(src, inv, mask, B, N, k), [(rw, "out")])
    cw = Flat((N, D), dtype=BF)
    call(lib, "dl_copy_rows3d", _p(src), 2100 * D, D, _p(cw.t), 2100 * D, D, 2, 2100, D, _s())
    settle("route-big-copy3d", {"dst": cw.t}, {"dst": fb.bits(src)}, [(cw, "dst")])
    t, gate = dense(rnd(g, N, D)), dense(rnd(g, 2, D))
    ow = Flat((N, D), dtype=BF)
    call(lib, "dl_gated_residual_fwd", _p(src), _p(t), _p(gate), D, 2100, _p(ow.t), D, N, D, _s())
    settle("route-big-gate", {"out": ow.t}, ab.gated_residual_ref(src, t, gate, 2100), [(ow, "out")])
    temb = dense(torch.randn(2, D, generator=g, device=DEV))
    zw = Flat((N, D), dtype=BF)
    call(lib, "dl_ddt_cond_fwd", _p(src), D, _p(temb), D, 2, 2100, D, _p(zw.t), _s())
    settle("route-big-ddt_fwd", {"out": zw.t}, ab.ddt_fwd_ref(src, temb, 2100), [(zw, "out")])


@pytest.mark.parametrize("C", [8, 72, 384])
@pytest.mark.parametrize("pick", ["none", "all", "some"])
def test_masked_colsum(lib, C, pick):
    R = 769
    cid = f"mcolsum-C{C}-{pick}"
    g = gen_for(cid)
    x = opnd(rnd(g, R, C) + 1.0)
    sel = torch.zeros(R, dtype=torch.int32, device=DEV)
    if pick == "all":
        sel[:] = -1
    elif pick == "some":
        sel[torch.rand(R, generator=g, device=DEV) < 0.5] = -1
    o0 = torch.randn(C, generator=g, device=DEV)
    ow = Flat((C,), init=o0)
    call(lib, "dl_masked_colsum", _p(x), x.stride(0), _p(sel), _p(ow.t), R, C, _s())
    settle(cid, {"out": ow.t}, ab.masked_colsum_ref(x, sel, o0), [(ow, "out")])
    if pick == "none":
        assert ab.same_bits(ow.t, o0)


@pytest.mark.parametrize("D", [8, 72, 384])
@pytest.mark.parametrize("rpm,G", [(1, 5), (5, 3), (64, 2)])
def test_gated_residual_and_copy_rows(lib, D, rpm, G):
    M = rpm * G
    cid = f"gate-D{D}-r{rpm}x{G}"
    g = gen_for(cid)
    x, t, gate = dense(rnd(g, M, D)), dense(rnd(g, M, D)), opnd(rnd(g, G, D))
    ow = win(M, D)
    call(lib, "dl_gated_residual_fwd", _p(x), _p(t), _p(gate), gate.stride(0), rpm, _p(ow.win), ow.win.stride(0), M, D, _s())
    settle(cid + "-fwd", {"out": ow.win}, ab.gated_residual_ref(x, t, gate, rpm), [(ow, "out")])
    # copy_rows3d: G batches of rpm rows, batch and row strides above the dense ones on both sides
    src = opnd(rnd(g, G * (rpm + 1), D))  # batch stride (rpm + 1) rows: one row of every batch is not copied
    cw = win(G * (rpm + 2), D)
    cw.win.copy_(rnd(g, G * (rpm + 2), D))
    before = cw.win.clone()
    call(lib, "dl_copy_rows3d", _p(src), (rpm + 1) * src.stride(0), src.stride(0), _p(cw.win), (rpm + 2) * cw.win.stride(0), cw.win.stride(0), G,
         rpm, D, _s())
    want = before.reshape(G, rpm + 2, D).clone()
    want[:, :rpm] = src.reshape(G, rpm + 1, D)[:, :rpm]
    settle(cid + "-copy3d", {"dst": cw.win}, {"dst": fb.bits(want.reshape(-1, D))}, [(cw, "dst")])


@pytest.mark.parametrize("D", [8, 264])
@pytest.mark.parametrize("N", [1, 16, 17, 33])
@pytest.mark.parametrize("B", [1, 3])
def test_ddt_cond(lib, D, N, B):
    M = B * N
    cid = f"ddt-D{D}-N{N}-B{B}"
    g = gen_for(cid)
    enc = opnd(ab.spread((M, D), g, DEV, lim=10.0))
    temb = win(B, D, dtype=F32, init=ab.spread((B, D), g, DEV, lim=5.0, dtype=F32))
    cw = Flat((M, D), dtype=BF)
    call(lib, "dl_ddt_cond_fwd", _p(enc), enc.stride(0), _p(temb.win), temb.win.stride(0), B, N, D, _p(cw.t), _s())
    settle(cid + "-fwd", {"out": cw.t}, ab.ddt_fwd_ref(enc, temb.win, N), [(cw, "out")])
    dsz = dense(rnd(g, M, D))
    t0 = torch.randn(B, D, generator=g, device=DEV)
    de, dtm = Flat((M, D), dtype=BF), win(B, D, dtype=F32, init=t0)
    assert dtm.win.stride(0) == temb.win.stride(0) > D  # dtemb shares ld_t
    call(lib, "dl_ddt_cond_bwd", _p(dsz), _p(enc), enc.stride(0), _p(temb.win), temb.win.stride(0), B, N, D, _p(de.t), _p(dtm.win), _s())
    settle(cid + "-bwd", {"denc": de.t, "dtemb": dtm.win}, ab.ddt_bwd_ref(dsz, enc, temb.win, t0, N), [(de, "denc"), (dtm, "dtemb")])


# ------------------------------------------------------------------------------------------------------------------ embed.hip
@pytest.mark.parametrize("p,order", [(1, 0), (2, 0), (2, 1), (4, 1)])
def test_patchify_unpatchify(lib, p, order):
    B, C, H, W = 2, 3, 8, 12
    Fq = C * p * p
    cid = f"patchify-p{p}-o{order}"
    g = gen_for(cid)
    x = dense(torch.randn(B, C, H, W, generator=g, device=DEV))
    M = B * (H // p) * (W // p)
    tok = Flat((M, Fq + 5), dtype=BF)
    call(lib, "dl_patchify", _p(x), _p(tok.t), B, C, H, W, p, Fq + 5, order, _s())
    settle(cid, {"tok": tok.t}, ab.patchify_ref(x, p, Fq + 5, order == 0), [(tok, "tok")])
    tk = opnd(torch.randn(M, Fq, generator=g, device=DEV), pad=5)
    img = Flat((B, C, H, W))
    call(lib, "dl_unpatchify", _p(tk), _p(img.t), B, C, H, W, p, tk.stride(0), _s())
    settle(cid + "-un", {"img": img.t}, ab.unpatchify_ref(tk.contiguous(), B, C, H, W, p), [(img, "img")])


def test_patchify_second_trip(lib):
    """more than 4096 x 256 items"""
    B, C, H, W, p = 3, 4, 304, 304, 2
    x = dense(torch.randn(B, C, H, W, generator=gen_for("patchify-big"), device=DEV))
    tok = Flat((B * (H // p) * (W // p), C * p * p), dtype=BF)
    call(lib, "dl_patchify", _p(x), _p(tok.t), B, C, H, W, p, C * p * p, 1, _s())
    settle("patchify-big", {"tok": tok.t}, ab.patchify_ref(x, p, C * p * p, False), [(tok, "tok")])
    img = Flat((B, C, H, W))
    tk = dense(x.reshape(-1, 16))
    call(lib, "dl_unpatchify", _p(tk), _p(img.t), B, C, H, W, p, 16, _s())
    settle("unpatchify-big", {"img": img.t}, ab.unpatchify_ref(tk, B, C, H, W, p), [(img, "img")])


@pytest.mark.parametrize("dim", [2, 256])
def test_timestep_embedding(lib, dim):
    t = torch.tensor([0.0, 0.5, 1.0, 17.0, 999.0], device=DEV)
    o = Flat((t.numel(), dim), dtype=BF)
    call(lib, "dl_timestep_embedding", _p(dense(t[None])[0]), _p(o.t), t.numel(), dim, 10000.0, _s())
    settle(f"temb-dim{dim}", {"emb": o.t}, ab.timestep_ref(t, dim, 10000.0), [(o, "emb")])


@pytest.mark.parametrize("B,E", [(7, 8), (7, 100), (65, 4096)])
def test_cond_combine(lib, B, E):
    n_cls = 11
    cid = f"cond-B{B}-E{E}"
    g = gen_for(cid)
    idx = torch.tensor([3, 10, 3, 0, 3, 10, 7], device=DEV).repeat(-(-B // 7))[:B].contiguous()  # the first-owner rule
    e, table = dense(ab.spread((B, E), g, DEV, dtype=F32)), dense(torch.randn(n_cls, E, generator=g, device=DEV))
    pe = dense(torch.randn(B, E, generator=g, device=DEV))
    dact, dt0 = dense(torch.randn(B, E, generator=g, device=DEV)), torch.randn(n_cls, E, generator=g, device=DEV)
    for form in ("table", "plain", "dense"):
        emb, act = Flat((B, E)), Flat((B, E), dtype=BF)
        if form == "dense":
            if E % 4:
                continue
            call(lib, "dl_cond_combine_dense_fwd", _p(e), _p(pe), _p(emb.t), _p(act.t), B, E, _s())
            addend = pe
        else:
            use = form == "table"
            call(lib, "dl_cond_combine_fwd", _p(e), _p(table) if use else None, _p(idx) if use else None, _p(emb.t), _p(act.t), B, E, _s())
            addend = table[idx] if use else None
        settle(f"{cid}-{form}-fwd", {"emb": emb.t, "act": act.t}, ab.cond_fwd_ref(e, addend), [(emb, "emb"), (act, "act")])
        if form == "plain":
            assert ab.same_bits(emb.t, e)
        embv = dense(emb.t.clone())
        runs = []
        for variant in (("full",) if form == "dense" else ("full", "noidx", "notable", "no16")):
            demb, d16, dtab = Flat((B, E)), Flat((B, E), dtype=BF), Flat((n_cls, E), init=dt0)
            if form == "dense":
                call(lib, "dl_cond_combine_dense_bwd", _p(dact), _p(embv), _p(demb.t), _p(d16.t), B, E, _s())
            else:
                call(lib, "dl_cond_combine_bwd", _p(dact), _p(embv), None if variant == "noidx" else _p(idx), _p(demb.t),
                     None if variant == "no16" else _p(d16.t), None if variant == "notable" else _p(dtab.t), B, E, _s())
            table_on = form != "dense" and variant in ("full", "no16")
            ref = ab.cond_bwd_ref(dact, embv, idx, dt0 if table_on else None)
            got = {"demb": demb.t, "demb16": d16.t, "dtable": dtab.t}
            guards = [(demb, "demb")]
            if variant == "no16":
                del ref["demb16"]
                assert bool(eb.is_poison(d16.buf).all())
            else:
                guards.append((d16, "demb16"))
            settle(f"{cid}-{form}-bwd-{variant}", got, ref, guards)
            torch.cuda.synchronize()
            dtab.check(cid)
            if table_on:
                runs.append(dtab.t.clone())
                assert ab.same_bits(dtab.t[2], dt0[2]), "the row of an absent class changed"
            else:
                assert ab.same_bits(dtab.t, dt0), "dtable written without idx / without a table"
        assert all(ab.same_bits(runs[0], r) for r in runs[1:]), "dtable differs between two calls"  # (full and no16: the same sums)


@pytest.mark.parametrize("n", [5, 1000, 524288 + 5])
def test_act_bwd(lib, n):
    cid = f"actbwd-n{n}"
    g = gen_for(cid)
    dy = dense(torch.randn(1, n, generator=g, device=DEV))
    pre = dense(ab.spread((1, n), g, DEV))
    for name, ref in (("dl_silu_bwd", ab.silu_bwd_ref), ("dl_gelu_bwd", ab.gelu_bwd_ref)):
        o = Flat((1, n), dtype=BF)
        call(lib, name, _p(dy), _p(pre), _p(o.t), n, _s())
        settle(f"{cid}-{name[3:]}", {"dx": o.t}, ref(dy, pre), [(o, "dx")])


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("rot", [None, 32, 64])
@pytest.mark.parametrize("n_off", [0, 5])
def test_heads(lib, H, rot, n_off):
    B, n_src = 2, 7
    n_dst, ld, M = n_src + 9, H * 64 + 8, B * n_src
    cid = f"heads-H{H}-rot{rot}-off{n_off}"
    g = gen_for(cid)
    cs = sn = None
    if rot:
        cs, sn = fb.rope_tables(n_src, rot, g, DEV)
        cs, sn = dense(cs), dense(sn)
    src = eb.operand(rnd(g, M, H * 64), ld)
    dst = Flat((B, H, n_dst, 64), dtype=BF)
    call(lib, "dl_heads_split_rope", _p(src), ld, _p(dst.t), B, H, n_src, n_dst, n_off, _p(cs), _p(sn), rot or 0, _s())
    torch.cuda.synchronize()
    rows = dst.t[:, :, n_off:n_off + n_src]
    settle(cid + "-split", {"dst": rows}, ab.heads_split_ref(src.contiguous(), cs, sn, B, H, n_src, rot or 0))
    dst.check(cid, finite=False)
    outside = torch.ones(n_dst, dtype=torch.bool, device=DEV)
    outside[n_off:n_off + n_src] = False
    assert bool(eb.is_poison(dst.t[:, :, outside]).all()), "rows outside [n_off, n_off + n_src) written"
    # backward: dst_grad rows outside the window hold NaN
    dg = Flat((B, H, n_dst, 64), dtype=BF)
    dg.t[:, :, n_off:n_off + n_src] = rnd(g, B, H, n_src, 64)
    for accumulate in (0, 1):
        s0 = rnd(g, M, H * 64)
        sw = eb.Guarded(M, H * 64, BF, DEV, left=0, ld=ld, init=s0 if accumulate else None)
        call(lib, "dl_heads_merge_rope_bwd", _p(dg.t), _p(sw.win), ld, B, H, n_src, n_dst, n_off, _p(cs), _p(sn), rot or 0, accumulate, _s())
        ref = ab.heads_merge_ref(dg.t[:, :, n_off:n_off + n_src], s0 if accumulate else None, cs, sn, B, H, n_src, rot or 0)
        settle(f"{cid}-merge-acc{accumulate}", {"src": sw.win}, ref, [(sw, "src_grad")])


def test_heads_second_trip(lib):
    """B n_src H 8 = 1,048,576 + 24 chunks: past the 4096 blocks"""
    B, H, n_src = 1, 3, 43691
    g = gen_for("heads-big")
    src = dense(rnd(g, B * n_src, H * 64))
    dst = Flat((B, H, n_src, 64), dtype=BF)
    call(lib, "dl_heads_split_rope", _p(src), H * 64, _p(dst.t), B, H, n_src, n_src, 0, None, None, 0, _s())
    settle("heads-big", {"dst": dst.t}, ab.heads_split_ref(src, None, None, B, H, n_src, 0), [(dst, "dst")])


def _colsum_want(dtype, C, ld, ptr):
    if dtype == F32:
        return "AUX_COLSUM_F32"
    return "AUX_COLSUM_BF16_VEC" if C % 8 == 0 and ld % 8 == 0 and ptr % 16 == 0 else "AUX_COLSUM_BF16_SCALAR"


COLSUM_CASES = [(R, C, BF) for R in (1, 255, 257, 769) for C in (1, 8, 12, 24, 520)] + [(131072 + 300, 8, BF), (257, 12, F32), (769, 520, F32)]


@pytest.mark.parametrize("R,C,dtype", COLSUM_CASES, ids=[f"R{r}-C{c}-{'f32' if d == F32 else 'bf16'}" for r, c, d in COLSUM_CASES])
def test_colsum(lib, R, C, dtype):
    cid = f"colsum-R{R}-C{C}-{'f32' if dtype == F32 else 'bf16'}"
    g = gen_for(cid)
    x = opnd(rnd(g, R, C, dtype=dtype) + 0.5, pad=8 if C % 8 == 0 else 4)
    ld, code = x.stride(0), (1 if dtype == F32 else 0)
    want = _colsum_want(dtype, C, ld, x.data_ptr())
    o0 = torch.randn(C, generator=g, device=DEV)
    ow = Flat((C,), init=o0)
    call(lib, "dl_colsum", _p(x), code, ld, _p(ow.t), R, C, _s())
    assert path(lib) == want, cid
    settle(cid + "-atomic", {"out": ow.t}, ab.colsum_ref(x, o0, R + 1), [(ow, "out")])  # slabs meet in atomics: depth = the terms
    for floats in (C, 512 * C + 7):  # one slab; ample
        runs = []
        for _ in range(2):
            ow, scr = Flat((C,), init=o0), Flat((floats,))
            call(lib, "dl_colsum_det", _p(x), code, ld, _p(ow.t), R, C, _p(scr.t), floats, _s())
            assert path(lib) == want, cid
            torch.cuda.synchronize()
            scr.check(cid + ": scratch", finite=False)
            depth = ab.colsum_det_depth(R, C, floats, want == "AUX_COLSUM_BF16_VEC")
            settle(f"{cid}-det{floats}", {"out": ow.t}, ab.colsum_ref(x, o0, depth), [(ow, "out")])
            runs.append(ow.t.clone())
        assert ab.same_bits(runs[0], runs[1]), f"{cid}: dl_colsum_det differs between two calls"


def test_colsum_batched(lib):
    """25 descriptors: one more than DL_COLSUM_BATCH_MAX, so the list is flushed in the middle; one of width 12 takes the fallback"""
    from diffulab_amd import ops

    g = gen_for("colsum-batched")
    shapes = [(1 + 37 * i % 700, (8, 24, 520, 72)[i % 4]) for i in range(25)]
    shapes[7] = (300, 12)
    for fallback in (True, False):
        items, outs = [], []
        for i, (R, C) in enumerate(shapes):
            if not fallback and C == 12:
                C = 16
            x = opnd(rnd(g, R, C) + 0.5, pad=8 if C % 8 == 0 else 4)
            o0 = torch.randn(C, generator=g, device=DEV)
            ow = Flat((C,), init=o0)
            items.append((x, ow.t, R, C))
            outs.append((ow, x, o0, R))
        ops.colsum_batched(items)
        CALLED.add("dl_colsum_batched")
        assert path(lib) == ("AUX_COLSUM_BATCHED_FALLBACK" if fallback else "AUX_COLSUM_BATCHED")
        for i, (ow, x, o0, R) in enumerate(outs):
            settle(f"colsumb-{int(fallback)}-{i}", {"out": ow.t}, ab.colsum_ref(x, o0, R + 1), [(ow, "out")])


@pytest.mark.parametrize("G", [1, 63, 65, 130])
@pytest.mark.parametrize("n", [1, 64, 70])
@pytest.mark.parametrize("clear", [0, 1])
def test_reduce_rows(lib, G, n, clear):
    cid = f"rrows-G{G}-n{n}-c{clear}"
    g = gen_for(cid)
    p0, o0 = torch.randn(G, n, generator=g, device=DEV), torch.randn(n, generator=g, device=DEV)
    pw, ow = Flat((G, n), init=p0), Flat((n,), init=o0)
    call(lib, "dl_reduce_rows_f32", _p(pw.t), _p(ow.t), G, n, clear, _s())
    settle(cid, {"out": ow.t, "partial": pw.t}, {**ab.colsum_ref(p0, o0, G + 1), "partial": fb.bits(torch.zeros_like(p0) if clear else p0)},
           [(ow, "out"), (pw, "partial")])


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("G", [1, 15, 17, 256])
@pytest.mark.parametrize("n", [1, 16, 21])
def test_reduce_rows_batched(lib, K, G, n):
    cid = f"rrowsb-K{K}-G{G}-n{n}"
    g = gen_for(cid)
    ps, os_ = G * n + 5, n + 3  # strides above the dense ones: the gaps hold NaN / poison
    part = eb.poison_(torch.empty(K * ps + 64, device=DEV))
    p0 = torch.randn(K, G, n, generator=g, device=DEV)
    o0 = torch.randn(K, n, generator=g, device=DEV)
    for kk in range(K):
        part[kk * ps:kk * ps + G * n] = p0[kk].reshape(-1)
    runs = []
    for _ in range(2):
        ow = eb.Guarded(K, n, F32, DEV, left=0, ld=os_, init=o0)
        call(lib, "dl_reduce_rows_batched_f32", _p(part), ps, _p(ow.win), os_, K, G, n, _s())
        ref = {"out": tuple(torch.stack(t) for t in zip(*(ab.colsum_ref(p0[kk], o0[kk], ab.reduce_rows_batched_depth(G))["out"] for kk in range(K))))}
        settle(cid, {"out": ow.win}, ref, [(ow, "out")])
        runs.append(ow.win.clone())
    assert ab.same_bits(runs[0], runs[1]), f"{cid}: two calls differ"


def _cosine_inputs(g, M, E):
    p, d = rnd(g, M, E), torch.randn(M, E, generator=g, device=DEV)
    if M >= 5:
        p[1] = 0.0                      # a zero p row: cos = 0 / eps
        p[3] *= 2.0**-20                # |p|^2 |d|^2 < eps^2: the clamp is active
        d[3] *= 2.0**-20
    return p, d


# (M = 16385 crosses the 4096-block grid cap: once, at the narrowest row)
@pytest.mark.parametrize("E,M", [(E, M) for E in (8, 512, 520) for M in (1, 5)] + [(8, 16385)])
def test_cosine_rows(lib, E, M):
    cid = f"cosine-E{E}-M{M}"
    g = gen_for(cid)
    p, d = _cosine_inputs(g, M, E)
    p, d = opnd(p), opnd(d, pad=4)
    cosv, pn2, dn2 = Flat((M,)), Flat((M,)), Flat((M,))
    call(lib, "dl_cosine_rows_fwd", _p(p), p.stride(0), _p(d), d.stride(0), _p(cosv.t), _p(pn2.t), _p(dn2.t), M, E, ab.COS_EPS, _s())
    ref = ab.cosine_fwd_ref(p, d)
    settle(cid + "-fwd", {"cos": cosv.t, "pn2": pn2.t, "dn2": dn2.t}, ref, [(cosv, "cos"), (pn2, "pn2"), (dn2, "dn2")])
    gs = torch.tensor([0.37], device=DEV)
    for gdev in (None, gs):
        dp = win(M, E)
        call(lib, "dl_cosine_rows_bwd", _p(p), p.stride(0), _p(d), d.stride(0), _p(cosv.t), _p(pn2.t), _p(dn2.t), -1.0 / M, _p(gdev), _p(dp.win),
             dp.win.stride(0), M, E, ab.COS_EPS, _s())
        settle(f"{cid}-bwd-{'dev' if gdev is not None else 'host'}", {"dp": dp.win},
               ab.cosine_bwd_ref(p, d, cosv.t, pn2.t, dn2.t, -1.0 / M, gdev), [(dp, "dp")])


# ------------------------------------------------------------------------------------------------------------------ unet.hip
IM2COL_CASES = [(1, 1, 1, 8, 0), (2, 1, 5, 8, 0), (2, 5, 1, 16, 0), (3, 4, 6, 24, 0), (2, 3, 4, 1, 0), (2, 3, 4, 3, 0), (2, 3, 4, 12, 0),
                (2, 3, 4, 8, 4)]


@pytest.mark.parametrize("B,H,W,C,xpad", IM2COL_CASES)
def test_im2col(lib, B, H, W, C, xpad):
    cid = f"im2col-{B}x{H}x{W}x{C}-p{xpad}"
    g = gen_for(cid)
    P, rows = B * H * W, B * H * W + 37
    ld = (9 * C + 7) // 8 * 8 + 8
    x = opnd(rnd(g, P, C), pad=xpad if xpad else (8 if C % 8 == 0 else 3))
    cols = Flat((rows, ld), dtype=BF)
    call(lib, "dl_im2col3x3", _p(x), x.stride(0), _p(cols.t), B, H, W, C, rows, ld, _s())
    vec = C % 8 == 0 and x.stride(0) % 8 == 0
    assert path(lib) == ("AUX_IM2COL_VEC" if vec else "AUX_IM2COL_SCALAR"), cid
    settle(cid, {"cols": cols.t}, ab.im2col_ref(x.contiguous(), B, H, W, C, rows, ld), [(cols, "cols")])


CONV_CASES = [(32, 32, 0, "TILED"), (64, 96, 0, "TILED"), (32, 32, 8, "DIRECT"), (3, 8, 0, "DIRECT"), (200, 24, 0, "DIRECT")]


@pytest.mark.parametrize("Co,Ci,padf,form", CONV_CASES)
def test_conv_weight_cast_and_fold(lib, Co, Ci, padf, form):
    cid = f"conv-{Co}x{Ci}-p{padf}"
    g = gen_for(cid)
    w = dense(torch.randn(Co, Ci * 9, generator=g, device=DEV)).view(Co, Ci, 3, 3)
    ldf, ldd = 9 * Ci + padf, 9 * Co
    wf, wd = Flat((Co, ldf), dtype=BF), Flat((Ci, ldd), dtype=BF)
    call(lib, "dl_cast_conv3x3_weight", _p(w), Co, Ci, _p(wf.t), ldf, _p(wd.t), ldd, _s())
    assert path(lib) == "AUX_CAST_CONV_" + form, cid
    settle(cid + "-cast", {"wf": wf.t, "wd": wd.t}, ab.cast_conv_ref(w, ldf, ldd), [(wf, "wf"), (wd, "wd")])
    gsrc = opnd(torch.randn(9 * Ci, Co, generator=g, device=DEV), pad=16)
    d0 = torch.randn(Co, Ci * 9, generator=g, device=DEV)
    dw = Flat((Co, Ci * 9), init=d0)
    call(lib, "dl_conv3x3_wgrad_fold", _p(gsrc), gsrc.stride(0), _p(dw.t), Co, Ci, _s())
    assert path(lib) == ("AUX_FOLD_TILED" if Co % 32 == 0 and Ci % 32 == 0 else "AUX_FOLD_DIRECT"), cid
    ref = ab.fold_ref(gsrc.contiguous()[None], d0, Co, Ci)
    settle(cid + "-fold", {"dw": dw.t.view(Co, Ci, 9)}, ref, [(dw, "dw")])


def test_conv_tables(lib):
    """ops.ConvCastTable with three shapes; ops.ConvFoldTable with every n_img class in one table (the binary search over tile_begin)
    and each entry in a table of its own"""
    from diffulab_amd import ops

    g = gen_for("conv-tables")
    ents, outs = [], []
    for Co, Ci in ((32, 32), (64, 96), (96, 32)):
        w = dense(torch.randn(Co, Ci * 9, generator=g, device=DEV)).view(Co, Ci, 3, 3)
        wf, wd = Flat((Co, 9 * Ci), dtype=BF), Flat((Ci, 9 * Co), dtype=BF)
        ents.append((w, wf.t, wd.t))
        outs.append((w, wf, wd))
    ops.ConvCastTable(ents).run()
    CALLED.add("dl_cast_conv3x3_weights_batched")
    for i, (w, wf, wd) in enumerate(outs):
        settle(f"casttable-{i}", {"wf": wf.t, "wd": wd.t}, ab.cast_conv_ref(w, wf.t.shape[1], wd.t.shape[1]), [(wf, "wf"), (wd, "wd")])

    T = ops.ConvFoldTable.TAP_SPLIT_MIN_IMAGES
    assert T == 8
    kinds = [("staged", 0, (64, 32)), ("staged", 0, (32, 96)), ("img", 1, (32, 32)), ("img", 7, (64, 32)), ("img", 8, (32, 64)), ("img", 9, (32, 32)),
             ("img", 12, (64, 64)), ("img", 17, (32, 32))]

    def build():
        es = []
        for kind, n_img, (Co, Ci) in kinds:
            ldg = Co + 16
            n = max(n_img, 1)
            vals = torch.randn(n, 9 * Ci, Co, generator=g, device=DEV)
            buf = eb.poison_(torch.empty(n * 9 * Ci + 2, ldg, device=DEV))
            gv = buf[:n * 9 * Ci].view(n, 9 * Ci, ldg)[:, :, :Co]
            gv.copy_(vals)
            d0 = torch.randn(Co, Ci, 3, 3, generator=g, device=DEV)
            dw = Flat((Co, Ci, 3, 3), init=d0)
            es.append(dict(kind=kind, n_img=n_img, Co=Co, Ci=Ci, vals=vals, g=gv if kind == "img" else gv[0], buf=buf, d0=d0, dw=dw))
        return es

    def check(es, clear, tag):
        torch.cuda.synchronize()
        for i, e in enumerate(es):
            # the device picks the tap-split form from n_img >= TAP_SPLIT_MIN_IMAGES, the image-sum tile below it, the staged tile at 0
            form = "staged" if e["n_img"] == 0 else ("tapsplit" if e["n_img"] >= T else "imgsum")
            ref = ab.fold_ref(e["vals"], e["d0"].reshape(e["Co"], -1), e["Co"], e["Ci"])
            settle(f"foldtable-{tag}-{i}-{form}", {"dw": e["dw"].t.view(e["Co"], e["Ci"], 9)}, ref, [(e["dw"], "dw")])
            n = max(e["n_img"], 1)
            gv = e["buf"][:n * 9 * e["Ci"]].view(n, 9 * e["Ci"], -1)
            assert bool(eb.is_poison(gv[:, :, e["Co"]:]).all()) and bool(eb.is_poison(e["buf"][n * 9 * e["Ci"]:]).all()), "g's gaps written"
            if e["kind"] == "staged" and clear:
                assert ab.same_bits(gv[:, :, :e["Co"]].contiguous(), torch.zeros_like(e["vals"])), "a cleared stage is not all zero"
            else:
                assert ab.same_bits(gv[:, :, :e["Co"]].contiguous(), e["vals"]), "a stage / partial image was modified"

    for clear in (True, False):
        finals = []
        for rep in range(2):
            g.manual_seed(77 + int(clear))
            es = build()
            ops.ConvFoldTable([(e["g"], e["dw"].t) for e in es]).run(clear=clear)
            CALLED.add("dl_conv3x3_wgrad_fold_batched")
            check(es, clear, f"all-c{int(clear)}")
            finals.append([e["dw"].t.clone() for e in es])
        assert all(ab.same_bits(a, b) for a, b in zip(*finals)), "the batched fold differs between two calls"
    g.manual_seed(79)
    es = build()
    for e in es:
        ops.ConvFoldTable([(e["g"], e["dw"].t)]).run(clear=True)
    check(es, True, "own")


RES_CASES = [(1, 1, 1, 8), (2, 3, 5, 24), (2, 4, 4, 12)]


@pytest.mark.parametrize("B,Hs,Ws,C", RES_CASES)
def test_resamplers(lib, B, Hs, Ws, C):
    cid = f"res-{B}x{Hs}x{Ws}x{C}"
    g = gen_for(cid)
    P = B * Hs * Ws
    for expand in (0, 1):
        for scale in (1.0, 0.25):
            ref_fn = ab.expand2x2_ref if expand else ab.reduce2x2_ref
            n_in, n_out = (P, 4 * P) if expand else (4 * P, P)
            xs = [dense(rnd(g, n_in, C)), dense(rnd(g, n_in, C))]
            # direct entry points
            o = Flat((n_out, C), dtype=BF)
            call(lib, "dl_expand2x2" if expand else "dl_reduce2x2", _p(xs[0]), _p(o.t), B, Hs, Ws, C, scale, _s())
            settle(f"{cid}-e{expand}-s{scale}", {"out": o.t}, ref_fn(xs[0], B, Hs, Ws, C, scale), [(o, "out")])
            # the pair: both, second absent, base moved by one element (scalar form)
            for mode in ("pair", "single", "shift"):
                sh = 1 if mode == "shift" else 0
                xin = [Flat((n_in, C), init=x, shift=sh, dtype=BF).t for x in xs]
                os_ = [Flat((n_out, C), shift=sh, dtype=BF) for _ in xs]
                two = mode != "single"
                call(lib, "dl_resample2x2_pair", _p(xin[0]), _p(os_[0].t), _p(xin[1]) if two else None, _p(os_[1].t) if two else None, B, Hs, Ws, C,
                     scale, expand, _s())
                want = "AUX_RESAMPLE_SCALAR" if (sh or C % 8) else ("AUX_RESAMPLE_VEC_PAIR" if two else "AUX_RESAMPLE_VEC_SINGLE")
                assert path(lib) == want, (cid, mode)
                if sh or C % 8:
                    CALLED.add("dl_expand2x2" if expand else "dl_reduce2x2")
                for j in range(2 if two else 1):
                    settle(f"{cid}-pair-{mode}-e{expand}-s{scale}-{j}", {"out": os_[j].t}, ref_fn(xs[j], B, Hs, Ws, C, scale), [(os_[j], "out")])
                if not two:
                    torch.cuda.synchronize()
                    assert bool(eb.is_poison(os_[1].buf).all())
    if C % 8 == 0:
        big, small = dense(rnd(g, 4 * P, C)), dense(rnd(g, P, C))
        o = Flat((P, C), dtype=BF)
        call(lib, "dl_pick2x2", _p(big), _p(o.t), B, Hs, Ws, C, _s())
        settle(cid + "-pick", {"out": o.t}, ab.pick_ref(big, B, Hs, Ws, C), [(o, "out")])
        o = Flat((4 * P, C), dtype=BF)
        call(lib, "dl_stuff2x2", _p(small), _p(o.t), B, Hs, Ws, C, _s())
        settle(cid + "-stuff", {"out": o.t}, ab.stuff_ref(small, B, Hs, Ws, C), [(o, "out")])


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("HW", [1, 7, 300])
@pytest.mark.parametrize("B", [1, 3])
def test_rowbias(lib, C, HW, B):
    cid = f"rowbias-C{C}-HW{HW}-B{B}"
    g = gen_for(cid)
    x, e = dense(rnd(g, B * HW, C)), opnd(rnd(g, B, C))
    o = Flat((B * HW, C), dtype=BF)
    call(lib, "dl_rowbias_add", _p(x), _p(e), e.stride(0), _p(o.t), B, HW, C, _s())
    settle(cid + "-add", {"out": o.t}, ab.rowbias_add_ref(x, e, B, HW, C), [(o, "out")])
    de = win(B, C)
    call(lib, "dl_rowbias_bwd", _p(x), _p(de.win), de.win.stride(0), B, HW, C, _s())
    settle(cid + "-bwd", {"de": de.win}, ab.rowbias_bwd_ref(x, B, HW, C), [(de, "de")])


@pytest.mark.parametrize("M", [1, 33])
@pytest.mark.parametrize("F", [8, 264])
def test_glu(lib, M, F):
    cid = f"glu-M{M}-F{F}"
    g = gen_for(cid)
    u, dh = opnd(ab.spread((M, 2 * F), g, DEV)), opnd(rnd(g, M, F))
    h, du = win(M, F), win(M, 2 * F)
    call(lib, "dl_geglu_fwd", _p(u), u.stride(0), _p(h.win), h.win.stride(0), M, F, _s())
    settle(cid + "-geglu_fwd", {"h": h.win}, ab.geglu_fwd_ref(u, F), [(h, "h")])
    call(lib, "dl_geglu_bwd", _p(dh), dh.stride(0), _p(u), u.stride(0), _p(du.win), du.win.stride(0), M, F, _s())
    settle(cid + "-geglu_bwd", {"du": du.win}, ab.geglu_bwd_ref(dh, u, F), [(du, "du")])
    ud, dd = dense(u.contiguous()), dense(dh.contiguous())  # the SwiGLU entry points take dense operands
    h, du = Flat((M, F), dtype=BF), Flat((M, 2 * F), dtype=BF)
    call(lib, "dl_swiglu_fwd", _p(ud), _p(h.t), M, F, _s())
    settle(cid + "-swiglu_fwd", {"h": h.t}, ab.swiglu_fwd_ref(ud, F), [(h, "h")])
    call(lib, "dl_swiglu_bwd", _p(dd), _p(ud), _p(du.t), M, F, _s())
    settle(cid + "-swiglu_bwd", {"du": du.t}, ab.swiglu_bwd_ref(dd, ud, F), [(du, "du")])


@pytest.mark.parametrize("B,C,HW", [(1, 1, 1), (2, 3, 5), (2, 8, 35), (3, 72, 4)])
def test_layout_and_glue(lib, B, C, HW):
    cid = f"layout-{B}x{C}x{HW}"
    g = gen_for(cid)
    P = B * HW
    nchw = dense(torch.randn(B, C, HW, generator=g, device=DEV))
    rows = win(P, C)
    call(lib, "dl_nchw_to_nhwc", _p(nchw), _p(rows.win), B, C, HW, rows.win.stride(0), _s())
    settle(cid + "-to_nhwc", {"o": rows.win}, {"o": fb.bits(nchw.permute(0, 2, 1).reshape(P, C).to(BF))}, [(rows, "rows")])
    x = opnd(rnd(g, P, C), pad=3)
    back = Flat((B, C, HW))
    call(lib, "dl_nhwc_to_nchw", _p(x), _p(back.t), B, C, HW, x.stride(0), _s())
    settle(cid + "-to_nchw", {"o": back.t}, {"o": fb.bits(x.float().reshape(B, HW, C).permute(0, 2, 1).contiguous())}, [(back, "nchw")])
    cw = win(P, C, pad=5)
    call(lib, "dl_copy2d_bf16", _p(x), x.stride(0), _p(cw.win), cw.win.stride(0), P, C, _s())
    settle(cid + "-copy2d", {"o": cw.win}, {"o": fb.bits(x.contiguous())}, [(cw, "dst")])
    a, b = dense(rnd(g, P, C, scale=4.0)), dense(rnd(g, P, C))
    o = Flat((P, C), dtype=BF)
    call(lib, "dl_add_bf16", _p(a), _p(b), _p(o.t), P * C, _s())
    settle(cid + "-add", {"out": o.t}, ab.add_ref(a, b), [(o, "out")])


# ------------------------------------------------------------------------------------------------------------------ argument contracts
def _z(*s, dtype=BF):
    return torch.zeros(*s, dtype=dtype, device=DEV)


def _off(t, n=1):
    """a view whose base is n elements off the 16-byte grid"""
    return t.reshape(-1)[n:]


def _rejection_cases():
    """(entry point, what, arguments as a function of the poisoned output) -- each names a condition its DL_CHECK_ARG states"""
    E, M = 16, 2
    p, d, v = _z(M * E + 8), _z(M * E + 8, dtype=F32), _z(M, dtype=F32)
    cs = _z(64, dtype=F32)
    x = _z(4 * 64 + 8)
    big = _z(8, dtype=F32)
    return [
        ("dl_cosine_rows_bwd", "dp off the 16-byte grid", BF, M * E + 8,
         lambda o: (_p(p), E, _p(d), E, _p(v), _p(v), _p(v), 1.0, None, _p(_off(o)), E, M, E, 1e-8, _s())),
        ("dl_cosine_rows_bwd", "p off the 16-byte grid", BF, M * E + 8,
         lambda o: (_p(_off(p)), E, _p(d), E, _p(v), _p(v), _p(v), 1.0, None, _p(o), E, M, E, 1e-8, _s())),
        ("dl_cosine_rows_bwd", "lddp < E", BF, M * E + 8,
         lambda o: (_p(p), E, _p(d), E, _p(v), _p(v), _p(v), 1.0, None, _p(o), 8, M, E, 1e-8, _s())),
        ("dl_cosine_rows_fwd", "ldp < E", F32, M,
         lambda o: (_p(p), 8, _p(d), E, _p(o), _p(v), _p(v), M, E, 1e-8, _s())),
        ("dl_heads_split_rope", "src off the 16-byte grid", BF, 2 * 64,
         lambda o: (_p(_off(x)), 64, _p(o), 1, 1, 2, 2, 0, None, None, 0, _s())),
        ("dl_heads_split_rope", "cs off the 16-byte grid", BF, 2 * 64,
         lambda o: (_p(x), 64, _p(o), 1, 1, 2, 2, 0, _p(_off(cs)), _p(cs), 8, _s())),
        ("dl_heads_merge_rope_bwd", "src_grad off the 16-byte grid", BF, 2 * 64 + 8,
         lambda o: (_p(x), _p(_off(o)), 64, 1, 1, 2, 2, 0, None, None, 0, 0, _s())),
        ("dl_pick2x2", "out off the 16-byte grid", BF, 16, lambda o: (_p(x), _p(_off(o)), 1, 1, 1, 8, _s())),
        ("dl_stuff2x2", "dy off the 16-byte grid", BF, 32, lambda o: (_p(_off(x)), _p(o), 1, 1, 1, 8, _s())),
        ("dl_rowbias_add", "e off the 16-byte grid", BF, 8, lambda o: (_p(x), _p(_off(x)), 8, _p(o), 1, 1, 8, _s())),
        ("dl_rowbias_add", "lde < C", BF, 16, lambda o: (_p(x), _p(x), 8, _p(o), 1, 1, 16, _s())),
        ("dl_rowbias_bwd", "dy off the 16-byte grid", BF, 8, lambda o: (_p(_off(x)), _p(o), 8, 1, 1, 8, _s())),
        ("dl_geglu_fwd", "h off the 16-byte grid", BF, 16, lambda o: (_p(x), 16, _p(_off(o)), 8, 1, 8, _s())),
        ("dl_geglu_bwd", "du off the 16-byte grid", BF, 24, lambda o: (_p(x), 8, _p(x), 16, _p(_off(o)), 16, 1, 8, _s())),
        ("dl_ddt_cond_bwd", "B = 65536", BF, 8, lambda o: (_p(x), _p(x), 8, _p(big), 8, 65536, 1, 8, _p(o), _p(big), _s())),
        ("dl_reduce_rows_batched_f32", "K = 65536", F32, 8, lambda o: (_p(big), 1, _p(o), 1, 65536, 1, 1, _s())),
        ("dl_reduce_rows_f32", "65536 slices of 64 rows", F32, 8, lambda o: (_p(big), _p(o), 64 * 65536, 1, 0, _s())),
    ]


@pytest.mark.parametrize("i", range(17))
def test_rejections(lib, i):
    """a call that breaks a stated condition returns an error and launches nothing: the poisoned output is untouched"""
    name, what, dtype, n, args = _rejection_cases()[i]
    out = eb.poison_(torch.empty(n, dtype=dtype, device=DEV))
    with pytest.raises(RuntimeError):
        lib.call(name, *args(out))
    torch.cuda.synchronize()
    assert bool(eb.is_poison(out).all()), f"{name}: {what}: the output was written"


def test_rejection_table_size():
    assert len(_rejection_cases()) == 17 and {c[0] for c in _rejection_cases()} >= {
        "dl_cosine_rows_fwd", "dl_cosine_rows_bwd", "dl_heads_split_rope", "dl_heads_merge_rope_bwd", "dl_pick2x2", "dl_stuff2x2",
        "dl_rowbias_add", "dl_rowbias_bwd", "dl_geglu_fwd", "dl_geglu_bwd", "dl_ddt_cond_bwd", "dl_reduce_rows_batched_f32", "dl_reduce_rows_f32"}


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_path_enum_mirror():
    """PATHS mirrors enum DlAuxPath by name and order"""
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "aux_paths.h")).read()
    body = text[text.index("enum DlAuxPath"):text.index("DL_AUX_PATH_COUNT")]
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", body.split("{", 1)[1], flags=re.M)
    assert names == PATHS


def test_every_aux_path_code_is_reached():
    """runs after the tables (module order): every DlAuxPath code was taken"""
    print("\nworst |diff| / bound: " + "; ".join(f"{o} {r:.3f} ({cid})" for o, (r, cid) in sorted(WORST.items())))
    missing = set(PATHS[1:]) - REACHED
    assert not missing, f"aux path codes no case reached: {sorted(missing)}"


def test_every_entry_point_is_exercised():
    """every name of ENTRY_POINTS is declared in the header, was called by this module, and the coverage list says where"""
    from diffulab_amd import _lib

    declared = set(_lib.parse_header())
    assert not set(ab.ENTRY_POINTS) - declared, sorted(set(ab.ENTRY_POINTS) - declared)
    assert set(ab.ENTRY_POINTS) == set(ab.COVERAGE), sorted(set(ab.ENTRY_POINTS) ^ set(ab.COVERAGE))
    assert not set(ab.ENTRY_POINTS) - CALLED, f"entry points no test called: {sorted(set(ab.ENTRY_POINTS) - CALLED)}"
    for name, tests in ab.COVERAGE.items():
        for t in tests:
            assert t in globals(), (name, t)
