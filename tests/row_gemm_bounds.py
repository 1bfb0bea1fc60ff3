"""fp64 references, per-element bounds, operand generators and the launcher mirror of the row-complete GEMMs (csrc/gemm_ln.hip,
body in csrc/gemm_rows_body.h: dl_ln_modulate_gemm_fwd = RK_LNF, dl_ln_modulate_gemm_bwd = RK_LNB, dl_gemm_nt_qk_norm_rope = RK_QK);
imported by tests/test_row_gemm_bounds_host.py and tests/test_row_gemm_paths_gpu.py, not a conftest.  Builds on
tests/elementwise_bounds.py (GEMM reference, gate / store terms, poison) and tests/row_bounds.py (the row kernels' references).

Every function works on the device of the tensors it is given: the host test runs it on the CPU against an f32 emulation, the GPU
test on the device against the kernels.  The operands come from oracle.synth (numpy's PCG64, keyed by name), so both see the same
values.

What the kernel rounds, step by step (gemm_rows_body.h):
    acc   f32 MFMA accumulation over K                                 -> eb.gemm_ref's acc_err = ACC_C * K * 2^-24 * |a| . |w|
    P     = pack2bf(acc): the accumulators ROUNDED TO bf16 before the epilogue (rk_gemm_body, "P[j][i][q]") -> half a bf16 ulp
    RK_LNF  t_out = P bit for bit; x = bf16(resid + gate * t) (f32 multiply and add, one bf16 store); mean / rstd / xm from the
            ROUNDED x ("statistics of what is stored"), i.e. the row kernel of norm.hip on x_out
    RK_QK   qkv = P bit for bit; rrms, q, k from P, i.e. the row kernel on the stored qkv
    RK_LNB  d = P is never stored.  xh = (x - mu) * rs, k0 = (1 + scale) * w, dxh = d * k0, c1 = mean dxh, c2 = mean dxh xh,
            dx = bf16(dres + rs * (dxh - c1 - xh c2)); dt = bf16(bf16(dx) * gate), S3 += bf16(dx) * gate_t; S1 += d, S2 += d xh per lane
            over the wave's 32 rows, then the eight waves' slots in wave order; dscale = w S2 + b S1, dshift = S1, dgate = S3,
            dwb = (1 + scale) * (S2, S1).
The forward and QK modes are therefore judged in stages, each from the previous stage's output as the kernel stored it.  The
backward cannot be staged; everything it computes is linear in d, so the input error e = acc_err + half a bf16 ulp of the fp64
product is propagated through the absolute values of that map, on top of the local f32 terms of row_bounds.ln_bwd_parts.
"""

from __future__ import annotations

import torch

import elementwise_bounds as eb
import row_bounds as rwb
from oracle import synth

D, BM, BN, BK = 384, 256, 384, 64  # RK_BN (= the model width), RK_BM (= rows per modulation group), RK_BN, RK_BK
U, C = eb.U32, eb.ACC_C
BF = torch.bfloat16

# ---------------------------------------------------------------------------------------------------------------- case tables
# (B, K, form, cap) -- M = 256 B.  B = 8: one tile per workgroup; B = 9: grid 8, workgroup 0 walks two tiles; B = 20 under a cap of 8:
# walks of 3 and 2 tiles.  K = 64: one k-step (the patch embedding's); 192: an odd number of k-steps, the epilogue's ring slot
# alternates from tile to tile of a walk; 384, 1152, 1536: the block's.
FWD_FORMS = {  # resid, gate, affine, t_out, eps
    "block": dict(resid=True, gate=True, affine=True, t_out=True, eps=1e-5),
    "nogate": dict(resid=True, gate=False, affine=True, t_out=True, eps=1e-5),
    "patch": dict(resid=False, gate=False, affine=True, t_out=False, eps=1e-5),  # x_out = the product itself
    "noaffine": dict(resid=True, gate=True, affine=False, t_out=True, eps=1e-6),
    "block_not": dict(resid=True, gate=True, affine=True, t_out=False, eps=1e-5),  # t not kept: the GEMM bound goes through the gate
}
FWD_CASES = [(8, 64, "patch", 0), (8, 384, "block", 0), (9, 192, "block", 0), (20, 1536, "block", 8), (9, 1152, "nogate", 0),
             (8, 192, "noaffine", 0), (9, 64, "block_not", 0)]
FWD_EXACT = (9, 192, "block", 0)
BWD_FORMS = {  # dres, gated (gate_t, gate, dt, dgate), affine, dwb
    "full": dict(dres=True, gated=True, affine=True, dwb=True),
    "bare": dict(dres=False, gated=False, affine=False, dwb=False),
    "head": dict(dres=False, gated=True, affine=False, dwb=False),
    "mixed": dict(dres=True, gated=False, affine=True, dwb=True),
}
BWD_CASES = [(8, 64, "bare", 0), (8, 1152, "full", 0), (9, 192, "full", 0), (20, 1536, "full", 8), (9, 384, "head", 0), (8, 192, "mixed", 0)]
BWD_EXACT = (9, 192, "full", 0)
# (B, N, H, dh, rot, n_off, n_dst, cap): K = D = 384 always.  N = 64: four samples per tile; N = 320, B = 8: tiles straddle samples
QK_CASES = [(8, 256, 6, 64, 64, 0, 256, 0), (9, 256, 6, 64, 32, 77, 356, 0), (20, 256, 6, 64, 64, 77, 356, 8), (32, 64, 6, 64, 64, 0, 64, 0),
            (8, 320, 6, 64, 32, 77, 420, 0), (8, 256, 12, 32, 32, 0, 256, 0), (8, 256, 6, 64, 0, 77, 356, 0)]
QK_EXACT = (9, 256, 6, 64, 64, 77, 356, 0)


# ---------------------------------------------------------------------------------------------------------------- operands
def _bf(key, shape, std=1.0):
    return synth.normal(key, shape, std=std).to(BF)


def exact_operands(key: str, M: int, Nw: int, K: int) -> tuple[torch.Tensor, torch.Tensor]:
    """A [M, K] in {-1, 0, 1}, W [Nw, K] in {-1, 0, 1} * 2^-3 with at most 255 non-zeros per row: every dot product is an integer of
    magnitude <= 255 times 2^-3 -- exact in bf16, and exact in f32 in every summation order.  The GEMM term of the bounds is zero."""
    a = (synth.integers(key + ".xa", (M, K), 3) - 1).to(BF)
    w = (synth.integers(key + ".xw", (Nw, K), 3) - 1).double()
    if K > 255:  # keep the 255 positions of each row with the smallest keys
        keys = synth.uniform(key + ".xk", (Nw, K))
        w = w * (keys <= keys.kthvalue(255, dim=1, keepdim=True).values)
    w = (w / 8).to(BF)
    assert_exact(a.double() @ w.double().t())
    return a, w


def assert_exact(ref: torch.Tensor) -> None:
    assert torch.equal(ref.to(BF).double(), ref), "the exact-product operands give a product that is not a bf16 value"


def _gemm_operands(key, M, Nw, K, exact, k_pad=0):
    if exact:
        return exact_operands(key, M, Nw, K)
    # k_pad: A has more columns than the K of the call (the patch embedding's zero-padded operand); the extra ones are not zero here
    return _bf(key + ".a", (M, K + k_pad)), _bf(key + ".w", (Nw, K), K**-0.5)


def fwd_case(B, K, form, exact=False) -> dict:
    f, M = FWD_FORMS[form], B * BM
    key = f"rgf.{B}.{K}.{form}"
    A, W = _gemm_operands(key, M, D, K, exact, k_pad=64 if form == "patch" else 0)
    return dict(mode="fwd", form=form, exact=exact, B=B, M=M, K=K, A=A, W=W, eps=f["eps"], t_out=f["t_out"],
                resid=_bf(key + ".r", (M, D)) + 0.25 if f["resid"] else None,
                gate=_bf(key + ".g", (B, D), 0.5) if f["gate"] else None,
                ln_w=1 + synth.normal(key + ".lw", (D,), std=0.1) if f["affine"] else None,
                ln_b=synth.normal(key + ".lb", (D,), std=0.1) if f["affine"] else None,
                scale=_bf(key + ".sc", (B, D), 0.3), shift=_bf(key + ".sh", (B, D), 0.3))


def bwd_case(B, K, form, exact=False) -> dict:
    f, M = BWD_FORMS[form], B * BM
    key = f"rgb.{B}.{K}.{form}"
    A, W = _gemm_operands(key, M, D, K, exact)
    x = _bf(key + ".x", (M, D), 2.0) + 0.25
    xf = x.float()
    return dict(mode="bwd", form=form, exact=exact, B=B, M=M, K=K, A=A, W=W, x=x, dwb=f["dwb"],
                mean=xf.mean(1).contiguous(), rstd=(xf.var(1, unbiased=False) + 1e-5).rsqrt().contiguous(),
                ln_w=1 + synth.normal(key + ".lw", (D,), std=0.1) if f["affine"] else None,
                ln_b=synth.normal(key + ".lb", (D,), std=0.2) if f["affine"] else None,
                scale=_bf(key + ".sc", (B, D), 0.3),
                dres=_bf(key + ".dr", (M, D)) if f["dres"] else None,
                gate_t=_bf(key + ".gt", (M, D)) if f["gated"] else None,
                gate=_bf(key + ".g", (B, D), 0.5) if f["gated"] else None)


def qk_case(B, N, H, dh, rot, n_off, n_dst, exact=False) -> dict:
    M = B * N
    key = f"rgq.{B}.{N}.{H}.{rot}.{n_off}"
    A, W = _gemm_operands(key, M, 3 * D, D, exact)
    ang = synth.uniform(key + ".ang", (N, max(rot // 2, 4)), hi=6.3).double()  # (rot = 0: tables the kernel must not read)
    return dict(mode="qk", form=f"N{N} H{H} rot{rot} off{n_off}", exact=exact, B=B, N=N, H=H, dh=dh, rot=rot, n_off=n_off, n_dst=n_dst,
                M=M, K=D, A=A, W=W, eps=1e-6, sq=1 + synth.normal(key + ".sq", (D,), std=0.1), sk=1 + synth.normal(key + ".sk", (D,), std=0.1),
                cos=ang.cos().float().contiguous(), sin=ang.sin().float().contiguous())


def to(case: dict, device) -> dict:
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in case.items()}


# ---------------------------------------------------------------------------------------------------------------- launcher mirror
def grid_of(ntiles: int, n_cu: int = 256, cap: int = 0) -> int:
    """rk_launch: min(budget, ntiles) & ~7 with dl_wg_budget's budget = max(8, cap or n_cu)"""
    budget = max(8, cap if 0 < cap < n_cu else n_cu)
    return min(budget, ntiles) & ~7


def slot_of(b: int, G: int) -> int:
    return (b & 7) * (G >> 3) + (b >> 3)


def walks(ntiles: int, n_cu: int = 256, cap: int = 0) -> list[list[int]]:
    """per workgroup, the tiles slot, slot + G, ... it walks (gemm_nt_rows_k: cnt = (ntiles - slot + G - 1) / G)"""
    G = grid_of(ntiles, n_cu, cap)
    return [list(range(slot_of(b, G), ntiles, G)) for b in range(G)]


def assert_owned_once(ntiles: int, n_cu: int = 256, cap: int = 0) -> None:
    seen = sorted(t for w in walks(ntiles, n_cu, cap) for t in w)
    assert seen == list(range(ntiles)), f"tiles {sorted(set(range(ntiles)) ^ set(seen))} without an owner or with two (ntiles {ntiles}, cap {cap})"


def row_of(s: int, wave: int) -> int:
    """rk_row_epilogue's row_of: the tile row wave `wave` processes as its s-th (s = (i * 2 + pair) * 8 + rr)"""
    i, pair, lr = s >> 4, (s >> 3) & 1, (s & 7) * 8 + wave
    return (2 * pair + (lr >> 5)) * 64 + i * 32 + (lr & 31)


ROW_OWNER = {row_of(s, w): (w, s) for w in range(8) for s in range(32)}  # tile row -> (wave, step)


def locator(M: int, tiles_n: int, K: int, n_cu: int = 256, cap: int = 0):
    """(row, column of a [M, 384 tiles_n] output) -> who computed it, for a failure message"""
    ntiles = (M // BM) * tiles_n
    G = grid_of(ntiles, n_cu, cap)

    def where(r, c):
        tile = (r // BM) * tiles_n + c // BN
        slot, t = tile % G, tile // G
        b = (slot % (G >> 3)) * 8 + slot // (G >> 3)
        lr, lc = r % BM, c % BN
        wave, s = ROW_OWNER[lr]
        return (f"workgroup {b} of {G}, tile {tile} = ({r // BM}, {c // BN}), number {t} of its walk (epilogue in ring slot "
                f"{((t + 1) * (K // BK) - 1) & 1}); accumulated by wave {(lr // 64) * 2 + lc // 192} fragment (j {lc % 192 // 32}, i {lr % 64 // 32}), "
                f"epilogue wave {wave} step {s} (dump i {s >> 4} pair {(s >> 3) & 1}, row {s & 7} of it), lane {lc // 8}")

    return where


# ---------------------------------------------------------------------------------------------------------------- judging
def judge(out, ref, bound, what, where=None) -> float:
    """every element of `out` within `bound` of `ref` (NaN fails) -> the worst |out - ref| / bound"""
    assert out.shape == ref.shape == bound.shape, (what, out.shape, ref.shape, bound.shape)
    o = out.to(ref.device).double()
    d = (o - ref).abs()
    ok = d <= bound
    if bool(ok.all()):
        return float((d / bound.clamp_min(1e-300)).max())
    excess = torch.where(ok, torch.full_like(d, -float("inf")), torch.nan_to_num(d - bound, nan=float("inf")))
    idx = int(excess.reshape(-1).argmax())
    r, c = divmod(idx, out.shape[-1])
    ov, rv, bv = float(o.reshape(-1)[idx]), float(ref.reshape(-1)[idx]), float(bound.reshape(-1)[idx])
    raise AssertionError(f"{what}: {int((~ok).sum())} of {out.numel()} elements outside their bound; worst [{r}, {c}] = {ov!r}, ref {rv!r}, "
                         f"|diff| {abs(ov - rv):.3e} > bound {bv:.3e}" + (f"; {where(r, c)}" if where else ""))


def _rows(v):
    return rwb.per_row(v, BM)


def _product(c):
    """(fp64 product, its f32 accumulation bound): A's first K columns only"""
    P, E = eb.gemm_ref(c["A"][:, :c["K"]], c["W"])
    if c["exact"]:
        assert_exact(P)
        E = torch.zeros_like(E)
    return P, E


def _affine(c):
    dev = c["A"].device
    w = c["ln_w"] if c["ln_w"] is not None else torch.ones(D, device=dev)
    b = c["ln_b"] if c["ln_b"] is not None else torch.zeros(D, device=dev)
    return w, b


def check_fwd(c: dict, o: dict, where=None) -> dict:
    """o: t (or None), x (or None), xm, mean, rstd as the kernel stored them -> worst ratio per output"""
    what, r = f"fwd {c['form']} B={c['B']} K={c['K']}", {}
    P, E = _product(c)
    t_bound = eb.store_bf16(P, E)  # pack2bf of the accumulators
    if o.get("t") is not None:
        r["t"] = judge(o["t"], P, t_bound, what + " t", where)
    if c["resid"] is None:  # x = t: the same bits
        assert o.get("x") is not None or o.get("t") is not None
        if o.get("x") is not None:
            r["x"] = judge(o["x"], P, t_bound, what + " x = t", where)
        xs = o["x"] if o.get("x") is not None else o["t"]
    else:
        gate = _rows(c["gate"]) if c["gate"] is not None else None
        if o.get("t") is not None:  # from the stored t: f32 multiply and add, bf16 store
            ref, e = eb.gate_resid(o["t"].double(), torch.zeros_like(P), c["resid"], gate)
        else:  # t not kept: its bound goes through the gate
            ref, e = eb.gate_resid(P, t_bound, c["resid"], gate)
        r["x"] = judge(o["x"], ref, eb.store_bf16(ref, e), what + " x = resid + gate t", where)
        xs = o["x"]
    w, b = _affine(c)  # statistics and modulated rows of the ROUNDED x: the row kernel's reference and bounds
    ref, mu, rs, err, ax = rwb.ln_fwd_ref(xs, w, b, c["scale"], c["shift"], BM, c["eps"])
    r["xm"] = judge(o["xm"], ref, eb.store_bf16(ref, err), what + " xm", where)
    r["mean"] = judge(o["mean"][:, None], mu[:, None], eb.store_f32(mu, C * D * U * ax)[:, None], what + " mean", where)
    r["rstd"] = judge(o["rstd"][:, None], rs[:, None], eb.store_f32(rs, rs * (C * D * U + 4 * U))[:, None], what + " rstd", where)
    return r


def check_qk(c: dict, o: dict, where=None) -> dict:
    """o: qkv [M, 3D], q, k [B, H, n_dst, dh], rrms [M, 2]; rows outside [n_off, n_off + N) of q / k must hold their poison"""
    B, N, H, dh, rot, n_off, n_dst, M = (c[k] for k in ("B", "N", "H", "dh", "rot", "n_off", "n_dst", "M"))
    what, r = f"qk {c['form']} B={B}", {}
    P, E = _product(c)
    r["qkv"] = judge(o["qkv"], P, eb.store_bf16(P, E), what + " qkv", where)
    x = o["qkv"].double().view(M, 3, H, dh)  # from here on: the row kernel on the stored rows (row_bounds.run_qk's forward)
    pos = torch.arange(M, device=P.device) % N
    inside = torch.zeros(n_dst, dtype=torch.bool, device=P.device)
    inside[n_off:n_off + N] = True
    r["rrms"] = 0.0
    for i, (nm, sc) in enumerate((("q", c["sq"]), ("k", c["sk"]))):
        xi = x[:, i]
        where_qk = None if where is None else (lambda r_, col, i=i: where(r_, i * D + col))  # column tile 0 = q, 1 = k
        rr = 1.0 / torch.sqrt((xi**2).reshape(M, D).mean(1) + c["eps"])
        r["rrms"] = max(r["rrms"], judge(o["rrms"][:, i:i + 1], rr[:, None], eb.store_f32(rr, rr * (C * D * U + 4 * U))[:, None],
                                         f"{what} rrms {nm}", where_qk))
        xn = xi * rr[:, None, None] * sc.double().view(H, dh)
        e_n = xn.abs() * (C * D * U + 4 * U)
        ref, e_rot = xn, e_n.clone()
        if rot:
            ref, e_r = rwb.rotate(xn, c["cos"][pos], c["sin"][pos], rot)
            e_rot = e_r.clone()
            e_rot[..., 0:rot:2] += e_n[..., 0:rot:2] + e_n[..., 1:rot:2]
            e_rot[..., 1:rot:2] += e_n[..., 0:rot:2] + e_n[..., 1:rot:2]
            e_rot[..., rot:] += e_n[..., rot:]
        assert bool(eb.is_poison(o[nm][:, :, ~inside]).all()), f"{what}: {nm} written outside its row window [{n_off}, {n_off + N})"
        win = rwb.heads(o[nm], B, N, H, dh, n_off, n_dst).reshape(M, D)
        r[nm] = judge(win, ref.reshape(M, D), eb.store_bf16(ref, e_rot).reshape(M, D), f"{what} {nm}", where_qk)
    return r


def check_bwd(c: dict, o: dict, where=None) -> dict:
    """o: dx, dscale, dshift [B, D], dwb [B, 2, D] (or None), dt, dgate (or None)"""
    what, r = f"bwd {c['form']} B={c['B']} K={c['K']}", {}
    P, E = _product(c)
    e = torch.zeros_like(E) if c["exact"] else eb.store_bf16(P, E)  # |d - P|: the accumulation, then pack2bf
    w, b = _affine(c)
    s1 = _rows(c["scale"]) + 1.0
    L = rwb.ln_bwd_parts(P, c["x"], w, b, s1, c["mean"], c["rstd"])  # the reference and the local f32 terms, at d = P
    xh, e_xh, wv, bv = L["xh"], L["e_xh"], L["w"], L["b"]
    rs = c["rstd"].double()[:, None]
    m = lambda v: v.mean(1, keepdim=True)  # noqa: E731
    ke, ax = (s1 * wv).abs() * e, xh.abs()
    # dx is linear in d: |k0| e through dxh, mean(|k0| e) through c1, |xh| mean(|k0| |xh| e) through c2 ...
    prop = rs * (ke + m(ke) + ax * m(ke * ax))
    # ... and the local terms of ln_bwd_parts (row sums over D, the 8 local roundings, the error of xh) of the perturbation itself
    second = rs * ((C * D + 8) * U * (ke + m(ke) + ax * m(ke * ax)) + m(ke * ax) * e_xh + m(ke * e_xh))
    ref, err = L["dx"], L["err"] + prop + second
    if c["dres"] is not None:  # rv += rs * (...): one more f32 addition
        dr = c["dres"].double()
        ref, err = ref + dr, err + 2 * U * (L["dx"].abs() + prop + dr.abs())
    r["dx"] = judge(o["dx"], ref, eb.store_bf16(ref, err), what + " dx", where)
    # column sums over the sample's 256 rows of d and d xh: 32 lane additions and 8 slots, within (C N + 4) 2^-24 of the magnitudes
    cs = lambda v: rwb.colsum(v, BM)  # noqa: E731
    S1, S2 = cs(P), cs(P * xh)
    dm = P.abs() + e
    e1 = (C * BM + 4) * U * cs(dm) + cs(e)
    e2 = (C * BM + 4) * U * cs(dm * ax) + cs(dm * e_xh) + cs(e * ax)
    per_col = None if where is None else (lambda g, col: f"column sum of sample {g}: " + where(g * BM, col))
    r["dscale"] = judge(o["dscale"], wv * S2 + bv * S1, eb.store_f32(wv * S2 + bv * S1, wv.abs() * e2 + bv.abs() * e1 + 2 * U * (
        wv.abs() * (S2.abs() + e2) + bv.abs() * (S1.abs() + e1))), what + " dscale = w S2 + b S1", per_col)
    r["dshift"] = judge(o["dshift"], S1, eb.store_f32(S1, e1), what + " dshift = S1", per_col)
    if c["dwb"]:
        sp = c["scale"].double() + 1.0  # sc1 = 1 + scale and the product: two roundings
        for i, (S, eS, nm) in enumerate(((S2, e2, "dw"), (S1, e1, "db"))):
            r[nm] = judge(o["dwb"][:, i], sp * S, eb.store_f32(sp * S, sp.abs() * eS + 2 * U * sp.abs() * (S.abs() + eS)),
                          f"{what} {nm} = (1 + scale) S", per_col)
    if c["gate_t"] is not None:  # of dx AS STORED: the kernel rounds dx to bf16 first
        dxs = o["dx"].double()
        gr = _rows(c["gate"])
        r["dt"] = judge(o["dt"], dxs * gr, eb.store_bf16(dxs * gr, 2 * U * (dxs * gr).abs()), what + " dt = gate dx", where)
        p = dxs * c["gate_t"].double()
        r["dgate"] = judge(o["dgate"], cs(p), eb.store_f32(cs(p), (C * BM + 4) * U * cs(p.abs())), what + " dgate = sum dx t", per_col)
    return r


# ---------------------------------------------------------------------------------------------------------------- dl_gemm_nt_ssq
def check_ssq(a, w, Cout, ssq, tiles, what) -> dict:
    """C against the fp64 product; ssq[m, t] against the fp64 sum of squares of the STORED C row inside 384-wide tile t (the last one
    may be narrower): at most 384 squares summed in f32 in any grouping, ACC_C * 384 * 2^-24 of the sum, and the f32 store"""
    ref, err = eb.gemm_ref(a, w)
    r = dict(C=judge(Cout, ref, eb.store_bf16(ref, err), what + " C"))
    c2 = Cout.double() ** 2
    s = torch.stack([c2[:, BN * t:BN * (t + 1)].sum(1) for t in range(tiles)], 1)
    r["ssq"] = judge(ssq, s, eb.store_f32(s, C * BN * U * s), what + " ssq")
    return r
