"""CPU checks of tests/row_gemm_bounds.py.  Each mode of the row-complete GEMMs (csrc/gemm_rows_body.h) is emulated in f32 torch in
the kernel's order of operations -- accumulators rounded to bf16 before the epilogue, statistics of the rounded x, dx rounded before
dt / dgate, column sums per wave and then in wave order -- on the GPU test's own inputs.  Every bound admits the emulation of every
case of the GPU table and rejects each local fault the kernel can have, applied to ONE tile (one fragment, one pair of rows, one
wave's prefetch, one sample's modulation row, one wave's column-sum slot, one walk's second tile).  The exact-product generator is
exact at every K it is used with, and the Python mirror of the launcher gives every tile of every (M, cap) exactly one owner.
Every listed fault is rejected by the sound bounds on these inputs; none had to be reported as undetectable."""

import pytest
import torch

import elementwise_bounds as eb
import row_gemm_bounds as rb

D, BM = rb.D, rb.BM
INV_D = torch.tensor(1.0 / D, dtype=torch.float32)
WROWS = torch.tensor([[rb.row_of(s, w) for s in range(32)] for w in range(8)])  # [wave, step] -> tile row
TILE = 1  # the tile (= sample) the local faults are applied to
FRAG = (TILE * BM + 96, 232)  # first row / column of the zeroed 32 x 8 block of accumulators (wave 3 = wm 1, wn 1; fragment i 1, j 1; registers 4..7)


def _truncate(x):
    return (x.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)


def _store(x, mut, name):
    return _truncate(x) if mut == "truncating " + name else x.to(torch.bfloat16)


def _stale(v, wave=3):
    """row operand one row behind in one wave's walk over tile TILE: step s gets the row fetched for step s - 1"""
    out = v.clone()
    rows = TILE * BM + WROWS[wave]
    out[rows[1:]] = v[rows[:-1]]
    return out


def _acc(c, mut, tiles_n):
    """the f32 accumulators [M, 384 tiles_n] as the epilogue packs them"""
    K = c["K"]
    A, W = c["A"][:, :K].float(), c["W"].float()
    acc = A @ W.t()
    if mut == "stale ring slot":  # the last k-step of the second tile of workgroup 0's walk read the first tile's operands
        t1, t2 = rb.walks((c["M"] // BM) * tiles_n)[0][:2]
        (m1, n1), (m2, n2) = divmod(t1, tiles_n), divmod(t2, tiles_n)
        R1, C1, R2, C2 = (slice(v * n, v * n + n) for v, n in ((m1, BM), (n1, D), (m2, BM), (n2, D)))
        k0 = K - 64
        acc[R2, C2] = A[R2, :k0] @ W[C2, :k0].t() + A[R1, k0:] @ W[C1, k0:].t()
    if mut == "zeroed fragment":
        acc[FRAG[0]:FRAG[0] + 32, FRAG[1]:FRAG[1] + 8] = 0
    tb = acc.to(torch.bfloat16)
    if mut == "rows exchanged":  # a wrong row_of: two rows of the dumped piece processed as each other
        r = TILE * BM + torch.tensor([5, 37])
        tb[r] = tb[r.flip(0)]
    return tb


def _mod_rows(c, mut):
    g = torch.arange(c["M"]) // BM
    if mut == "neighbour modulation":
        g[TILE * BM:(TILE + 1) * BM] = TILE + 1
    return g


def _w_b(c):
    return (c["ln_w"] if c["ln_w"] is not None else torch.ones(D)), (c["ln_b"] if c["ln_b"] is not None else torch.zeros(D))


def emulate_fwd(c, mut=None):
    tb = _acc(c, mut, 1)
    t, g = tb.float(), _mod_rows(c, mut)
    if c["resid"] is not None:
        rs_ = _stale(c["resid"].float()) if mut == "stale resid" else c["resid"].float()
        x = (rs_ + c["gate"].float()[g] * t if c["gate"] is not None else rs_ + t).to(torch.bfloat16)
    else:
        x = tb
    xf = x.float()
    mu = xf.sum(1) * INV_D
    dd = xf - mu[:, None]
    rs = torch.rsqrt((dd * dd).sum(1) * INV_D + c["eps"])
    w, b = _w_b(c)
    xm = (dd * rs[:, None] * w + b) * (1.0 + c["scale"].float()[g]) + c["shift"].float()[g]
    return dict(t=tb if c["t_out"] else None, x=x, xm=_store(xm, mut, "xm"), mean=mu, rstd=rs)


def emulate_bwd(c, mut=None):
    B = c["B"]
    d, g = _acc(c, mut, 1).float(), _mod_rows(c, mut)
    x = c["x"].float()
    dres = c["dres"].float() if c["dres"] is not None else torch.zeros_like(x)
    if mut == "stale x / dres":
        x, dres = _stale(x), _stale(dres)
    w, b = _w_b(c)
    xh = (x - c["mean"][:, None]) * c["rstd"][:, None]
    dxh = d * ((1.0 + c["scale"].float()[g]) * w)
    c1, c2 = dxh.sum(1, keepdim=True) * INV_D, (dxh * xh).sum(1, keepdim=True) * INV_D
    dxb = _store(dres + c["rstd"][:, None] * (dxh - c1 - xh * c2), mut, "dx")
    parts = [d, d * xh]
    o = dict(dx=dxb, dt=None, dgate=None, dwb=None)
    if c["gate_t"] is not None:  # from dx as rounded
        gt = _stale(c["gate_t"].float()) if mut == "stale gate_t" else c["gate_t"].float()
        o["dt"] = (dxb.float() * c["gate"].float()[g]).to(torch.bfloat16)
        parts.append(dxb.float() * gt)
    S = []
    for p in parts:  # the wave's 32 rows in its lanes, then the eight slots in wave order
        slots = p.view(B, BM, D)[:, WROWS].sum(2)
        if mut == "missing slot":
            slots[TILE, 5] = 0
        acc = torch.zeros(B, D)
        for wv in range(8):
            acc = acc + slots[:, wv]
        S.append(acc)
    o["dscale"] = w * S[1] + (0 if mut == "dscale without b S1" else b * S[0])
    o["dshift"] = S[0]
    if c["gate_t"] is not None:
        o["dgate"] = S[2]
    if c["dwb"]:
        sp = 1.0 if mut == "dwb without 1 + scale" else 1.0 + c["scale"].float()
        o["dwb"] = torch.stack([sp * S[1], sp * S[0]], 1)
    return o


def emulate_qk(c, mut=None):
    B, N, H, dh, rot, n_off, n_dst, M = (c[k] for k in ("B", "N", "H", "dh", "rot", "n_off", "n_dst", "M"))
    tb = _acc(c, mut, 3)
    o = dict(qkv=tb, rrms=torch.empty(M, 2))
    pos = torch.arange(M) % (256 if mut == "rope by row % 256" else N)
    for i, (nm, sc) in enumerate((("q", c["sq"]), ("k", c["sk"]))):
        t = tb[:, i * D:(i + 1) * D].float()
        rq = torch.rsqrt((t * t).sum(1) * INV_D + c["eps"])
        v = (t * rq[:, None] * sc).view(M, H, dh).clone()
        if rot:
            cc, ss = c["cos"][pos][:, None, :], c["sin"][pos][:, None, :]
            a, b = v[..., 0:rot:2].clone(), v[..., 1:rot:2].clone()
            v[..., 0:rot:2], v[..., 1:rot:2] = a * cc - b * ss, a * ss + b * cc
        out = eb.poison_(torch.empty(B, H, n_dst, dh, dtype=torch.bfloat16))
        off = 0 if mut == "n_off ignored" else n_off
        out[:, :, off:off + N] = _store(v, mut, "q" if nm == "q" else "-").view(B, N, H, dh).permute(0, 2, 1, 3)
        o[nm], o["rrms"][:, i] = out, rq
    return o


MODES = {"fwd": (rb.fwd_case, emulate_fwd, rb.check_fwd, 1), "bwd": (rb.bwd_case, emulate_bwd, rb.check_bwd, 1),
         "qk": (rb.qk_case, emulate_qk, rb.check_qk, 3)}
_CASES = {}


def _case(mode, key, exact=False):
    if (mode, key, exact) not in _CASES:
        _CASES[mode, key, exact] = MODES[mode][0](*key[:-1], exact=exact)
    return _CASES[mode, key, exact]


def _check(mode, c, o):
    return MODES[mode][2](c, o, rb.locator(c["M"], MODES[mode][3], c["K"]))


ALL = [("fwd", k, False) for k in rb.FWD_CASES] + [("bwd", k, False) for k in rb.BWD_CASES] + [("qk", k, False) for k in rb.QK_CASES] + [
    ("fwd", rb.FWD_EXACT, True), ("bwd", rb.BWD_EXACT, True), ("qk", rb.QK_EXACT, True)]


@pytest.mark.parametrize("mode,key,exact", ALL, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_emulation_is_inside_every_bound(mode, key, exact):
    c = _case(mode, key, exact)
    ratios = _check(mode, c, MODES[mode][1](c))
    print(mode, key, "exact" if exact else "", {k: round(v, 3) for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values())


# the smallest inputs of the GPU table on which each fault exists: a walk of two tiles (B = 9), K = 192 (three k-steps)
SMALL = {"fwd": (9, 192, "block", 0), "bwd": (9, 192, "full", 0), "qk": (9, 256, 6, 64, 32, 77, 356, 0), "qk320": (8, 320, 6, 64, 32, 77, 420, 0)}
MUTANTS = [
    ("fwd", "zeroed fragment"), ("fwd", "rows exchanged"), ("fwd", "stale resid"), ("fwd", "truncating xm"), ("fwd", "neighbour modulation"),
    ("fwd", "stale ring slot"),
    ("bwd", "zeroed fragment"), ("bwd", "rows exchanged"), ("bwd", "stale x / dres"), ("bwd", "stale gate_t"), ("bwd", "truncating dx"),
    ("bwd", "neighbour modulation"), ("bwd", "missing slot"), ("bwd", "dscale without b S1"), ("bwd", "dwb without 1 + scale"),
    ("bwd", "stale ring slot"),
    ("qk", "zeroed fragment"), ("qk", "rows exchanged"), ("qk", "truncating q"), ("qk", "n_off ignored"), ("qk", "stale ring slot"),
    ("qk320", "rope by row % 256"),
]


@pytest.mark.parametrize("which,mut", MUTANTS, ids=lambda v: str(v).replace(" ", "_"))
def test_mutants_are_rejected(which, mut):
    mode = which[:2] if which.startswith("qk") else which
    c = _case(mode, SMALL[which])
    _check(mode, c, MODES[mode][1](c))  # (the unmutated emulation passes on these inputs)
    with pytest.raises(AssertionError, match="outside their bound|outside its row window"):
        _check(mode, c, MODES[mode][1](c, mut))


@pytest.mark.parametrize("mode,mut", [("fwd", "truncating xm"), ("bwd", "truncating dx"), ("qk", "truncating q"), ("bwd", "missing slot")])
def test_exact_product_cases_reject_the_epilogue_faults_at_the_row_kernels_own_bounds(mode, mut):
    key = {"fwd": rb.FWD_EXACT, "bwd": rb.BWD_EXACT, "qk": rb.QK_EXACT}[mode]
    c = _case(mode, key, True)
    with pytest.raises(AssertionError, match="outside their bound"):
        _check(mode, c, MODES[mode][1](c, mut))


def test_a_mutant_failure_names_its_owner():
    c = _case("fwd", SMALL["fwd"])
    with pytest.raises(AssertionError) as e:
        _check("fwd", c, emulate_fwd(c, "zeroed fragment"))
    msg = str(e.value)
    assert " t:" in msg and "workgroup 1 of 8, tile 1 = (1, 0), number 0 of its walk" in msg and "accumulated by wave 3 fragment (j 1, i 1)" in msg, msg
    c = _case("qk", SMALL["qk"])
    o = emulate_qk(c)
    o["k"][:, :, c["n_off"]:c["n_off"] + c["N"]] = emulate_qk(c, "truncating q")["q"][:, :, c["n_off"]:c["n_off"] + c["N"]]  # k := a wrong q
    with pytest.raises(AssertionError) as e:
        _check("qk", c, o)
    msg = str(e.value)
    assert " k:" in msg and "of 24, tile" in msg and ", 1), number" in msg, msg  # column tile 1 = k


# ------------------------------------------------------------------------------------------------------------------ exact products
@pytest.mark.parametrize("K", sorted({64, 192, 384, 1152, 1536}))
def test_exact_product_generator_is_exact(K):
    a, w = rb.exact_operands(f"host.{K}", 512, 384, K)  # (asserts bf16(ref) == ref itself)
    ref = a.double() @ w.double().t()
    assert torch.equal((a.float() @ w.float().t()).double(), ref)  # and f32 accumulation is exact
    assert float(ref.abs().max()) > 1.0 and set(torch.unique(a.float()).tolist()) == {-1.0, 0.0, 1.0}
    assert set(torch.unique(w.float() * 8).tolist()) == {-1.0, 0.0, 1.0}


# ------------------------------------------------------------------------------------------------------------------ launcher mirror
def _launches():
    out = {(B, 1, cap) for B, _, _, cap in rb.FWD_CASES + rb.BWD_CASES + [rb.FWD_EXACT, rb.BWD_EXACT]}
    out |= {(k[0] * k[1] // BM, 3, k[-1]) for k in rb.QK_CASES + [rb.QK_EXACT]}
    return sorted(out)


@pytest.mark.parametrize("panels,tiles_n,cap", _launches())
def test_every_tile_is_owned_once(panels, tiles_n, cap):
    rb.assert_owned_once(panels * tiles_n, 256, cap)


def test_mirror_facts():
    assert sorted(rb.ROW_OWNER) == list(range(BM))  # row_of is a bijection of (wave, step) onto the tile's rows
    assert rb.grid_of(8) == 8 and rb.grid_of(9) == 8 and rb.grid_of(27) == 24 and rb.grid_of(20, cap=8) == 8 and rb.grid_of(60, cap=8) == 8
    assert rb.grid_of(300) == 256 and rb.grid_of(300, n_cu=304) == 296
    assert sorted(len(w) for w in rb.walks(9)) == [1] * 7 + [2]
    assert sorted(len(w) for w in rb.walks(27)) == [1] * 21 + [2] * 3
    assert sorted(len(w) for w in rb.walks(20, cap=8)) == [2] * 4 + [3] * 4
    assert rb.walks(64)[9] == [rb.slot_of(9, 64)] == [9]  # (9 & 7) * 8 + (9 >> 3)
    for ntiles in range(8, 200):
        for cap in (0, 8, 12, 20, 100):
            rb.assert_owned_once(ntiles, 256, cap)
