"""What the GroupNorm bounds of tests/groupnorm_bounds.py admit and what they reject (no GPU).

A torch-f32 emulation of the kernels' arithmetic -- pixel lanes that walk the pixels serially, lanes and channels of a group added
in one chain, the mean first and then the CENTRED second moment, f32 element-wise steps in the kernels' order, round-to-nearest bf16
stores -- must stay inside every bound on every input class of the GPU table (tests/test_gn_paths_gpu.py).  Planted mutants must each
leave at least one bound:

    chunk        a chunk of 8 channels booked wholly to the group of its first channel (C/G = 12 and C/G = 4)
    n8           n = HW * 8 instead of HW * C/G
    tail         the pixels after the last full round of the pixel lanes dropped (HW = 77, 32 lanes)
    trunc        bf16 stores that truncate
    noeps        eps omitted                      -- only the constant-group class can see it: elsewhere eps = 1e-5 moves rstd by
                                                     5e-6 / var relative, inside the bound for var >~ 2; the mutant is judged there
    film         FiLM scale applied without the 1 +
    dres         the residual gradient dropped
    dsilu_post   the SiLU derivative taken at the post-activation value
    onepass      var = E[x^2] - mean^2 from f32 sums (the formula the kernels used before): rejected on the offset32 class

The fp64 references themselves are checked against torch's fp64 autograd.
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import elementwise_bounds as eb
import groupnorm_bounds as gb

BF = torch.bfloat16
SHAPES = [(2, 77, 96, 8, 32), (2, 64, 64, 16, 32), (2, 16, 128, 32, 16)]  # (B, HW, C, G, pixel lanes): C/G = 12, 4, 4
REPORT: dict[str, tuple[float, str]] = {}


# ------------------------------------------------------------------------------------------------------------------ emulation
def lane_sum(t, lanes, drop_tail=False):
    """t f32 [B, HW, C]: lane l adds pixels l, l + lanes, ... serially, then the lanes are added serially -> [B, C]"""
    B, HW, C = t.shape
    if drop_tail:
        t = t[:, :HW // lanes * lanes]
        HW = t.shape[1]
    T = -(-HW // lanes)
    t = F.pad(t, (0, 0, 0, T * lanes - HW)).reshape(B, T, lanes, C)  # (adding +0 is exact)
    acc = torch.zeros(B, lanes, C)
    for i in range(T):
        acc = acc + t[:, i]
    out = torch.zeros(B, C)
    for l in range(lanes):
        out = out + acc[:, l]
    return out


def group_sum(t, G, chunk_bug=False):
    """t f32 [B, C] -> [B, G], the channels of a group added serially; chunk_bug: every 8-channel chunk goes to its first channel's group"""
    B, C = t.shape
    cg = C // G
    out = torch.zeros(B, G)
    for c in range(C):
        g = (c // 8 * 8) // cg if chunk_bug else c // cg
        out[:, g] = out[:, g] + t[:, c]
    return out


def store(t, mut):
    if mut == "trunc":
        return (t.float().view(torch.int32) & -65536).view(torch.float32).to(BF)
    return t.to(BF)


def silu32(h):
    return h * (1.0 / (1.0 + torch.exp(-h)))


def dsilu32(h):
    s = 1.0 / (1.0 + torch.exp(-h))
    return s * (1.0 + h * (1.0 - s))


def emu_fwd(x, w, b, sc, sh, silu, G, lanes, mut=""):
    """-> mean, rstd f32 [B, G], out bf16 [B, HW, C]"""
    B, HW, C = x.shape
    cg = C // G
    n = torch.tensor(float(HW * (8 if mut == "n8" else cg)))
    X = x.float()
    eps = 0.0 if mut == "noeps" else gb.EPS
    mu = group_sum(lane_sum(X, lanes, mut == "tail"), G, mut == "chunk") / n
    muc = mu.repeat_interleave(cg, 1)[:, None, :]
    if mut == "onepass":
        q = group_sum(lane_sum(X * X, lanes), G) / n
        var = (q - mu * mu).clamp_min(0.0)
    else:
        d = X - muc
        var = group_sum(lane_sum(d * d, lanes, mut == "tail"), G, mut == "chunk") / n
    r = torch.rsqrt(var + eps)
    y = (X - muc) * r.repeat_interleave(cg, 1)[:, None, :] * w + b
    if sc is not None:
        y = y * ((0.0 if mut == "film" else 1.0) + sc.float()[:, None, :]) + sh.float()[:, None, :]
    return mu, r, store(silu32(y) if silu else y, mut)


def emu_bwd(dout, x, stats, w, b, sc, sh, silu, dres, dw0, db0, G, lanes, mut=""):
    B, HW, C = x.shape
    cg = C // G
    n = float(HW * (8 if mut == "n8" else cg))
    X, D = x.float(), dout.float()
    muc, rc = (stats[..., i].repeat_interleave(cg, 1)[:, None, :] for i in (0, 1))
    xh = (X - muc) * rc
    y = xh * w + b
    s1 = 1.0 + sc.float()[:, None, :] if sc is not None else torch.ones(B, 1, C)
    h = y * s1 + (sh.float()[:, None, :] if sc is not None else 0.0)
    if silu:
        dh = D * dsilu32(silu32(h) if mut == "dsilu_post" else h)
    else:
        dh = D
    dy = dh * s1
    tail = mut == "tail"
    S = [lane_sum(t, lanes, tail) for t in (dh * y, dh, dy * xh, dy)]
    res = {"dw": dw0 + S[2].sum(0), "db": db0 + S[3].sum(0)}
    if sc is not None:
        res["dfilm_scale"], res["dfilm_shift"] = store(S[0], mut), store(S[1], mut)
    A = (group_sum(w * S[3], G, mut == "chunk") * (1.0 / n)).repeat_interleave(cg, 1)[:, None, :]
    Bv = (group_sum(w * S[2], G, mut == "chunk") * (1.0 / n)).repeat_interleave(cg, 1)[:, None, :]
    dx = rc * (dy * w - A - xh * Bv)
    if dres is not None and mut != "dres":
        dx = dx + dres.float()
    res["dx"] = store(dx, mut)
    return res


# ------------------------------------------------------------------------------------------------------------------ one run
def ratios(shape, cls, mut="", film=True, silu=True, seed=0):
    """worst |diff| / bound per output of the (mutated) emulation on one shape and input class"""
    B, HW, C, G, lanes = shape
    gen = torch.Generator().manual_seed(seed + 1000 * gb.CLASSES.index(cls))
    n = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    x = gb.make_x(cls, B, HW, C, G, gen, "cpu")
    w, b = 1.0 + 0.2 * n(C), 0.2 * n(C)
    sc, sh = ((0.3 * n(B, C)).to(BF), (0.3 * n(B, C)).to(BF)) if film else (None, None)
    dout, dres = n(B, HW, C).to(BF), n(B, HW, C).to(BF)
    dw0, db0 = n(C), n(C)
    depth = -(-HW // lanes) + lanes + C // G
    ref = gb.fwd_ref(x, w, b, sc, sh, silu, G, gb.EPS, depth)
    mu, r, out = emu_fwd(x, w, b, sc, sh, silu, G, lanes, mut)
    got = {"mean": mu, "rstd": r, "out": out}
    # the backward takes CORRECT f32 statistics: a mutant of the backward is judged on the backward's own outputs
    stats = torch.stack([ref["mean"][0], ref["rstd"][0]], -1).float()
    ref.update(gb.bwd_ref(dout, x, stats, w, b, sc, sh, silu, dres, dw0, db0, G))
    got.update(emu_bwd(dout, x, stats, w, b, sc, sh, silu, dres, dw0, db0, G, lanes, mut))
    return {k: gb.worst_ratio(got[k], *ref[k]) for k in got}


# ------------------------------------------------------------------------------------------------------------------ tests
def test_references_match_fp64_autograd():
    B, HW, C, G = 2, 33, 48, 4
    gen = torch.Generator().manual_seed(5)
    n = lambda *s: torch.randn(s, generator=gen)  # noqa: E731
    x = gb.make_x("scaled", B, HW, C, G, gen, "cpu")
    w, b, sc, sh = 1.0 + 0.2 * n(C), 0.2 * n(C), (0.3 * n(B, C)).to(BF), (0.3 * n(B, C)).to(BF)
    dout, dres = n(B, HW, C).to(BF), n(B, HW, C).to(BF)
    for film in (False, True):
        for silu in (False, True):
            leaves = [t.double().requires_grad_(True) for t in (x, w, b, sc, sh)]
            xd, wd, bd, scd, shd = leaves
            y = F.group_norm(xd.permute(0, 2, 1), G, wd, bd, gb.EPS).permute(0, 2, 1)
            if film:
                y = y * (1.0 + scd[:, None]) + shd[:, None]
            if silu:
                y = F.silu(y)
            (y * dout.double()).sum().backward()
            ref = gb.fwd_ref(x, w, b, sc if film else None, sh if film else None, silu, G, gb.EPS, 8)
            assert float((ref["out"][0] - y.detach()).abs().max()) < 1e-12
            st = torch.stack([ref["mean"][0], ref["rstd"][0]], -1)  # (fp64 statistics: the exact gradient)
            br = gb.bwd_ref(dout, x, st, w, b, sc if film else None, sh if film else None, silu, dres, torch.zeros(C), torch.zeros(C), G)
            assert float((br["dx"][0] - dres.double() - xd.grad).abs().max()) < 1e-11
            assert float((br["dw"][0] - wd.grad).abs().max()) < 1e-11 and float((br["db"][0] - bd.grad).abs().max()) < 1e-11
            if film:
                assert float((br["dfilm_scale"][0] - scd.grad).abs().max()) < 1e-11
                assert float((br["dfilm_shift"][0] - shd.grad).abs().max()) < 1e-11


@pytest.mark.parametrize("cls", gb.CLASSES)
def test_emulation_stays_inside_every_bound(cls):
    for shape in SHAPES:
        for film, silu in ((True, True), (False, False), (True, False), (False, True)):
            for out, ratio in ratios(shape, cls, film=film, silu=silu).items():
                if ratio > REPORT.get(out, (-1.0, ""))[0]:
                    REPORT[out] = (ratio, f"{cls} {shape}")
                assert ratio <= 1.0, f"{cls} {shape} film={film} silu={silu}: {out} at {ratio:.3f} of its bound"


MUTANTS = [  # (mutant, shape, input class, outputs of which at least one must leave its bound)
    ("chunk", SHAPES[0], "scaled", ("mean", "rstd", "out")),
    ("chunk", SHAPES[1], "scaled", ("mean", "rstd", "out")),
    ("chunk", SHAPES[0], "scaled", ("dx",)),
    ("n8", SHAPES[0], "scaled", ("mean", "rstd")),
    ("n8", SHAPES[1], "scaled", ("dx",)),
    ("tail", SHAPES[0], "scaled", ("mean", "rstd")),
    ("tail", SHAPES[0], "scaled", ("dw", "db", "dx")),
    ("trunc", SHAPES[1], "scaled", ("out",)),
    ("trunc", SHAPES[1], "scaled", ("dx", "dfilm_scale", "dfilm_shift")),
    ("noeps", SHAPES[1], "const", ("rstd", "out")),
    ("film", SHAPES[1], "scaled", ("out",)),
    ("dres", SHAPES[1], "scaled", ("dx",)),
    ("dsilu_post", SHAPES[1], "scaled", ("dx", "dw", "db")),
    ("onepass", SHAPES[0], "offset32", ("rstd",)),
    ("onepass", SHAPES[1], "offset32", ("rstd",)),
]


@pytest.mark.parametrize("mut,shape,cls,outs", MUTANTS, ids=[f"{m[0]}-cg{m[1][2] // m[1][3]}-{m[3][0]}" for m in MUTANTS])
def test_mutant_leaves_a_bound(mut, shape, cls, outs):
    r = ratios(shape, cls, mut)
    verdict = {o: round(r[o], 2) for o in outs}
    print(f"mutant {mut} on {cls} {shape}: |diff| / bound {verdict}")
    assert any(not r[o] <= 1.0 for o in outs), f"mutant {mut} passes: {verdict}"


def test_onepass_is_invisible_without_an_offset():
    """why the offset classes exist: on zero-offset groups the one-pass variance sits inside the bound"""
    r = ratios(SHAPES[1], "spike", "onepass")
    assert r["rstd"] <= 1.0, r


def test_report():
    """runs last: the worst |diff| / bound of the unmutated emulation per output"""
    print("\nemulation, worst |diff| / bound: " + "; ".join(f"{o} {r:.3f} ({w})" for o, (r, w) in sorted(REPORT.items())))
    assert REPORT and all(r <= 1.0 for r, _ in REPORT.values())
