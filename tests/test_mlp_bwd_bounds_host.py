"""CPU checks of tests/mlp_bwd_bounds.py: both bounds admit an emulation of a correct dl_mlp_dswiglu_recompute (f32 products, u
rounded to bf16 to nearest even, silu / dsilu through exp2 and a reciprocal) and reject the local faults that kernel can have, each
applied to ONE 32 x 8 block (one lane half of one wave's row block and unit octet); the pure-Python mirror of the kernel's tile
ownership gives every tile of every table case exactly one owner, and the table reaches every ownership situation."""

import pytest
import torch

import elementwise_bounds as eb
import mlp_bwd_bounds as mb
from oracle import synth

SHAPES = [(256, 128, 64, 64), (512, 256, 384, 128), (300, 136, 64, 192)]  # (M, F, K1, K2): the reference has no tile constraint
CORRUPTIONS = ["zeroed", "x1 <-> x3", "lane halves", "neighbour dh", "stale ring slot", "poison"]
L2E = torch.tensor(1.4426950408889634, dtype=torch.float32)


def _operands(M, F, K1, K2):
    bf = torch.bfloat16
    X = synth.normal(f"mb.x{M}.{K1}", (M, K1)).to(bf)
    Wp = synth.normal(f"mb.wp{F}.{K1}", (2 * F, K1), std=K1**-0.5).to(bf)
    dT = synth.normal(f"mb.dt{M}.{K2}", (M, K2)).to(bf)
    W2t = synth.normal(f"mb.w2{F}.{K2}", (F, K2), std=F**-0.5).to(bf)
    return X, Wp, dT, W2t


def _du(a, b, g):
    """the epilogue in f32, in the kernel's order"""
    s = 1.0 / (1.0 + torch.exp2((-a) * L2E))
    return torch.cat([(g * b) * (s * (1.0 + a * (1.0 - s))), g * (a * s)], 1)


def _truncate(x):
    return (x.contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)  # exact in bf16: no second rounding


def _block(M, F):
    return (M // 2) // 32 * 32, (F // 2) // 16 * 16


def emulate(X, Wp, dT, W2t, corrupt=None, truncating=False):
    """-> (du [M, 2F] bf16, the bf16 u = [x1 | x3] it was computed from)"""
    M, K1 = X.shape
    F = W2t.shape[0]
    i1, i3 = mb.unit_columns(F, "cpu")
    Xf, Wf = X.float(), Wp.float()
    u = Xf @ Wf.t()
    a, b = u[:, i1].to(torch.bfloat16).float(), u[:, i3].to(torch.bfloat16).float()
    ustored = torch.cat([a, b], 1).to(torch.bfloat16)
    g = dT.float() @ W2t.float().t()
    r0, c0 = _block(M, F)
    R, Cc = slice(r0, r0 + 32), slice(c0, c0 + 8)
    a, b, g = a.clone(), b.clone(), g.clone()
    if corrupt == "x1 <-> x3":
        a[R, Cc], b[R, Cc] = b[R, Cc].clone(), a[R, Cc].clone()
    elif corrupt == "lane halves":  # the block gets units c0 + 8 .. c0 + 15: the exchange between the accumulator layouts left out
        for t in (a, b, g):
            t[R, Cc] = t[R, c0 + 8:c0 + 16].clone()
    elif corrupt == "neighbour dh":
        g[R, Cc] = g[r0 + 32:r0 + 64, Cc].clone()
    elif corrupt == "stale ring slot":  # the last 64-deep k-step of phase 1 read the weights of another column tile
        other = (c0 + (128 if F >= 256 else F // 2) + torch.arange(8)) % F
        k0 = K1 - 64
        for t, idx in ((a, i1), (b, i3)):
            part = Xf[R, :k0] @ Wf[idx[Cc], :k0].t() if k0 else torch.zeros(32, 8)
            t[R, Cc] = (part + Xf[R, k0:] @ Wf[idx[other], k0:].t()).to(torch.bfloat16).float()
    d = _du(a, b, g)
    du = _truncate(d) if truncating else d.to(torch.bfloat16)
    if corrupt in ("zeroed", "poison"):
        for half in (0, F):
            blk = du[R, half + c0:half + c0 + 8]
            du[R, half + c0:half + c0 + 8] = torch.zeros_like(blk) if corrupt == "zeroed" else eb.poison_(blk.clone())
    return du, ustored


_CACHE = {}


def _case(shape):
    """operands, the correct emulation and both (ref, bound) pairs, computed once per shape"""
    if shape not in _CACHE:
        ops = _operands(*shape)
        du, u = emulate(*ops)
        _CACHE[shape] = (ops, du, u, mb.du_sound(*ops), mb.du_tight(u, ops[2], ops[3]))
    return _CACHE[shape]


def _check(du, ref, bound, F, what):
    """both halves, each on its own"""
    eb.assert_within(du[:, :F], ref[:, :F], bound[:, :F], tile=(256, 128), what=what + " du1")
    eb.assert_within(du[:, F:], ref[:, F:], bound[:, F:], tile=(256, 128), what=what + " du3")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_emulation_is_inside_both_bounds(shape):
    ops, du, u, sound, tight = _case(shape)
    _check(du, *sound, shape[1], "sound")
    _check(du, *tight, shape[1], "tight")
    assert float((tight[1] / sound[1].clamp_min(1e-300)).median()) < 0.5  # the tight bound is the tighter one


@pytest.mark.parametrize("corrupt", CORRUPTIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_corruptions_are_rejected(shape, corrupt):
    """each fault, in one 32 x 8 block, is outside both bounds in BOTH halves of du"""
    ops, _, _, sound, tight = _case(shape)
    F = shape[1]
    bad, _ = emulate(*ops, corrupt=corrupt)
    for name, (ref, bound) in (("sound", sound), ("tight", tight)):
        for lo, half in ((0, "du1"), (F, "du3")):
            with pytest.raises(AssertionError, match="outside their bound"):
                eb.assert_within(bad[:, lo:lo + F], ref[:, lo:lo + F], bound[:, lo:lo + F], tile=(256, 128), what=f"{name} {corrupt} {half}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_truncating_store_is_rejected(shape):
    """A store that truncates instead of rounding is outside the tight bound in both halves.  The sound bound rejects it as well at
    every shape here, in both halves: a truncation is off by up to one bf16 ulp of du, and where x1 and x3 sit low in their binades
    (or silu' / dsilu' is small) their half ulps add less than the missing half ulp to the sound bound."""
    ops, _, _, sound, tight = _case(shape)
    F = shape[1]
    bad, _ = emulate(*ops, truncating=True)
    for name, (ref, bound) in (("tight", tight), ("sound", sound)):
        for lo in (0, F):
            with pytest.raises(AssertionError, match="outside their bound"):
                eb.assert_within(bad[:, lo:lo + F], ref[:, lo:lo + F], bound[:, lo:lo + F], tile=(256, 128), what=name + " truncating store")


def test_tight_bound_sees_a_u_of_other_bits():
    """one recomputed x1 an ulp away from the stored one (what a different accumulation order would give) leaves the tight bound"""
    shape = SHAPES[1]
    ops, du, u, _, tight = _case(shape)
    M, F = shape[0], shape[1]
    r0, c0 = _block(M, F)
    a, b = u[:, :F].clone(), u[:, F:].float()
    a.view(torch.int16)[r0:r0 + 32, c0:c0 + 8] += 1
    bad = _du(a.float(), b, ops[2].float() @ ops[3].float().t()).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="outside their bound"):
        eb.assert_within(bad, *tight, tile=(256, 128), what="u moved by an ulp")


# ------------------------------------------------------------------------------------------------------------------ ownership
def _launches():
    return [(shape, cap) for shape, _, caps in mb.CASES for cap in caps]


@pytest.mark.parametrize("shape,cap", _launches(), ids=str)
def test_every_tile_is_owned_once(shape, cap):
    assert mb.supported(*shape)
    mb.assert_owned_once(mb.ownership(shape[0], shape[1], 256, cap))


def test_table_facts():
    """what the table says each case reaches (256 CUs)"""
    own = {(s, c): mb.ownership(s[0], s[1], 256, c) for s, c in _launches()}
    o = own[(2048, 1024, 64, 64), 0]
    assert o["grid"] == 64 and all(len(w) == 1 for w in o["walks"])
    o = own[(1280, 1792, 128, 64), 0]
    assert o["grid"] == 64 and o["csplit"] == 2 and o["np_of_xcd"].count(0) == 2 and max(len(w) for w in o["walks"]) == 2
    assert own[(1280, 1792, 128, 64), 20]["grid"] == 16
    o = own[(1280, 1664, 64, 192), 0]
    assert o["csplit"] == 1 and o["np_of_xcd"][5:] == [0, 0, 0] and all(o["np_of_xcd"][:5])
    o = own[(256, 8192, 64, 64), 0]
    assert [len(w) for w in o["walks"]] == [4 if blk & 7 < 2 else 0 for blk in range(64)]
    assert max(len(w) for w in own[(256, 8192, 64, 64), 8]["walks"]) == 32
    assert own[(16384, 128, 384, 384), 0]["np_max"] == 8
    o = own[(2304, 1152, 64, 128), 0]
    assert o["grid"] == 80 and "short last panel group" in mb.situations(o)


def test_table_reaches_every_ownership_situation():
    reached = set()
    for shape, cap in _launches():
        reached |= mb.situations(mb.ownership(shape[0], shape[1], 256, cap))
    assert reached == mb.CHECKLIST, mb.CHECKLIST ^ reached


def test_ownership_sweep():
    """every supported panel x column-tile count up to 20 x 20 under a range of budgets: no tile without an owner, none with two"""
    for panels in range(1, 21):
        for tiles_n in range(1, 21):
            if panels * tiles_n < mb.MIN_TILES:
                continue
            for cap in (0, 8, 12, 20, 64, 100, 200):
                mb.assert_owned_once(mb.ownership(panels * mb.TBM, tiles_n * mb.TU, 256, cap))


def test_refused_shapes():
    for shape in ((2000, 1024, 64, 64), (2048, 1000, 64, 64), (2048, 1024, 96, 64), (2304, 896, 64, 64)):
        assert not mb.supported(*shape)
