"""What the weight-gradient checks of tests/conv_wgrad_bounds.py admit and what they reject (no GPU).

  * the fp64 reference g[(tap, ci), co] against torch's fp64 autograd of conv2d on every map geometry of the GPU table
    (tests/test_conv_wgrad_paths_gpu.py takes its cases from the same list): pins tap = 3 ky + kx independently of the library;
  * the table's expected path codes and range counts against a mirror of the dispatcher's arithmetic for 256 CUs;
  * the f32 emulation of the kernels' pixel walk: inside the bound on `gauss` inputs, EQUAL to the reference on `exact` inputs, in both
    forms, on every case of the table;
  * every mutant of conv_wgrad_bounds.MUTANTS, planted into ONE tile (and one tap, step or range where that applies) of the smallest
    table case in which it exists: rejected by the gauss bound or by exact equality.  The mode that rejects it is recorded; the last
    test prints the table and fails if a mutant was left out or passed.  Mutant (c) is visible only because the rows below x are
    poisoned: the dY rows it multiplies are zero, and 0 * NaN is what shows;
  * why the exact class exists: at 8192 pixels a result rounded to bf16 is inside the gauss bound, and not equal.
"""

from __future__ import annotations

import pytest
import torch
import torch.nn.functional as F

import conv_wgrad_bounds as wb

VERDICTS: dict[str, dict] = {}
WORST: dict[str, tuple[float, str]] = {}
COL0 = 16
# table cases this file does not emulate (fp64 operand too large for a few seconds on a CPU): none
SKIPPED_ON_HOST: list[str] = []


def operands(c, mode, seed=1):
    x, dy, init = wb.make_inputs(c, mode, seed, "cpu")
    xbuf, xw = wb.x_operand(x, c.W, col0=COL0)
    _, dyw = wb.dy_operand(dy, c.R)
    return xbuf, xw, dyw, init


def test_table_matches_the_dispatch_arithmetic():
    for c in wb.CASES:
        p = wb.plan(c)
        assert (p.path, p.nparts) == (c.path, c.nparts), f"{c.id}: the dispatcher's rules give {p}"
    assert {c.path for c in wb.CASES} == set(wb.PATHS[1:])
    assert len({c.id for c in wb.CASES}) == len(wb.CASES)


@pytest.mark.parametrize("geom", sorted({(c.B, c.H, c.W) for c in wb.CASES}), ids=lambda g: "x".join(map(str, g)))
def test_reference_matches_fp64_autograd(geom):
    """g[(3 ky + kx, ci), co] - init == d/dw[co, ci, ky, kx] of sum(conv2d(x, w, padding=1) * dY)"""
    B, H, W = geom
    c = wb.Case(B, H, W, 3, 8, "", 0)
    x, dy, init = wb.make_inputs(c, "gauss", 7, "cpu")
    dyp = torch.zeros(c.R, c.Co, dtype=wb.BF)
    dyp[:c.npix] = dy
    ref, bound = wb.reference(x, dyp, c, init)
    xn = x.double().reshape(B, H, W, c.Ci).permute(0, 3, 1, 2)
    w = torch.zeros(c.Co, c.Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    (F.conv2d(xn, w, padding=1) * dy.double().reshape(B, H, W, c.Co).permute(0, 3, 1, 2)).sum().backward()
    assert float((wb.to_dw(ref - init.double(), c.Ci) - w.grad).abs().max()) < 1e-10
    assert bool((bound > 0).all())
    ref0, _ = wb.reference(x, dyp, c, None)
    assert torch.equal(ref0, ref - init.double())


@pytest.mark.parametrize("form", wb.FORMS)
@pytest.mark.parametrize("case", [c for c in wb.CASES if c.id not in SKIPPED_ON_HOST], ids=lambda c: c.id)
def test_emulation_inside_the_bound_and_exact(case, form):
    p = wb.plan(case)
    for mode in wb.MODES:
        xbuf, xw, dyw, init = operands(case, mode)
        ref, bound = wb.reference(xw, dyw, case, init if form == "atomic" else None)
        got = wb.emulate(xbuf, COL0, dyw, init, case, p, form, seed=3)
        if form == "parts":
            assert got.shape[0] == case.nparts and bool(torch.isfinite(got).all())
            got = got.double().sum(0)
        if mode == "gauss":
            r = wb.worst_ratio(got, ref, bound)
            if r > WORST.get(p.path, (-1.0, ""))[0]:
                WORST[p.path] = (r, case.id)
        assert not wb.rejected(got, ref, bound, mode), f"{case.id} {form} {mode}: the unmutated emulation is rejected"


def smallest_case(m, family=""):
    cs = [c for c in wb.CASES if wb.mutant_exists(m, c, wb.plan(c)) and c.path.startswith(family)]
    return min(cs, key=lambda c: (c.npix * c.Ci * c.Co, c.id))


def verdict(m, c, form):
    """{mode: rejected} of mutant m on case c"""
    p = wb.plan(c)
    out = {}
    for mode in wb.MODES:
        xbuf, xw, dyw, init = operands(c, mode)
        ref, bound = wb.reference(xw, dyw, c, init if form == "atomic" else None)
        got = wb.emulate(xbuf, COL0, dyw, init, c, p, form, seed=3, mut=m)
        out[mode] = wb.rejected(got.double().sum(0) if form == "parts" else got, ref, bound, mode)
    return out


@pytest.mark.parametrize("m", list(wb.MUTANTS))
def test_mutant_is_rejected(m):
    c = smallest_case(m)
    forms = {"j": ("atomic",), "k": ("parts",)}.get(m, wb.FORMS)
    v = {form: verdict(m, c, form) for form in forms}
    owner = {form: next((mode for mode in wb.MODES if r[mode]), None) for form, r in v.items()}
    VERDICTS[m] = {"case": c.id, "verdict": v, "owner": owner}
    print(f"mutant ({m}) {wb.MUTANTS[m]} on {c.id} [{wb.plan(c).path}]: rejected {v}")
    for form in forms:
        assert owner[form] is not None, f"mutant ({m}) passes both modes in the {form} form on {c.id}"


@pytest.mark.parametrize("m", [m for m in wb.MUTANTS if m != "i"])  # (i) lives in the 384-row tiles of gemm_tn_big_k only
def test_mutant_is_rejected_in_a_halo_tile(m):
    """the same faults in the halo kernel's tile (all nine taps of a 64-channel chunk), on its smallest case that has them"""
    c = smallest_case(m, "WG_HALO")
    forms = {"j": ("atomic",), "k": ("parts",)}.get(m, wb.FORMS)
    for form in forms:
        v = verdict(m, c, form)
        print(f"mutant ({m}) on {c.id} [{wb.plan(c).path}] {form}: rejected {v}")
        assert any(v.values()), f"mutant ({m}) passes both modes in the {form} form on {c.id}"


def test_bf16_rounding_at_8192_pixels_is_inside_the_bound_and_not_equal():
    """why the exact class exists: the accumulation bound grows with R^2 and at R = 8192 admits a result rounded to bf16"""
    c = next(c for c in wb.CASES if (c.B, c.H, c.W) == (8, 32, 32))
    v = verdict("l", c, "atomic")
    assert v == {"gauss": False, "exact": True}, v


def test_every_mutant_was_judged_and_rejected():
    """runs last: the verdict table; no mutant left out, none passed"""
    lines = [f"  ({m}) {wb.MUTANTS[m]}: {VERDICTS[m]['case']}, owner {VERDICTS[m]['owner']}" for m in wb.MUTANTS if m in VERDICTS]
    print("\nmutants rejected:\n" + "\n".join(lines))
    print("emulation, worst |diff| / bound (gauss): " + "; ".join(f"{k} {r:.3f} ({w})" for k, (r, w) in sorted(WORST.items())))
    print(f"table cases not emulated on the host: {SKIPPED_ON_HOST or 'none'}")
    assert sorted(VERDICTS) == sorted(wb.MUTANTS) == list("abcdefghijkl")
    assert all(o is not None for v in VERDICTS.values() for o in v["owner"].values())
