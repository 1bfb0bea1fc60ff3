"""What the bounds of tests/step_bounds.py admit and what they reject, on the CPU, on the inputs tests/test_step_paths_gpu.py uses.

Admits: the kernels' formulas evaluated in torch f32, once with every product and sum rounded separately and once with each
a * b + c as one fused multiply-add (emulated through fp64, then rounded), stay inside every bound; the worst ratio is printed.
Rejects: each wrong kernel of the list below leaves its bound, or fails the bit comparison, on those same inputs.
"""

from __future__ import annotations

import math

import pytest
import torch

import elementwise_bounds as eb
import f32_bounds as fb
import step_bounds as sb

F32 = torch.float32
N_HOST = 1027  # the GPU table's size with a float4 body and a 3-element tail


def T(x: float) -> torch.Tensor:
    return torch.tensor(x, dtype=F32)


def fma32(a, b, c):
    """fmaf through fp64: the product of two f32 values is exact there, the sum is rounded to 53 bits and then to 24"""
    return (a.double() * b.double() + c.double()).float()


def mad(a, b, c, fma: bool):
    return fma32(a, b, c) if fma else a * b + c


# ------------------------------------------------------------------------------------------------------------------ emulated kernels
def adamw_f32(p, g, m, v, S, fma: bool, mutant: str | None = None):
    gr = g * T(S["gs"])
    gr_v = g if mutant == "scale_m_only" else gr  # v sees the unscaled gradient
    b1, b2, omb1, omb2, eps = T(S["b1"]), T(S["b2"]), T(S["omb1"]), T(S["omb2"]), T(S["eps"])
    ilr, isb = T(S["ilr"]), T(S["isb"])
    if mutant == "bias_swapped":
        ilr, isb = T(sb.f32c(S["lr"] / S["bc2"])), T(sb.f32c(1.0 / math.sqrt(S["bc1"])))
    mj = mad(b1, m, omb1 * gr, fma)
    vj = mad(gr_v, omb2 * gr_v, b2 * v, fma)
    if mutant == "eps_in_sqrt":
        den = torch.sqrt(vj + eps) * isb
    elif mutant == "eps_scaled":
        den = (torch.sqrt(vj) + eps) * isb
    else:
        den = mad(torch.sqrt(vj), isb, eps, fma)
    q = mj / den
    decay = mad(-T(S["lr"]), T(S["wd"]), T(1.0), fma)
    if mutant == "wd_after":
        pj = (p - ilr * q) * decay
    else:
        pj = fma32(decay, p, -(ilr * q)) if fma else decay * p - ilr * q
    return {"p": pj, "m": mj, "v": vj}


def flow_f32(x, e, t, fma: bool, mutant: str | None = None):
    tt = t[:, None].expand_as(x).clone()
    if mutant == "neighbour_t":  # the float4 that ends a sample reads the next sample's t
        tt[:, -4:] = torch.roll(t, -1)[:, None]
    return {"z": mad(T(1.0) - tt, x, tt * e, fma)}


def ddpm_f32(x, e, t, sqrt_ab, ab, fma: bool, mutant: str | None = None):
    ti = t.long()
    if mutant == "t_off_by_one":
        ti = torch.where(ti + 1 < ab.numel(), ti + 1, ti - 1)
    ca, cb = sqrt_ab[ti][:, None], torch.sqrt(T(1.0) - ab[ti])[:, None]
    return {"xt": mad(ca.expand_as(x), x, cb * e, fma)}


def ema_f32(ema, p, beta, fma: bool, mutant: str | None = None):
    w = T(sb.f32c(beta)) if mutant == "beta" else T(1.0) - T(sb.f32c(beta))
    return {"ema": mad(w, p - ema, ema, fma)}


def worst(got, ref) -> float:
    return max(fb.judge(got, ref).values())


def tables(Tn: int):
    return sb.ddpm_tables(Tn)


def adamw_cases():
    for name, lr, betas, eps, wd, step, gs, coef in sb.ADAMW_HYPERS:
        for clip in (False, True):
            yield f"{name}{'-clip' if clip else ''}", sb.adamw_scalars(lr, betas, eps, wd, step, gs, coef if clip else None)


# ------------------------------------------------------------------------------------------------------------------ admits
@pytest.mark.parametrize("fma", (False, True), ids=("separate", "fused"))
def test_bounds_admit_the_f32_formulas(fma):
    w = {}
    for n in (5, N_HOST, 4099):
        p, g, m, v = sb.adamw_inputs(n, seed=n)
        for name, S in adamw_cases():
            r = fb.judge(adamw_f32(p, g, m, v, S, fma), sb.adamw_ref(p, g, m, v, S))
            for k, x in r.items():
                w[f"adamw.{k}"] = max(w.get(f"adamw.{k}", 0.0), x)
    for shapes in (sb.FLOW_VEC_SHAPES[:3], sb.FLOW_SCALAR_SHAPES[:3]):
        for i, (B, chw) in enumerate(shapes):
            x, e = sb.noise_inputs(B, chw, seed=i)
            t = sb.sample_times(B)
            w["flow.z"] = max(w.get("flow.z", 0.0), worst(flow_f32(x, e, t, fma), sb.flow_ref(x, e, t)))
            for Tn in (8, 1000):
                sab, ab = tables(Tn)
                ti = sb.sample_steps(B, Tn)
                w["ddpm.xt"] = max(w.get("ddpm.xt", 0.0), worst(ddpm_f32(x, e, ti, sab, ab, fma), sb.ddpm_ref(x, e, ti, sab, ab)))
    for beta in sb.EMA_BETAS:
        ema, p = sb.noise_inputs(1, 4099, seed=7)
        w["ema"] = max(w.get("ema", 0.0), worst(ema_f32(ema[0], p[0], beta, fma), sb.ema_ref(ema[0], p[0], beta)))
    print("\nworst |diff| / bound, " + ("fused" if fma else "separate") + ": " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(w.items())))
    assert all(x <= 1.0 for x in w.values()), w
    assert all(x > 0.02 for x in w.values()), ("a bound fifty times above the f32 formula's own error checks nothing", w)


def test_integer_rounding_reference_agrees_with_torch_on_every_pattern():
    """the integer round-to-nearest-even of step_bounds against torch's CPU cast, on all 393 216 patterns (a check of the reference:
    the GPU test never uses a library cast)"""
    x = sb.f32_patterns()
    assert sb.cast_mismatch(x.bfloat16(), x) == 0
    want, nan = sb.f32_to_bf16_bits(x)
    assert int(nan.sum()) == 2 * (127 * 6 + 5)  # exponent all ones, mantissa non-zero: 127 high halves x 6 + 0x7F80 / 0xFF80 x 5 low halves
    assert bool(torch.equal(nan, torch.isnan(x)))
    for bits, expect in ((0x7F7FFFFF, 0x7F80), (0xFF7F8000, 0xFF80), (0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3FFF8000, 0x4000),
                         (0x00008000, 0x0000), (0x00018000, 0x0002), (0x80000001, 0x8000), (0x007FFFFF, 0x0080), (0x7F800000, 0x7F80)):
        assert int(sb.f32_to_bf16_bits(sb.from_bits32(torch.tensor([bits])))[0]) == expect, hex(bits)
    b = sb.bf16_patterns()
    assert bool(torch.equal(sb.bits32(b.float()), sb.bf16_to_f32_bits(b)))


# ------------------------------------------------------------------------------------------------------------------ rejects
def _truncate(x):
    return sb.from_bits16(sb.bits32(x) >> 16)


def _ties_away(x):
    return sb.from_bits16((sb.bits32(x) + 0x8000) >> 16)


@pytest.mark.parametrize("store", (_truncate, _ties_away), ids=("truncate", "ties-away"))
def test_a_wrong_bf16_store_is_rejected(store):
    """on the pattern table and on every weight shape of the GPU test (the data carries ties for this)"""
    x = sb.f32_patterns()
    x = x[~torch.isnan(x)]
    assert sb.cast_mismatch(store(x), x) > 0
    for (R, C) in sb.CAST_WEIGHT_SHAPES + tuple((2 * F, C) for F, C, _ in sb.SWIGLU_SHAPES) + tuple(e[:2] for e in sb.CAST_TABLE):
        w = sb.weight_input(R, C)
        assert sb.cast_mismatch(store(w), w) > 0 or R * C < 16, (R, C)  # (a single element cannot show both wrong stores)
        assert sb.cast_mismatch(w.bfloat16(), w) == 0


ADAMW_MUTANTS = (("wd_after", "visible"), ("eps_in_sqrt", "visible"), ("eps_scaled", "visible"), ("eps_scaled", "default-step1"),
                 ("bias_swapped", "visible"), ("bias_swapped", "default-step1000"), ("scale_m_only", "visible-gs0.5"),
                 ("scale_m_only", "visible-coef0.37-clip"))


@pytest.mark.parametrize("mutant,case", ADAMW_MUTANTS)
def test_a_wrong_adamw_is_rejected(mutant, case):
    S = dict(adamw_cases())[case]
    p, g, m, v = sb.adamw_inputs(N_HOST, seed=N_HOST)
    ref = sb.adamw_ref(p, g, m, v, S)
    for fma in (False, True):
        assert worst(adamw_f32(p, g, m, v, S, fma), ref) <= 1.0
        r = fb.judge(adamw_f32(p, g, m, v, S, fma, mutant), ref)
        print(f"{mutant} on {case}, {'fused' if fma else 'separate'}: " + ", ".join(f"{k} {x:.3g}" for k, x in r.items()))
        assert max(r.values()) > 1.0


def test_an_unwritten_tail_element_is_rejected():
    for n in (3, 7, N_HOST):  # tail only; one float4 and a tail; the body and a tail
        p, g, m, v = sb.adamw_inputs(n, seed=n)
        S = dict(adamw_cases())["default-step1"]
        ref = sb.adamw_ref(p, g, m, v, S)
        for k in ("p", "m", "v"):
            got = adamw_f32(p, g, m, v, S, True)
            got[k][n - 1] = eb.poison_(torch.empty(1))[0]  # what the poisoned allocation of the GPU test still holds there
            assert fb.judge(got, ref)[k] > 1.0
            got[k][n - 1] = (p, m, v)["pmv".index(k)][n - 1]  # ... or the old value, where the buffer is updated in place
            assert fb.judge(got, ref)[k] > 1.0


def test_a_neighbouring_samples_t_is_rejected():
    for (B, chw) in sb.FLOW_VEC_SHAPES[1:3]:  # (5, 4): the sample is one float4; (3, 1024)
        x, e = sb.noise_inputs(B, chw)
        t = sb.sample_times(B)
        ref = sb.flow_ref(x, e, t)
        assert worst(flow_f32(x, e, t, True), ref) <= 1.0
        assert worst(flow_f32(x, e, t, True, "neighbour_t"), ref) > 1.0


def test_tables_gathered_one_step_off_are_rejected():
    for Tn in (8, 1000):
        sab, ab = tables(Tn)
        for (B, chw) in sb.FLOW_SCALAR_SHAPES[:3]:
            x, e = sb.noise_inputs(B, chw)
            ti = sb.sample_steps(B, Tn)
            ref = sb.ddpm_ref(x, e, ti, sab, ab)
            assert worst(ddpm_f32(x, e, ti, sab, ab, False), ref) <= 1.0
            assert worst(ddpm_f32(x, e, ti, sab, ab, False, "t_off_by_one"), ref) > 1.0, (Tn, B, chw)


def test_ema_with_beta_for_one_minus_beta_is_rejected():
    for beta in sb.EMA_BETAS:
        for n in sb.EMA_N[:2]:
            ema, p = sb.noise_inputs(1, n, seed=n)
            ref = sb.ema_ref(ema[0], p[0], beta)
            assert worst(ema_f32(ema[0], p[0], beta, True), ref) <= 1.0
            assert worst(ema_f32(ema[0], p[0], beta, True, "beta"), ref) > 1.0, (beta, n)


def test_wrong_layouts_are_rejected():
    R, C, ld_t = 100, 72, 108
    w = sb.weight_input(R, C)
    want = sb.transposed_bits(w, ld_t)
    got = want.clone()
    got[32:64, 32:64] = sb.f32_to_bf16_bits(w)[0][32:64, 32:64]  # one 32 x 32 tile copied without the transposition
    assert not torch.equal(got, want)
    for (F, C, ld) in sb.SWIGLU_SHAPES[:2] + ((32, 8, 8),):
        w = sb.weight_input(2 * F, C)
        want = sb.swiglu_bits(w, ld)
        assert not torch.equal(torch.roll(want, 16, dims=0), want)  # the permutation shifted by one 16-row group
        assert F == 16 or not torch.equal(sb.plain_bits(w, ld), want)  # no permutation at all (F = 16: the identity)
    for (R, C) in sb.CAST_WEIGHT_SHAPES:
        w = sb.weight_input(R, C)
        want = sb.plain_bits(w, C + 8)
        assert bool((want[:, C:] == 0).all()) and bool(torch.equal(want[:, :C], sb.bits16(w.bfloat16())))
        got = want.clone()
        got[R - 1, C + 7] = eb.BF16_POISON  # a padding column left as it was
        assert not torch.equal(got, want)
    assert sb.swiglu_rows(32).tolist() == list(range(16)) + list(range(32, 48)) + list(range(16, 32)) + list(range(48, 64))


# ------------------------------------------------------------------------------------------------------------------ CastTable
def test_cast_table_refuses_a_swiglu_entry_with_rows_not_a_multiple_of_32():
    """F = R / 2 = 24: the kernel's row map ((rr >> 4) * 32 + 16 + (rr & 15)) would reach row 55 of the 48-row destination"""
    from diffulab_amd import ops

    src, dst = torch.zeros(48, 8), torch.zeros(48, 8, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="rows % 32"):
        ops.CastTable([(src, None, None, dst)])
    with pytest.raises(ValueError, match="entry 1"):
        ops.CastTable([(torch.zeros(64, 8), None, None, torch.zeros(64, 8, dtype=torch.bfloat16)), (src, dst, None, dst)])
    try:  # rows % 32 == 0 passes this check (and then needs device tensors, which is not a ValueError)
        ops.CastTable([(torch.zeros(64, 8), None, None, torch.zeros(64, 8, dtype=torch.bfloat16))])
    except ValueError as e:  # pragma: no cover
        raise AssertionError(f"a valid SwiGLU entry was refused: {e}")
    except RuntimeError:
        pass
