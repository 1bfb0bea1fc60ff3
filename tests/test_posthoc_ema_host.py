"""CPU checks of post-hoc EMA: the fp64 host math of diffulab_amd/training/posthoc_ema.py against the independent numpy restatement
(tests/posthoc_ema_common.py), the reconstruction of an untracked profile from snapshots, the argument validation of PowerEMA,
synthesize and BaseTrainer, and the declarations and refusals of the two C entry points (which validate before any device work)."""

from __future__ import annotations

import ctypes
import json
import re

import numpy as np
import pytest

import posthoc_ema_common as pc
from diffulab_amd import _lib, ops
from diffulab_amd.training import posthoc_ema as ph

SIGMAS = (0.03, 0.05, 0.075, 0.1, 0.15, 0.2, 0.25)


# ---------------------------------------------------------------------------------------------------------------- profiles
def test_sigma_rel_to_gamma_known_values_and_round_trip():
    assert round(ph.sigma_rel_to_gamma(0.05), 3) == 16.972
    assert round(ph.sigma_rel_to_gamma(0.10), 3) == 6.937
    for s in SIGMAS:
        g = ph.sigma_rel_to_gamma(s)
        assert abs(ph.gamma_to_sigma_rel(g) - s) <= 1e-12, (s, g)
        assert abs(g - pc.gamma_of(s)) <= 1e-9 * g, (s, g, pc.gamma_of(s))  # the cubic's root is the closed form's
        c = 1.0 / (s * s)
        assert abs(g ** 3 + 7 * g ** 2 + (16 - c) * g + (12 - c)) <= 1e-9 * c * g  # and a root of the stated polynomial
    for bad in (0.0, -0.1, 0.28, 0.3, float("nan")):
        with pytest.raises(ValueError, match="sigma_rel"):
            ph.sigma_rel_to_gamma(bad)


def test_ema_weight_keeps_its_precision_where_one_minus_beta_loses_it():
    """why dl_ema_update_multi takes the weight and not the decay: at t = 1e6 the weight ~ (gamma + 1) / t survives the rounding to
    f32, while 1.0f - f32(beta) is a multiple of 2^-24 ~ 6e-8 next to a value of ~1e-5"""
    for s in (0.05, 0.10):
        g = ph.sigma_rel_to_gamma(s)
        assert ph.ema_weight(1, g) == 1.0
        t = 10 ** 6
        new = ph.ema_weight(t, g) * t / (g + 1.0)
        beta32 = np.float32((1.0 - 1.0 / t) ** (g + 1.0))
        old = float(np.float32(1.0) - beta32) * t / (g + 1.0)
        print(f"sigma_rel {s}: w t / (gamma + 1) = {new:.8f} (weight passed), {old:.8f} (1.0f - f32(beta))")
        assert abs(new - 1.0) <= 1e-5, (s, new)
        assert abs(old - 1.0) > 1e-5, (s, old)
        assert ph.ema_weight(t, g) == pc.weight32(t, g)
        assert np.float32(ph.ema_weight(t, g)) == ph.ema_weight(t, g)  # already an f32 value
    with pytest.raises(ValueError, match="t counts"):
        ph.ema_weight(0, 5.0)


@pytest.mark.parametrize("ta,tb", [(700.0, 1000.0), (1000.0, 700.0), (1000.0, 1000.0)])
def test_correlation_closed_form_matches_quadrature(ta, tb):
    for sa, sb in ((0.05, 0.10), (0.10, 0.05), (0.075, 0.075), (0.2, 0.03)):
        ga, gb = ph.sigma_rel_to_gamma(sa), ph.sigma_rel_to_gamma(sb)
        got, want = ph.power_function_correlation(ta, ga, tb, gb), pc.correlation_quadrature(ta, ga, tb, gb)
        assert abs(got - want) <= 1e-6 * abs(want), (ta, tb, sa, sb, got, want)
        assert got == ph.power_function_correlation(tb, gb, ta, ga)  # symmetric
        assert abs(got - pc.correlation(ta, ga, tb, gb)) <= 1e-14 * abs(got)


def test_coefficients_are_one_hot_when_the_target_is_a_stored_snapshot():
    in_t = [t for t in range(64, 513, 64) for _ in (0, 1)]
    in_s = [0.05, 0.10] * 8
    for pick in (0, 7, 15):
        w = ph.solve_posthoc_coefficients(in_t, in_s, in_t[pick], in_s[pick])
        want = np.zeros(16)
        want[pick] = 1.0
        print(f"target = snapshot {pick}: sum |w| - 1 = {np.abs(w).sum() - 1.0:.2e}")
        assert np.abs(w - want).max() <= 1e-9, (pick, w)
    many = ph.solve_posthoc_coefficients(in_t, in_s, [512, 512], [0.075, 0.05])
    assert many.shape == (16, 2)
    # (one solve with two right-hand sides against one with a single one: the same system, not the same order of operations)
    assert np.abs(many[:, 0] - ph.solve_posthoc_coefficients(in_t, in_s, 512, 0.075)).max() <= 1e-9


def test_reconstruction_of_an_untracked_profile_from_snapshots():
    """0.075 at t = 2048 from 32 snapshot times of the profiles 0.05 and 0.10, against the same profile tracked directly.  Measured
    where this test was written: synthesised 8.1e-5, nearer tracked profile 0.254 (both relative to |direct EMA - theta[-1]|),
    condition number of A 9.5e4.  The assertion asks for a factor 100 of the measured ~3100: the slack covers other BLAS builds."""
    c = pc.reconstruction_case()
    w = ph.solve_posthoc_coefficients(c["in_t"], c["in_sigma"], 2048, 0.075)
    w_ref, A = pc.coefficients(c["in_t"], c["in_sigma"], 2048, 0.075)
    synth = w @ c["snaps"]
    scale = np.linalg.norm(c["direct"] - c["theta"][-1])
    e_synth = np.linalg.norm(synth - c["direct"]) / scale
    e_near = min(np.linalg.norm(tr - c["direct"]) for tr in c["tracked"]) / scale
    print(f"synthesised vs direct {e_synth:.3e}, nearer tracked profile vs direct {e_near:.3e}, ratio {e_near / e_synth:.0f}, "
          f"cond(A) {np.linalg.cond(A):.2e}, sum |w| {np.abs(w).sum():.3f}")
    assert e_synth * 100.0 <= e_near, (e_synth, e_near)
    assert np.linalg.norm((w - w_ref) @ c["snaps"]) / scale <= 1e-6  # both solvers synthesise the same point
    for s in (0.03, 0.2):  # outside the tracked range the combination is ill-conditioned: the weights the GPU test imitates
        wo = ph.solve_posthoc_coefficients(c["in_t"], c["in_sigma"], 2048, s)
        print(f"target sigma_rel {s}: sum |w| = {np.abs(wo).sum():.2f}")


# ---------------------------------------------------------------------------------------------------------------- arguments
KW = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=2, patch_size=2, depth=1,
          n_classes=4, classifier_free=True)


def _model():
    from diffulab_amd import MMDiT

    return MMDiT(simple_dit=True, **KW)


def test_power_ema_names_the_argument_it_refuses():
    from diffulab_amd.training import PowerEMA

    m = _model()
    for kw, name in ((dict(sigma_rels=(0.03, 0.05, 0.1, 0.15, 0.2)), "sigma_rels"), (dict(sigma_rels=()), "sigma_rels"),
                     (dict(sigma_rels=(0.05, 0.05)), "sigma_rels"), (dict(sigma_rels=(0.05, 0.28)), "sigma_rels"),
                     (dict(sigma_rels=(0.0, 0.1)), "sigma_rels"), (dict(eval_sigma_rel=0.075), "eval_sigma_rel"),
                     (dict(update_every=0), "update_every")):
        with pytest.raises(ValueError, match=name):
            PowerEMA(m, **kw)
    e = PowerEMA(m, sigma_rels=(0.05, 0.10, 0.2), eval_sigma_rel=0.10)
    assert len(e.ema_models) == 3 and e.ema_model is e.ema_models[1] and e.t == 0 and e.calls == 0
    assert all(not q.requires_grad for q in e.ema_models.parameters())
    assert PowerEMA(m).ema_model is not m
    sd = e.state_dict()
    assert sd["t"] == 0 and sd["calls"] == 0 and sd["sigma_rels"] == [0.05, 0.10, 0.2] and len(sd["profiles"]) == 3
    assert set(sd["profiles"][0]) == set(m.state_dict())
    with pytest.raises(ValueError, match="sigma_rels"):
        PowerEMA(m, sigma_rels=(0.05, 0.15)).load_state_dict(sd)
    with pytest.raises(ValueError, match="snapshot"):
        e.snapshot("unused")


def test_synthesize_refuses_an_empty_index_and_a_time_after_the_last_snapshot(tmp_path):
    m = _model()
    with pytest.raises(ValueError, match="snapshot_dir"):
        ph.synthesize(m, tmp_path, 0.075)  # no index at all
    (tmp_path / ph.INDEX_NAME).write_text("")
    with pytest.raises(ValueError, match="snapshot_dir.*empty"):
        ph.synthesize(m, tmp_path, 0.075)
    rows = [{"t": t, "sigma_rel": s, "file": ph.snapshot_name(t, s)} for t in (8, 16) for s in (0.05, 0.1)]
    (tmp_path / ph.INDEX_NAME).write_text("".join(json.dumps(r) + "\n" for r in rows))
    with pytest.raises(ValueError, match="t = 17 is later than the last snapshot"):
        ph.synthesize(m, tmp_path, 0.075, t=17)
    with pytest.raises(ValueError, match="sigma_rel"):
        ph.synthesize(m, tmp_path, 0.5)
    with pytest.raises(ValueError, match="group"):
        ph.synthesize(m, tmp_path, 0.075, group=0)
    used, t = ph.select_snapshots(ph.read_index(tmp_path), 8)
    assert t == 8 and [r["file"] for r in used] == ["phema_000000008_0.050.pt", "phema_000000008_0.100.pt"]


def test_base_trainer_names_the_argument_it_refuses(tmp_path):
    from diffulab_amd.training import BaseTrainer

    base = dict(n_epoch=1, save_path=tmp_path, project_name="p", use_ema=True)
    for kw, name in ((dict(ema_type="karras"), "ema_type"), (dict(ema_type="power", ema_update_after_step=10), "ema_update_after_step"),
                     (dict(ema_type="power", ema_sigma_rels=(0.05, 0.05)), "sigma_rels"),
                     (dict(ema_type="power", ema_sigma_rels=(0.05, 0.4)), "sigma_rels"),
                     (dict(ema_type="power", ema_eval_sigma_rel=0.2), "eval_sigma_rel"),
                     (dict(ema_type="power", ema_snapshot_every=-1), "ema_snapshot_every")):
        with pytest.raises(ValueError, match=name):
            BaseTrainer(**base, **kw)
    t = BaseTrainer(**base, ema_type="power", ema_update_every=2, gradient_accumulation_step=3, ema_snapshot_every=5)
    assert (t.ema_type, t.ema_update_every, t.ema_snapshot_every, t.ema_sigma_rels) == ("power", 6, 5, (0.05, 0.10))
    d = BaseTrainer(**base, ema_update_after_step=10)  # the default keeps the classic EMA and its warm-up
    assert d.ema_type == "classic" and d.ema_update_after_step == 10


# ---------------------------------------------------------------------------------------------------------------- C ABI
def test_entry_points_are_declared_and_resolve():
    protos = _lib.parse_header()
    assert protos["dl_ema_update_multi"][2] == ["ema0", "ema1", "ema2", "ema3", "p", "K", "w0", "w1", "w2", "w3", "n", "stream"]
    assert protos["dl_arena_lincomb"][2] == ["out", "srcs_host", "srcs_dev", "w_host", "w_dev", "K", "n", "flags", "stream"]
    L = _lib.lib()
    for name in ("dl_ema_update_multi", "dl_arena_lincomb"):
        assert name in L._fns and getattr(L.cdll, name)
    text = open(_lib.HEADER_PATH).read()
    m = re.search(r"enum \{ DL_LINCOMB_ACCUMULATE = (\d+) \}", text)
    assert m and int(m.group(1)) == ops.LINCOMB_ACCUMULATE
    assert callable(ops.ema_update_multi) and callable(ops.arena_lincomb)


def test_entry_points_refuse_out_of_contract_arguments_before_any_launch():
    """validation happens before any device work: the dummy non-null pointers are never dereferenced"""
    raw = ctypes.create_string_buffer(1024)
    base = (ctypes.addressof(raw) + 63) & ~63
    P = [ctypes.c_void_p(base + 64 * i) for i in range(6)]
    L = _lib.lib()
    f, i64, ci = ctypes.c_float, ctypes.c_int64, ctypes.c_int

    def upd(e=(P[0], P[1], P[2], P[3]), p=P[4], K=2, w=(0.5, 0.5, 0.5, 0.5), n=8):
        rc = L.cdll.dl_ema_update_multi(*e, p, ci(K), *(f(x) for x in w), i64(n), None)
        return rc, L.cdll.dl_last_error().decode()

    inf, nan = float("inf"), float("nan")
    for kw in (dict(K=0), dict(K=5), dict(K=-1), dict(e=(None, P[1], P[2], P[3])), dict(e=(P[0], None, P[2], P[3])), dict(p=None),
               dict(n=0), dict(n=-8), dict(w=(inf, 0.5, 0.5, 0.5)), dict(w=(0.5, nan, 0.5, 0.5)), dict(e=(P[0], P[0], P[2], P[3])),
               dict(K=4, e=(P[0], P[1], P[2], P[1])), dict(K=3, e=(P[0], P[1], None, P[3])), dict(e=(P[0], P[4], P[2], P[3]))):
        rc, msg = upd(**kw)
        assert rc == -1 and "dl_ema_update_multi" in msg, (kw, rc, msg)

    srcs = (ctypes.c_int64 * 4)(base + 64, base + 128, base + 192, base + 256)
    wts = (ctypes.c_float * 4)(1.0, -1.0, 0.5, 0.5)

    def lin(out=P[0], sh=srcs, sd=P[5], wh=wts, wd=P[5], K=4, n=8, flags=0):
        rc = L.cdll.dl_arena_lincomb(out, sh, sd, wh, wd, ci(K), i64(n), ci(flags), None)
        return rc, L.cdll.dl_last_error().decode()

    null_in = (ctypes.c_int64 * 4)(base + 64, 0, base + 192, base + 256)
    odd_in = (ctypes.c_int64 * 4)(base + 64, base + 128 + 4, base + 192, base + 256)
    out_in = (ctypes.c_int64 * 4)(base + 64, base + 128, base, base + 256)
    for kw in (dict(K=0), dict(K=257), dict(out=None), dict(sh=None), dict(sd=None), dict(wh=None), dict(wd=None), dict(n=0), dict(n=-1),
               dict(flags=2), dict(flags=-1), dict(sh=null_in), dict(sh=odd_in), dict(sh=out_in), dict(out=ctypes.c_void_p(base + 4))):
        rc, msg = lin(**kw)
        assert rc == -1 and "dl_arena_lincomb" in msg, (kw, rc, msg)
    del raw
