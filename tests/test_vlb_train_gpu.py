"""GPU tests of L_vlb training with loss-aware timestep sampling (Nichol & Dhariwal 2021, sec. 3.3): the row head
(dl_gd_loss_rows_fwd / _bwd), the resampler's state (dl_loss_history_update, dl_draw_timesteps), and `GaussianDiffusion.compute_loss` /
`draw_timesteps` / the trainer over them.

Expected values: the f64 evaluation of tests/vlb_train_common.py on the same f32 inputs, and its numpy resampler.

Tolerance, the suite's rule for f32 element-wise kernels (`bpd_common.bound`, tests/test_learned_variance_gpu.py): the kernel and the f32
CPU evaluation of the restatement are both f32 evaluations of the same formulas on the same inputs, so the f32 CPU evaluation's own
error against f64 is measured per case and, per output array, every element is allowed 2 * max|f32 CPU - f64| + 3e-6 * max|f64|.
Every figure is printed before it is asserted.  The resampler's history and counts, and the draws, are compared exactly.

Inputs: the builders of tests/bpd_common.py, B = 5 with t = (0, 0, 1, T-2, T-1) on the 8-step and 20-step respaced chains and the
1000-step one (every forward, backward, footprint and bit-for-bit check runs on all three); chw = 192 (under one wave's share of a block), 960 (no multiple of 256), 4096 and 4097 (the boundary of a 4096-element
share), 12288 (three shares).
"""

import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bpd_common as bp  # noqa: E402
import elementwise_bounds as eb  # noqa: E402
import gd_param_common as gp  # noqa: E402
import vlb_train_common as vt  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
CHWS = (192, 960, 4096, 4097, 12288)
CHAINS = ("t8", "r20", "full")  # 8 and 20 steps (respaced), 1000 steps
VAR_TYPES = gp.VAR_TYPES  # fixed, learned, learned_range
VB_SCALE = 0.37


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as _ops

    return _ops


def var_mode(ops, var_type: str) -> int:
    return ops.VAR_MODES.get(var_type, ops.VAR_FIXED)


@lru_cache(maxsize=None)
def inputs(chain: str, chw: int, name: str, var_type: str):
    T, t = vt.chain(chain)
    c = bp.case(T, t, chw, name, vt.VAR_TABLE[var_type], tag=chain)
    n = c["tab"].shape[1]
    c["weight"] = None if name == "xprev" else gp.min_snr(T.alphas_bar, name).float()
    c["imp"] = vt.imp_table(n)
    return c


def pick(c, weighted: bool, importance: bool):
    """(weight, imp) of one case; xprev has no min-SNR weight: a table built like the importance one stands in"""
    w = None
    if weighted:
        w = c["weight"] if c["weight"] is not None else vt.imp_table(c["tab"].shape[1]).flip(0).contiguous()
    return w, (c["imp"] if importance else None)


@lru_cache(maxsize=None)
def reference(chain: str, chw: int, name: str, var_type: str, weighted: bool, importance: bool, loss_type: str):
    """(inputs, f64 outputs, f32 CPU outputs) of one forward case: computed once, shared, never modified"""
    c = inputs(chain, chw, name, var_type)
    w, im = pick(c, weighted, importance)
    args = (c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], name, var_type, w, im, loss_type, VB_SCALE)
    with torch.no_grad():
        return c, vt.rows(*args, torch.float64), vt.rows(*args, torch.float32)


def dev(c, w, im):
    d = {k: c[k].to(DEV) for k in ("pred", "eps", "x0", "xt", "t", "tab")}
    d["weight"], d["imp"] = (None if w is None else w.to(DEV)), (None if im is None else im.to(DEV))
    return d


def run_fwd(ops, d, name, var_type, loss_type, out=None):
    return ops.gd_loss_rows_fwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], ops.MEAN_TYPES[name], d["weight"], d["imp"],
                                var_mode(ops, var_type), ops.LOSS_TYPES[loss_type], VB_SCALE, out=out)


def run_bwd(ops, d, name, var_type, loss_type, g_mse, g_vb, out=None):
    return ops.gd_loss_rows_bwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], ops.MEAN_TYPES[name], d["weight"], d["imp"],
                                var_mode(ops, var_type), ops.LOSS_TYPES[loss_type], g_mse, g_vb, out=out)


def check(what: str, got, ref, cpu32):
    err, e32, bound = bp.bound(got, ref, cpu32)
    print(f"{what}: max|ref| {float(ref.abs().max()):.6g}  f32-cpu max err {e32:.3e}  kernel max err {err:.3e}  bound {bound:.3e}")
    assert bool(torch.isfinite(got).all()) and err <= bound, (what, err, bound)


def check_fwd(what, got, ref, cpu32, fixed):
    mse_row, vb_row, total_row, loss = got
    check(f"{what} mse_row", mse_row, ref["mse_row"], cpu32["mse_row"])
    check(f"{what} total_row", total_row, ref["total_row"], cpu32["total_row"])
    if fixed:
        assert vb_row is None
        check(f"{what} loss[0]", loss[:1], ref["loss"], cpu32["loss"])
    else:
        check(f"{what} vb_row", vb_row, ref["vb_row"], cpu32["vb_row"])
        check(f"{what} loss", loss, ref["loss"], cpu32["loss"])


def modes(var_type):
    """(weighted, importance, loss_type) of every mode of one (target, var_type)"""
    return [(w, im, lt) for w in (False, True) for im in (False, True) for lt in (("mse",) if var_type == "fixed" else vt.LOSS_TYPES)]


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("var_type", VAR_TYPES)
@pytest.mark.parametrize("name", gp.TARGETS)
def test_rows_fwd_against_f64(ops, name, var_type, chain):
    T = vt.CHAINS[chain]
    for chw in CHWS:
        for weighted, importance, loss_type in modes(var_type):
            c, ref, cpu32 = reference(chain, chw, name, var_type, weighted, importance, loss_type)
            assert c["tab"].shape == (6, T) and c["t"].tolist() == [0, 0, 1, T - 2, T - 1]
            vt.check_inputs(c, ref)
            got = run_fwd(ops, dev(c, *pick(c, weighted, importance)), name, var_type, loss_type)
            assert all(g is None or (g.dtype == torch.float32 and g.shape == (bp.ROWS,)) for g in got[:3]) and got[3].shape == (2,)
            check_fwd(f"{chain} {name}/{var_type} chw {chw} w{int(weighted)} imp{int(importance)} {loss_type}", got, ref, cpu32,
                      var_type == "fixed")


@pytest.mark.parametrize("var_type", VAR_TYPES)
@pytest.mark.parametrize("name", gp.TARGETS)
@pytest.mark.parametrize("chain", CHAINS)
def test_rows_average_to_the_batch_head_scalars(ops, name, var_type, chain):
    """imp NULL: the mean over the rows of mse_row (times the weight) / vb_row is what dl_gd_loss_fwd reduces over the whole batch"""
    for chw in CHWS:
        for weighted in (False, True):
            c, ref, cpu32 = reference(chain, chw, name, var_type, weighted, False, "mse")
            w, _ = pick(c, weighted, False)
            d = dev(c, w, None)
            mse_row, vb_row, _, loss = run_fwd(ops, d, name, var_type, "mse")
            both = ops.gd_loss_fwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], ops.MEAN_TYPES[name], d["weight"],
                                   var_mode(ops, var_type)).reshape(-1)
            wt = vt.per_timestep(w, c["t"], torch.float64)
            pairs = [("mse", (wt * mse_row.double().cpu()).mean(), 0)] + ([] if var_type == "fixed" else [("vb", vb_row.double().cpu().mean(), 1)])
            for key, mean, k in pairs:
                _, e32, bound = bp.bound(loss[k:k + 1], ref["loss"][k:k + 1], cpu32["loss"][k:k + 1])
                diff, diff2 = abs(float(mean) - float(both[k])), abs(float(loss[k]) - float(both[k]))
                print(f"{chain} {name}/{var_type} chw {chw} w{int(weighted)} {key}: mean of rows {float(mean):.9g}  dl_gd_loss_fwd {float(both[k]):.9g}  "
                      f"|diff| {diff:.3e}  |loss[{k}] - it| {diff2:.3e}  bound {bound:.3e}")
                assert diff <= bound and diff2 <= bound


# ------------------------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("var_type", VAR_TYPES)
@pytest.mark.parametrize("name", gp.TARGETS)
def test_rows_bwd_against_f64_per_element(ops, name, var_type, chain):
    g_mse, g_vb = 0.7, 1.3
    for chw in CHWS:
        for weighted, importance, loss_type in modes(var_type):
            c = inputs(chain, chw, name, var_type)
            w, im = pick(c, weighted, importance)
            args = (c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], c["t"], name, var_type, w, im, loss_type, g_mse, g_vb)
            ref, cpu32 = vt.rows_backward(*args, torch.float64), vt.rows_backward(*args, torch.float32)
            d = dev(c, w, im)
            got = run_bwd(ops, d, name, var_type, loss_type, torch.tensor(g_mse, device=DEV), torch.tensor(g_vb, device=DEV))
            assert got.shape == c["pred"].shape and got.dtype == torch.float32
            what = f"{chain} {name}/{var_type} chw {chw} w{int(weighted)} imp{int(importance)} {loss_type}"
            halves = [("mean half", slice(0, chw))] + ([] if var_type == "fixed" else [("variance half", slice(chw, 2 * chw))])
            for half, cols in halves:  # each half against its own magnitude
                check(f"{what} dpred {half}", got[:, cols], ref[:, cols], cpu32[:, cols])
            if var_type != "fixed":
                stop = vt.rows_backward(*args[:10], "mse", g_mse, g_vb, torch.float64)[:, :chw]
                from_bound = (got[:, :chw].double().cpu() - stop).abs()
                if loss_type == "vlb":  # no stop-gradient: the bound reaches the mean output of every sample
                    assert bool((from_bound.flatten(1).max(1).values > 0).all()) and float((ref[:, :chw] - stop).abs().max()) > 0
            if loss_type == "mse" and not importance:
                # the same coefficients formed in the same order, the same element-wise arithmetic: dl_gd_loss_bwd's bits
                old = ops.gd_loss_bwd(d["pred"], d["eps"], d["x0"], d["xt"], d["t"], d["tab"], ops.MEAN_TYPES[name], d["weight"],
                                      var_mode(ops, var_type), torch.tensor(g_mse, device=DEV), torch.tensor(g_vb, device=DEV))
                assert torch.equal(got.view(torch.int32), old.view(torch.int32)), what


def test_null_upstream_gradients_are_ones(ops):
    c = inputs("t8", 960, "v", "learned_range")
    d = dev(c, None, c["imp"])
    one = torch.ones((), device=DEV)
    a = run_bwd(ops, d, "v", "learned_range", "vlb", None, None)
    b = run_bwd(ops, d, "v", "learned_range", "vlb", one, one)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ footprint, bits
@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("var_type", ["fixed", "learned_range"])
def test_outputs_stay_inside_their_windows_and_two_runs_agree(ops, var_type, chain):
    fixed = var_type == "fixed"
    for chw in (192, 4097, 12288):
        for loss_type in (("mse",) if fixed else vt.LOSS_TYPES):
            c = inputs(chain, chw, "v", var_type)
            d = dev(c, c["weight"], c["imp"])
            first = run_fwd(ops, d, "v", var_type, loss_type)
            rows = [eb.Guarded(1, bp.ROWS, torch.float32, DEV) for _ in range(3)]
            loss = eb.Guarded(1, 1 if fixed else 2, torch.float32, DEV)
            out = (rows[0].win[0], None if fixed else rows[1].win[0], rows[2].win[0], loss.win[0])
            run_fwd(ops, d, "v", var_type, loss_type, out=out)
            for g, a, k in zip(rows + [loss], first, ("mse_row", "vb_row", "total_row", "loss")):
                if a is None:
                    assert bool(eb.is_poison(g.buf).all())
                    continue
                g.check(f"dl_gd_loss_rows_fwd {chain} {var_type} {loss_type} chw {chw}: {k}")
                m = g.win.shape[1]
                assert int((~eb.is_poison(g.buf)).sum()) == m
                assert torch.equal(g.win[0].view(torch.int32), a.reshape(-1)[:m].view(torch.int32)), (chw, k)
            n = c["pred"].numel()
            gd = eb.Guarded(1, n, torch.float32, DEV)
            one = torch.ones((), device=DEV)
            a = run_bwd(ops, d, "v", var_type, loss_type, one, one)
            run_bwd(ops, d, "v", var_type, loss_type, one, one, out=gd.win[0].view(c["pred"].shape))
            gd.check(f"dl_gd_loss_rows_bwd {chain} {var_type} {loss_type} chw {chw}")
            assert int((~eb.is_poison(gd.buf)).sum()) == n and torch.equal(gd.win[0].view(torch.int32), a.view(-1).view(torch.int32))


# ------------------------------------------------------------------------------------------------------------------ history
def history_batches(T: int, H: int):
    """three steps of a run: a batch with duplicate indices that leaves some indices out; one that brings every count to H (each index
    as often as it still lacks, plus two more of index 1, which shift); one more with duplicates after the warm-up"""
    g = np.random.default_rng(T * 100 + H)
    t1 = np.concatenate([g.integers(0, max(2, T // 2), size=min(3 * T, 300)), [1, 1]]).astype(np.int32)  # the upper half stays empty
    count = np.minimum(np.bincount(t1, minlength=T), H)
    t2 = np.concatenate([np.repeat(np.arange(T), H - count), [1, 1]]).astype(np.int32)
    g.shuffle(t2)
    t3 = np.concatenate([g.integers(0, T, size=37), [T - 1, T - 1, 0, T - 1]]).astype(np.int32)
    return [(t, (0.05 + 3.0 * g.random(t.size) * (1.0 + t / T)).astype(np.float32)) for t in (t1, t2, t3)]


def fresh_state(T: int, H: int):
    return {"hist": torch.zeros(T, H, device=DEV), "count": torch.zeros(T, dtype=torch.int32, device=DEV),
            **{k: eb.Guarded(1, T, torch.float32, DEV) for k in ("p", "imp", "cdf")}}


def step_state(ops, s, t, loss, up):
    ops.loss_history_update(None if t is None else torch.from_numpy(t).to(DEV), None if loss is None else torch.from_numpy(loss).to(DEV),
                            s["hist"], s["count"], s["p"].win[0], s["imp"].win[0], s["cdf"].win[0], up)


@pytest.mark.parametrize("T,H", [(8, 3), (8, 10), (1000, 3)])
def test_history_update_against_the_numpy_resampler(ops, T, H):
    up = 0.001
    runs = []
    for _ in range(2):
        s, r = fresh_state(T, H), vt.Resampler(T, H, up)
        snaps = []
        for k, (t, loss) in enumerate(history_batches(T, H)):
            step_state(ops, s, t, loss, up)
            r.update(t, loss)
            assert r.warmed_up() == (k >= 1)  # the second batch completes the warm-up, not the first
            assert np.array_equal(s["hist"].cpu().numpy(), r.hist) and np.array_equal(s["count"].cpu().numpy(), r.count), (T, H, k)
            for key, ref, c32 in zip(("p", "imp", "cdf"), r.tables(np.float64), r.tables(np.float32)):
                s[key].check(f"dl_loss_history_update T {T} H {H}: {key}")
                check(f"T {T} H {H} step {k} {key}", s[key].win[0], torch.from_numpy(ref), torch.from_numpy(c32))
            cdf = s["cdf"].win[0].cpu().numpy()
            assert bool((np.diff(cdf) >= 0).all()) and cdf[-1] == 1.0 and cdf[0] > 0
            if k == 0:
                assert np.array_equal(s["p"].win[0].cpu().numpy(), np.full(T, np.float32(1.0) / np.float32(T)))
            snaps.append([s[key].win[0].clone() for key in ("p", "imp", "cdf")] + [s["hist"].clone(), s["count"].clone()])
        step_state(ops, s, None, None, up)  # no pairs: the same history gives the same tables
        assert all(torch.equal(s[key].win[0].view(torch.int32), a.view(torch.int32)) for key, a in zip(("p", "imp", "cdf"), snaps[-1]))
        runs.append(snaps)
    for a, b in zip(runs[0], runs[1]):  # two runs: identical bits
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("T,H", [(8, 3), (1000, 3)])
def test_draw_is_searchsorted_on_the_tables_read_back(ops, T, H):
    s = fresh_state(T, H)
    cdfs = [np.cumsum(np.full(T, 1.0 / T)).astype(np.float32)]  # before any update the state's table is uniform
    cdfs[0][-1] = 1.0
    for t, loss in history_batches(T, H)[:2]:
        step_state(ops, s, t, loss, 0.001)
    cdfs.append(s["cdf"].win[0].cpu().numpy())
    for cdf in cdfs:
        u = np.concatenate([[0.0], cdf, np.nextafter(cdf, np.float32(0)), np.nextafter(cdf, np.float32(2)),
                            [np.nextafter(np.float32(1), np.float32(0))]]).astype(np.float32)
        u = u[u < 1.0]
        out = eb.Guarded(1, u.size, torch.int32, DEV)
        ops.draw_timesteps(torch.from_numpy(u).to(DEV), torch.from_numpy(cdf).to(DEV), out=out.win[0])
        got = out.win[0].cpu().numpy()
        assert int((~eb.is_poison(out.buf)).sum()) == u.size and bool((eb.is_poison(out.buf) | ~out.mask).all())
        want = vt.draw(cdf, u)
        assert np.array_equal(got, want) and got.min() == 0 and got.max() == T - 1
        assert set(got.tolist()) == set(range(T))  # every index is reachable


# ------------------------------------------------------------------------------------------------------------------ argument errors
def test_out_of_contract_calls_return_a_status_and_launch_nothing(ops):
    from diffulab_amd import _lib

    cd = _lib.lib().cdll
    c = inputs("t8", 192, "epsilon", "learned_range")
    d = dev(c, None, None)
    P = {k: ctypes.c_void_p(v.data_ptr()) for k, v in d.items() if v is not None}
    outs = [eb.poison_(torch.empty(2 * 5 * 192, device=DEV)) for _ in range(5)]
    O = [ctypes.c_void_p(o.data_ptr()) for o in outs]
    i64, F = ctypes.c_int64, ctypes.c_float

    def fwd(rc_want=-1, B=5, chw=192, T=8, target=0, vm=1, lt=0, null=(), outs_null=()):
        a = {k: (None if k in null else v) for k, v in P.items()}
        o = [None if i in outs_null else p for i, p in enumerate(O)]
        rc = cd.dl_gd_loss_rows_fwd(a["pred"], a["eps"], a["x0"], a["xt"], a["t"], a["tab"], T, target, None, None, vm, lt, F(1.0), None,
                                    o[0], o[1], o[2], o[3], i64(B), i64(chw), None)
        assert rc == rc_want and "dl_gd_loss_rows_fwd" in cd.dl_last_error().decode(), (rc, cd.dl_last_error().decode())

    def bwd(B=5, chw=192, T=8, target=0, vm=1, lt=0, null=(), dp=True):
        a = {k: (None if k in null else v) for k, v in P.items()}
        rc = cd.dl_gd_loss_rows_bwd(a["pred"], a["eps"], a["x0"], a["xt"], a["t"], a["tab"], T, target, None, None, vm, lt, None, None,
                                    O[4] if dp else None, i64(B), i64(chw), None)
        assert rc == -1 and "dl_gd_loss_rows_bwd" in cd.dl_last_error().decode(), (rc, cd.dl_last_error().decode())

    for k in P:
        fwd(null=(k,))
        bwd(null=(k,))
    for i in range(4):
        fwd(outs_null=(i,))
    bwd(dp=False)
    for kw in ({"B": 0}, {"chw": 0}, {"T": 0}, {"target": 4}, {"vm": 2}, {"lt": 2}, {"lt": 1, "vm": -1}):
        fwd(**kw)
        bwd(**kw)
    fwd(chw=4097)  # two shares per row and no scratch
    hist, count = torch.zeros(8, 3, device=DEV), torch.zeros(8, dtype=torch.int32, device=DEV)
    H = [ctypes.c_void_p(x.data_ptr()) for x in (hist, count)]

    def upd(rc_want, n=5, T=8, Hh=3, up=0.001, null=()):
        a = [None if i in null else p for i, p in enumerate([P["t"], O[0], H[0], H[1], O[1], O[2], O[3]])]
        rc = cd.dl_loss_history_update(a[0], a[1], i64(n), a[2], a[3], a[4], a[5], a[6], T, Hh, F(up), None)
        assert rc == rc_want and "dl_loss_history_update" in cd.dl_last_error().decode(), (rc, cd.dl_last_error().decode())

    upd(-3, T=4097)  # DL_ERR_UNSUPPORTED: the distribution no longer fits one workgroup's shared memory
    upd(-3, n=65537)
    for i in range(7):
        upd(-1, null=(i,))
    for kw in ({"T": 0}, {"Hh": 0}, {"n": -1}, {"up": -0.5}, {"up": 1.5}):
        upd(-1, **kw)
    for args in ((None, O[1], 8, O[2], i64(5)), (O[0], None, 8, O[2], i64(5)), (O[0], O[1], 8, None, i64(5)), (O[0], O[1], 0, O[2], i64(5)),
                 (O[0], O[1], 8, O[2], i64(0))):
        assert cd.dl_draw_timesteps(*args, None) == -1 and "dl_draw_timesteps" in cd.dl_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool(eb.is_poison(o).all()) for o in outs) and float(hist.abs().sum()) == 0 and int(count.sum()) == 0


# ------------------------------------------------------------------------------------------------------------------ end to end
def _unet(out_channels):
    from diffulab_amd.networks.denoisers import UNetModel

    return UNetModel(image_size=[16, 16], in_channels=1, model_channels=32, out_channels=out_channels, num_res_blocks=1,
                     attention_resolutions=[2], channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True,
                     n_classes=10, classifier_free=True)


def _dit(output_channels):
    from diffulab_amd import MMDiT

    return MMDiT(simple_dit=True, input_channels=4, output_channels=output_channels, inner_dim=128, embedding_dim=64, num_heads=2,
                 mlp_ratio=4, patch_size=2, depth=2, n_classes=10, classifier_free=True)


FAMILIES = {"unet": (_unet, 1, "out.2.weight"), "dit": (_dit, 4, "last_layer.linear.weight")}


def diffuser(family: str, steps: int = 8, **extra):
    from diffulab_amd import Diffuser

    torch.manual_seed(0)
    make, C, head = FAMILIES[family]
    m = make(2 * C)
    with torch.no_grad():  # the output heads start at zero
        dict(m.named_parameters())[head].normal_(std=0.02)
    m = m.to(DEV)
    sp = extra.pop("sampler_parameters", {"var_type": "learned_range"})
    d = Diffuser(m, model_type="gaussian_diffusion", sampling_method="ddpm", n_steps=1000, extra_args={"sampler_parameters": sp, **extra})
    if steps != 1000:
        d.set_steps(steps)
    return d, m, C, head


class Stub(torch.nn.Module):
    """a denoiser that is one learnable tensor: nothing but the diffusion's own calls reaches `ops`"""

    def __init__(self, shape):
        super().__init__()
        self.w = torch.nn.Parameter(0.1 * synth.normal("vlbt.stub", shape))

    def forward(self, x, timesteps, **kw):
        return {"x": self.w + 0.0 * x.mean()}


@pytest.mark.parametrize("kw,fwd,bwd", [
    ({}, "dl_mse_loss_fwd", "dl_mse_loss_bwd"),
    ({"sampler_parameters": {"var_type": "learned_range"}}, "dl_vlb_loss_fwd", "dl_vlb_loss_bwd"),
    ({"sampler_parameters": {"mean_type": "v"}, "loss_target": "mean_type", "loss_weighting": "min_snr"}, "dl_gd_loss_fwd", "dl_gd_loss_bwd"),
])
def test_defaults_make_the_calls_of_the_batch_scalar_heads(ops, monkeypatch, kw, fwd, bwd):
    """timestep_sampler="uniform", loss_type="mse": draw_timesteps is the one torch.randint call, compute_loss + backward reach the
    library through the same entry points, in the same order, as before the row head existed"""
    from diffulab_amd import Diffuser

    B, C = 4, 2
    learned = kw.get("sampler_parameters", {}).get("var_type") == "learned_range"
    m = Stub((B, 2 * C if learned else C, 8, 8)).to(DEV)
    d = Diffuser(m, model_type="gaussian_diffusion", sampling_method="ddpm", n_steps=1000, extra_args=kw)
    calls, draws = [], []
    orig_call, orig_randint = ops._call, torch.randint
    monkeypatch.setattr(ops, "_call", lambda name, *a: (calls.append(name), orig_call(name, *a))[1])
    monkeypatch.setattr(torch, "randint", lambda *a, **k: (draws.append((a, k)), orig_randint(*a, **k))[1])
    t = d.draw_timesteps(B)
    assert draws == [((0, 1000, (B,)), {"dtype": torch.int32})] and calls == [] and t.device.type == "cpu" and t.dtype == torch.int32
    x0 = synth.uniform("vlbt.calls", (B, C, 8, 8), lo=-1.0, hi=1.0).to(DEV)
    losses = d.compute_loss({"x": x0}, timesteps=t)
    assert calls == ["dl_ddpm_add_noise", fwd] and set(losses) == ({"loss", "vb"} if learned else {"loss"})
    sum(losses.values()).backward()
    assert calls == ["dl_ddpm_add_noise", fwd, bwd] and not d.diffusion.last_terms and d.diffusion.timestep_sampler_state is None


@pytest.mark.parametrize("family,mean_type", [("unet", "epsilon"), ("dit", "v")])
def test_vlb_loss_and_gradients_end_to_end(family, mean_type):
    from diffulab_amd.training.optim import FusedAdamW

    extra = {"sampler_parameters": {"var_type": "learned_range", "mean_type": mean_type}, "loss_type": "vlb"}
    if mean_type != "epsilon":
        extra["loss_target"] = "mean_type"
    d, m, C, head = diffuser(family, **extra)
    gd = d.diffusion
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    B = 4
    x0 = synth.uniform(f"vlbt.{family}", (B, C, 16, 16), lo=-1.0, hi=1.0).to(DEV)
    noise = synth.normal(f"vlbt.{family}.n", (B, C, 16, 16)).to(DEV)
    y = synth.integers("vlbt.y", (B,), 10).to(DEV)
    ti = torch.tensor([0, 1, 4, 7], dtype=torch.int32)
    seen = []
    h = m.register_forward_hook(lambda mod, a, kw, out: seen.append((kw["x"].detach().clone(), out["x"].detach().clone())), with_kwargs=True)
    try:
        losses = d.compute_loss({"x": x0.clone(), "y": y, "p": 0.0}, timesteps=ti, noise=noise)
    finally:
        h.remove()
    assert set(losses) == {"loss"} and losses["loss"].shape == () and bool(torch.isfinite(losses["loss"]))
    assert set(gd.last_terms) == {"t", "mse", "vb", "total"} and torch.equal(gd.last_terms["total"], gd.last_terms["vb"])
    assert all(v.shape == (B,) and v.is_cuda and not v.requires_grad for v in gd.last_terms.values())
    losses["loss"].backward()
    w = dict(m.named_parameters())[head]
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters() if p.grad is not None)
    rows_of_mean = w.grad.flatten(1).abs().sum(1)[:C] if family == "unet" else w.grad.flatten(1).abs().sum(1)
    assert bool((rows_of_mean > 0).all())  # the parameters that feed the mean output receive the bound's gradient
    before = w.detach().clone()
    opt.step()
    assert bool(torch.isfinite(w).all()) and not torch.equal(w.detach(), before)
    # "loss" against the restatement on the prediction the denoiser made
    (xt, pred), = seen
    tab = gd.sampler._tables(torch.device("cpu"))
    args = (tab, pred.float().cpu(), noise.cpu(), x0.cpu(), xt.cpu(), ti, mean_type, "learned_range", None, None, "vlb", gd.vlb_weight)
    with torch.no_grad():
        ref, cpu32 = vt.rows(*args, torch.float64), vt.rows(*args, torch.float32)
    assert float(ref["prob"][ref["first"]].min()) > 10 * 1e-12
    check(f"{family} {mean_type} vlb loss", losses["loss"].detach().view(1), ref["loss"][1:], cpu32["loss"][1:])
    check(f"{family} {mean_type} vlb rows", gd.last_terms["vb"], ref["vb_row"], cpu32["vb_row"])


def test_loss_second_moment_sampler_end_to_end(monkeypatch):
    """an 8-step chain fed with seeded draws until the warm-up is over: the state equals the numpy resampler fed the same
    `last_terms`; validation under no_grad leaves it bit-identical; nothing inside draw_timesteps / compute_loss reads a device value
    back (`.item()`, `.cpu()`, `.tolist()` raise while they run)"""
    d, m, C, head = diffuser("dit", timestep_sampler="loss_second_moment", sampler_history=3, sampler_uniform_prob=0.01)
    gd = d.diffusion
    state = gd.timestep_sampler_state
    r = vt.Resampler(8, 3, 0.01)
    B = 8
    y = synth.integers("vlbt.lsm.y", (B,), 10).to(DEV)
    torch.manual_seed(11)

    def guarded(fn, *a, **k):
        def refuse(self, *a_, **k_):
            raise AssertionError("a device value was read back")

        with monkeypatch.context() as mp_:
            for name in ("item", "cpu", "tolist"):
                mp_.setattr(torch.Tensor, name, refuse)
            return fn(*a, **k)

    warm_at = None
    for step in range(40):
        x0 = synth.uniform(f"vlbt.lsm.{step % 3}", (B, C, 16, 16), lo=-1.0, hi=1.0).to(DEV)
        t = guarded(d.draw_timesteps, B)
        assert t.is_cuda and t.dtype == torch.int32 and t.shape == (B,)
        imp_before = state.tensors["imp"].clone()
        losses = guarded(d.compute_loss, {"x": x0, "y": y, "p": 0.0}, timesteps=t)
        assert set(losses) == {"loss", "vb"} and set(gd.last_terms) == {"t", "mse", "vb", "total"}
        guarded(sum(losses.values()).backward)
        lt = {k: v.cpu() for k, v in gd.last_terms.items()}
        assert torch.equal(lt["t"], t.cpu()) and int(lt["t"].min()) >= 0 and int(lt["t"].max()) < 8
        # the scalars carry the weights the step was drawn with; total_b is the sample's loss before them
        im = imp_before.cpu()[lt["t"].long()]

        def scalars(dtype):
            w, mse, vb = im.to(dtype), lt["mse"].to(dtype), lt["vb"].to(dtype)
            return torch.stack([(w * mse).mean(), gd.vlb_weight * (w * vb).mean()]), mse + gd.vlb_weight * vb

        (want, total), (want32, total32) = scalars(torch.float64), scalars(torch.float32)
        check(f"step {step} scalars", torch.stack([losses["loss"].detach(), losses["vb"].detach()]), want, want32)
        check(f"step {step} total", lt["total"], total, total32)
        r.update(lt["t"].numpy(), lt["total"].numpy())
        assert np.array_equal(state.tensors["history"].cpu().numpy(), r.hist) and np.array_equal(state.tensors["counts"].cpu().numpy(), r.count)
        if r.warmed_up() and warm_at is None:
            warm_at = step
        if warm_at is not None and step >= warm_at + 2:
            break
    assert warm_at is not None and warm_at > 0, "the seeded draws complete the warm-up within 40 steps"
    for key, ref, c32 in zip(("p", "imp", "cdf"), r.tables(np.float64), r.tables(np.float32)):
        check(f"after warm-up {key}", state.tensors[key], torch.from_numpy(ref), torch.from_numpy(c32))
    p = state.tensors["p"].cpu()
    assert float(p.max()) > float(p.min()) > 0
    # validation: drawn from the current distribution, weighted, and the state untouched
    snap = {k: v.clone() for k, v in state.tensors.items()}
    with torch.no_grad():
        t = guarded(d.draw_timesteps, B)
        val = guarded(d.compute_loss, {"x": x0, "y": y, "p": 0.0}, timesteps=t)
    assert all(bool(torch.isfinite(v)) for v in val.values())
    for k, v in snap.items():
        assert torch.equal(v.view(torch.int32) if v.dtype == torch.float32 else v, state.tensors[k].view(torch.int32) if v.dtype == torch.float32
                           else state.tensors[k]), k
    sd = state.state_dict()
    gd.set_steps(8)  # the same chain: kept
    assert torch.equal(state.tensors["counts"], sd["counts"])
    gd.set_steps(20)  # another chain: a fresh history
    assert state.n_steps == 20 and int(state.on(DEV)["counts"].sum()) == 0 and state.tensors["history"].shape == (20, 3)


def test_trainer_lowers_the_bound_with_the_config_settings(tmp_path):
    """30 steps of `BaseTrainer.training_step` with the settings of configs/train_mnist_ddpm_vlb.yaml (learned_range, loss_type vlb,
    loss_second_moment with its defaults) on an 8-step chain; the bound of a fixed probe (fixed samples, timesteps and noise, uniform
    weights) is lower afterwards"""
    from diffulab_amd import Diffuser
    from diffulab_amd.config import load_config
    from diffulab_amd.training import BaseTrainer, FusedAdamW
    from diffulab_amd.training.utils import AverageMeter
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ea = load_config(os.path.join(root, "configs"), "train_mnist_ddpm_vlb").diffuser.extra_args
    extra = {k: (dict(v) if hasattr(v, "items") else v) for k, v in ea.items()}
    d, m, C, head = diffuser("dit", **extra)
    assert d.diffusion.loss_type == "vlb" and d.diffusion.timestep_sampler_state.history_per_term == 10
    probe = Diffuser(m, model_type="gaussian_diffusion", sampling_method="ddpm", n_steps=1000,
                     extra_args={"sampler_parameters": {"var_type": "learned_range"}, "loss_type": "vlb"})
    probe.set_steps(8)
    B = 16
    data = [(synth.uniform(f"vlbt.tr.x{i}", (B, C, 16, 16), lo=-1.0, hi=1.0), synth.integers(f"vlbt.tr.y{i}", (B,), 10)) for i in range(2)]
    pt = torch.arange(B, dtype=torch.int32) % 8
    pn = synth.normal("vlbt.tr.n", (B, C, 16, 16)).to(DEV)

    def bound():
        with torch.no_grad():
            return sum(float(probe.compute_loss({"x": x.to(DEV), "y": y.to(DEV), "p": 0.0}, timesteps=pt, noise=pn)["loss"]) for x, y in data)

    before = bound()
    opt = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.0)
    tr = BaseTrainer(n_epoch=1, save_path=tmp_path, project_name="vlb")
    meter = AverageMeter()
    torch.manual_seed(5)
    for step in range(30):
        x, y = data[step % 2]
        tr.training_step(d, opt, {"model_inputs": {"x": x, "y": y}}, meter, p_classifier_free_guidance=0.1)
    after = bound()
    avg = meter.avg
    print(f"probe bound before {before:.6g}  after {after:.6g}  train/loss mean {avg['train/loss']:.6g}")
    assert set(avg) == {"train/loss"} and np.isfinite(avg["train/loss"]) and np.isfinite(after) and after < before
    counts = d.diffusion.timestep_sampler_state.tensors["counts"]
    assert int(counts.max()) == 10 and int(counts.min()) > 0  # 480 pairs over 8 indices went into the history

