"""GPU checks of the UNet's dropout: ``dl_dropout`` element by element against the numpy mask definition (tests/dropout_common.py) and
the fp64 value, with write guards; then ``UNetModel(dropout=0.3)`` in ``train()`` mode against the outputs of the reference run with the
same masks (tests/golden/unet_dropout.npz + unet_dropout_wide.npz, made by tests/golden/make_unet_dropout_golden.py), in both precision
regimes and at the bars the p = 0 fixture is held to; eval mode and launch-plan replay."""

import functools

import numpy as np
import pytest
import torch

import dropout_common as dc

pytestmark = pytest.mark.gpu

from oracle import diffusion as od  # noqa: E402
from oracle import synth  # noqa: E402
from oracle import unet as ounet  # noqa: E402

DEV = "cuda"
BF = torch.bfloat16
SEED = 0x123456789ABCDEF0  # (a key with a non-zero high word)
STATES = ((3, 7), (123456789, 14))  # (step, site)

# the launch cap of the elementwise kernels (csrc/common.h, ew_grid): at most 2048 workgroups of 256 threads, and a thread of
# dropout_k takes one group of 8 elements per iteration: one pass of the grid covers 2048 * 256 * 8 = 4194304 elements
ONE_PASS = 2048 * 256 * 8
BIG = (4100, 1024)
assert BIG[0] * BIG[1] > ONE_PASS


def rel(a, b):
    a = torch.as_tensor(a).detach().double().cpu()
    b = torch.as_tensor(b).detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def halves(n, step, site):
    return dc.halves(n, SEED, step, site)


@functools.lru_cache(maxsize=None)
def values(tag, rows, cols):
    """|v| in [0.5, 2] with a random sign, exactly representable in bf16 (so both dtypes start from the same numbers)"""
    u = synth.uniform(f"drop.{tag}.{rows}x{cols}", (rows, cols), lo=0.5, hi=2.0)
    s = synth.uniform(f"drop.{tag}.sign.{rows}x{cols}", (rows, cols), lo=-1.0, hi=1.0)
    return (u * torch.where(s < 0, -1.0, 1.0)).to(BF).float()


def bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


def ulp(ref64, dtype):
    """one unit in the last place of `dtype` at |ref64| (normal range)"""
    e = np.floor(np.log2(np.maximum(np.abs(ref64), 1e-30)))
    return 2.0 ** (e - (7 if dtype == BF else 23))


def pitched(src, ld, dtype, sentinel):
    """[rows + 2, ld] buffer full of `sentinel` with `src` in its [rows, cols] window (pad columns and two guard rows around it)"""
    rows, cols = src.shape
    buf = torch.full((rows + 2, ld), sentinel, dtype=dtype, device=DEV)
    buf[:rows, :cols] = src.to(DEV, dtype)
    return buf


def outside_unchanged(buf, before, rows, cols):
    a, b = bits(buf).clone(), bits(before).clone()
    a[:rows, :cols] = 0
    b[:rows, :cols] = 0
    return torch.equal(a, b)


def run_case(rows, cols, dtype, with_resid, inplace, pad, p, step, site, state, zero_patterns):
    from diffulab_amd import ops

    ld = cols + pad
    T, scale = ops.dropout_threshold(p), ops.dropout_scale(p)
    assert T == dc.threshold(p) and np.float32(scale) == dc.scale_of(p)
    xv, rv = values("x", rows, cols), values("r", rows, cols)
    xb = pitched(xv, ld, dtype, -777.0)
    rb = pitched(rv, ld, dtype, 555.0) if with_resid else None
    ob = xb if inplace else torch.full((rows + 2, ld), 333.0, dtype=dtype, device=DEV)
    x_before, o_before = xb.clone(), ob.clone()
    r_before = rb.clone() if with_resid else None
    state.copy_(torch.tensor([SEED, step], dtype=torch.int64))
    win = lambda b: b[:rows, :cols]  # noqa: E731
    ops.dropout(win(xb), win(ob), state, site, T, scale, resid=win(rb) if with_resid else None)
    torch.cuda.synchronize()
    cid = (rows, cols, str(dtype), with_resid, inplace, pad, p, step, site)
    # write guards: pad columns and guard rows of every buffer, and all of the read-only operands
    assert outside_unchanged(ob, o_before, rows, cols), cid
    if not inplace:
        assert torch.equal(bits(xb), bits(x_before)), cid
    if with_resid:
        assert torch.equal(bits(rb), bits(r_before)), cid
    keep = (halves(rows * cols, step, site) >= T).reshape(rows, cols)
    got = win(ob).float().cpu().numpy().astype(np.float64)
    r64 = rv.numpy().astype(np.float64) if with_resid else np.zeros((rows, cols))
    # dropped: resid bit for bit, or a zero of either sign
    if with_resid:
        gb, rbits = bits(win(ob).contiguous()).cpu().numpy(), bits(win(r_before).contiguous()).cpu().numpy()
        assert np.array_equal(gb[~keep], rbits[~keep]), cid
    else:
        assert np.all(got[~keep] == 0.0), cid
        assert np.all(got[keep] != 0.0), cid
        other = zero_patterns.setdefault((rows, cols, inplace, pad, p, step, site), got == 0.0)
        assert np.array_equal(other, got == 0.0), (cid, "bf16 and f32 disagree on which elements are dropped")
    # kept: within one unit in the last place of the fp64 value x * scale + resid (fma or multiply-then-add, one or two roundings)
    ref = xv.numpy().astype(np.float64) * np.float64(np.float32(scale)) + r64
    err = np.abs(got - ref)[keep] / ulp(ref, dtype)[keep]
    assert err.size == 0 or err.max() <= 1.0, (cid, err.max())
    assert 0 < keep.sum() or rows * cols <= 8
    if not inplace:  # the same state again: identical bits
        ob2 = torch.full((rows + 2, ld), 333.0, dtype=dtype, device=DEV)
        ops.dropout(win(xb), win(ob2), state, site, T, scale, resid=win(rb) if with_resid else None)
        assert torch.equal(bits(ob2), bits(ob)), cid
    return float(err.max()) if err.size else 0.0


# ------------------------------------------------------------------ 1. the kernel, element by element
@pytest.mark.parametrize("rows,cols", [(1, 8), (67, 96), (1024, 128)])
def test_kernel_element_by_element(rows, cols):
    """both dtypes x with / without resid x in place / out of place x pitch cols / cols + 8 x p in {0.1, 0.5} x two (step, site)"""
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    zero_patterns: dict = {}
    worst = 0.0
    for dtype in (BF, torch.float32):
        for with_resid in (False, True):
            for inplace in (False, True):
                for pad in (0, 8):
                    for p in (0.1, 0.5):
                        for step, site in STATES:
                            worst = max(worst, run_case(rows, cols, dtype, with_resid, inplace, pad, p, step, site, state, zero_patterns))
    print(f"\n[{rows} x {cols}] worst kept-element error: {worst:.3f} ulp")
    assert len(zero_patterns) == 16


def test_kernel_beyond_one_pass_of_the_grid():
    """BIG = 4100 x 1024 = 4198400 elements > ONE_PASS = 4194304: the last 4096 elements are reached by the grid-stride loop only"""
    rows, cols = BIG
    state = torch.zeros(2, dtype=torch.int64, device=DEV)
    zero_patterns: dict = {}
    for dtype in (BF, torch.float32):
        run_case(rows, cols, dtype, False, True, 0, 0.5, *STATES[0], state, zero_patterns)  # the dense form
        run_case(rows, cols, dtype, True, False, 8, 0.1, *STATES[1], state, zero_patterns)  # the pitched form


# ------------------------------------------------------------------ whole model
KW = dict(image_size=(16, 16), in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(2,),
          channel_mult=(1, 2), num_heads=2, use_scale_shift_norm=True, resblock_updown=True, n_classes=10, classifier_free=True)


def make_model(dropout, precision="bf16"):
    from diffulab_amd.networks.denoisers import UNetModel

    mk = dict(KW, image_size=list(KW["image_size"]), attention_resolutions=list(KW["attention_resolutions"]),
              channel_mult=", ".join(map(str, KW["channel_mult"])))
    m = UNetModel(dropout=dropout, **mk)
    m.load_state_dict(synth.generic_params(ounet.param_shapes(ounet.UNetConfig(**KW)), seed=23))
    return m.set_precision(precision).to(DEV)


@functools.lru_cache(maxsize=None)
def inputs():
    B = 4
    x0, noise = synth.normal("un.x0", (B, 1, 16, 16)), synth.normal("un.noise", (B, 1, 16, 16))
    yl = synth.integers("un.y", (B,), 10)
    ti = torch.tensor([3, 500, 999, 0], dtype=torch.int32)
    xt = od.ddpm_add_noise(od.GaussianTables(1000), x0, ti, noise)
    return x0.to(DEV), noise.to(DEV), yl.to(DEV), ti.to(DEV), xt.to(DEV)


def fixture(golden):
    return {**golden("unet_dropout"), **golden("unet_dropout_wide")}


def test_same_seed_and_step_same_masks_next_step_other_masks():
    m = make_model(dc.FIXTURE_P).train()
    _, _, yl, ti, xt = inputs()
    preds = []
    for seed_step in ((1234, 0), (1234, 0), None, (1234, 1), (1235, 0)):
        if seed_step is not None:
            m.set_dropout_seed(*seed_step)
        with torch.no_grad():
            preds.append(m(x=xt, timesteps=ti, y=yl, p=0.0)["x"].clone())
    assert torch.equal(preds[0], preds[1]), "the same (seed, step) must reproduce the prediction bit for bit"
    assert not torch.equal(preds[1], preds[2]) and rel(preds[2], preds[1]) > 0.1, "the next forward runs at step 1"
    assert torch.equal(preds[2], preds[3]), "a forward advances the step by exactly one"
    assert not torch.equal(preds[4], preds[0])
    assert m._dropout_step == 1 and m._dropout_seed == 1235


def check_against_fixture(golden, precision):
    from diffulab_amd import Diffuser

    g = fixture(golden)
    bf = precision == "bf16"
    m = make_model(float(g["p"]), precision).train()
    assert type(m.engine).__name__ == ("UNetEngine" if bf else "UNetEngineF32")
    assert m.engine.sites == dict(zip(g["site_prefixes"].tolist(), g["site_ids"].tolist()))
    x0, noise, yl, ti, xt = inputs()
    m.set_dropout_seed(int(g["seed"]), int(g["step"]))
    with torch.no_grad():
        pred = m(x=xt, timesteps=ti, y=yl, p=0.0)["x"]
    e_pred = rel(pred, g["un_pred"])
    gd = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    m.set_dropout_seed(int(g["seed"]), int(g["step"]))
    loss = gd.compute_loss({"x": x0, "y": yl, "p": 0.0}, timesteps=ti, noise=noise)["loss"]
    loss.backward()
    e_loss = abs(loss.item() - float(g["un_loss"])) / float(g["un_loss"])
    norms = dict(zip(g["un_grad_names"].tolist(), g["un_grad_norms"].tolist()))
    named = dict(m.named_parameters())
    assert set(named) == set(norms)
    top = max(norms.values())
    floor = (1e-3 if bf else 1e-6) * top
    e_norm = {n: abs(named[n].grad.double().norm().item() - ref) / ref for n, ref in norms.items() if ref > floor}
    e_tensor = {k[5:]: rel(named[k[5:]].grad, g[k]) for k in g if k.startswith("un_g_") and norms[k[5:]] > floor}
    print(f"\nUNet dropout {precision}: prediction {e_pred:.3e}, loss {e_loss:.3e}, worst norm "
          f"{max(e_norm.items(), key=lambda kv: kv[1])}, worst tensors {sorted(((v, k) for k, v in e_tensor.items()), reverse=True)[:4]}")
    if bf:  # the bars of test_unet_gpu.py::test_small_unet_ddpm_loss_and_grads
        assert e_pred < 2e-2
        assert e_loss < 5e-3
        for n, ref in norms.items():
            if ref <= floor:
                assert named[n].grad.double().norm().item() <= 30 * floor, n
            else:
                assert e_norm[n] < (8e-2 if n == "out.2.bias" else 3e-2), (n, e_norm[n])
        for n, e in e_tensor.items():
            if n != "out.2.bias":
                assert e < (4e-2 if g["un_g_" + n].ndim > 1 else 8e-2), (n, e)
    else:  # the bars of test_unet_fp32_gpu.py::test_unet_fp32_against_reference_fixtures
        assert e_pred < 1e-5
        assert e_loss < 1e-5
        for n, ref in norms.items():
            if ref <= floor:
                assert named[n].grad.double().norm().item() <= 1e-4 * top, n
            else:
                assert e_norm[n] < 1e-5, (n, e_norm[n])
        assert max(e_tensor.values()) < 2e-5, sorted(((v, k) for k, v in e_tensor.items()), reverse=True)[:4]


def test_unet_dropout_against_the_reference_fixture_bf16(golden):
    check_against_fixture(golden, "bf16")


def test_unet_dropout_against_the_reference_fixture_fp32(golden):
    check_against_fixture(golden, "fp32")


def test_eval_mode_is_the_dropout_free_model_bit_for_bit():
    m3, m0 = make_model(0.3).eval(), make_model(0.0).eval()
    _, _, yl, ti, xt = inputs()
    outs = []
    with torch.no_grad():
        for _ in range(2):  # the second call of a shape is the hipGraph replay
            outs.append((m3(x=xt, timesteps=ti, y=yl, p=0.0)["x"].clone(), m0(x=xt, timesteps=ti, y=yl, p=0.0)["x"].clone()))
    assert m3._graphs and all(v is not False for v in m3._graphs.values()), "the eval forward of a dropout model is still captured"
    assert torch.equal(outs[0][0], outs[0][1]) and torch.equal(outs[1][0], outs[1][1]) and torch.equal(outs[0][0], outs[1][0])
    assert m3._dropout_step == 0 and m3._dropout_seed is None  # nothing was drawn, nothing advanced


def test_launch_plan_replay_advances_the_step(monkeypatch):
    """DL_LAUNCH_PLAN=1: the training pass is eager, then recorded, then replayed twice.  The recorded dl_dropout launches read
    (seed, step) from device memory, which is written outside the plan: every replay runs at its own step."""
    _, _, yl, ti, xt = inputs()
    w = synth.normal("drop.dy", (4, 1, 16, 16)).to(DEV)

    def run(plans):
        monkeypatch.setenv("DL_LAUNCH_PLAN", "1" if plans else "0")
        m = make_model(dc.FIXTURE_P).train()
        m.set_dropout_seed(1234, 0)
        preds = []
        for _ in range(4):
            m.zero_grad()
            pred = m(x=xt, timesteps=ti, y=yl, p=0.0)["x"]
            (pred * w).sum().backward()
            preds.append(pred.detach().clone())
        made = [v for v in m.engine.__dict__.get("_launch_plans", {}).values() if not isinstance(v, (int, bool))]
        return preds, made, m._flat_grad.clone()

    p1, made, g1 = run(True)
    p0, none, g0 = run(False)
    assert len(made) == 1 and made[0].bwd is not None and not none
    n_sites = 14
    assert sum(1 for fn, _ in made[0].calls if getattr(fn, "__name__", "") == "dl_dropout") == n_sites
    assert sum(1 for fn, _ in made[0].bwd.calls if getattr(fn, "__name__", "") == "dl_dropout") == n_sites
    for k in range(4):
        assert torch.equal(p1[k], p0[k]), f"forward {k + 1} with plans differs from the eager run"
    for a in range(4):
        for b in range(a + 1, 4):
            assert not torch.equal(p1[a], p1[b]), (a, b)
    # the last backward ran under the eager run's masks: the two gradient arenas differ by the order of the f32 atomics in the bias /
    # GroupNorm reductions alone: a few 1e-7 relative per sum, which can flip the bf16 rounding (2^-8 relative) of a value the chain
    # reads back -- so one bf16 ulp, 3.9e-3, over the whole arena bounds it; a backward under another step's masks is off by O(1)
    assert rel(g1, g0) < 2.0**-8
