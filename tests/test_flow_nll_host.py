"""Host tests (no GPU) of the rectified-flow likelihood: the C declarations and refusals of its three entry points, the plain-torch
restatement of the loop (tests/flow_nll_common.py) against the exact log-density of the closed-form Gaussian model, the bound functions
the GPU tests use, and every refusal of `Flow.calc_nll_loop` / `Diffuser.evaluate_nll` / `train(val_nll_batches=...)`."""

import ast
import ctypes
import math
import os

import pytest
import torch

import flow_nll_common as fn
import guidance_common as gc
import multistep_common as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dl_patch_embed_dgrad", "dl_hutchinson_step", "dl_normal_nll_rows")


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_header_declares_and_ops_binds_every_argument():
    from diffulab_amd import _lib

    protos = _lib.parse_header()
    assert protos["dl_patch_embed_dgrad"][2] == ["dtok", "dtype", "ld", "w", "dimg", "B", "C", "H", "W", "p", "D", "stream"]
    assert protos["dl_hutchinson_step"][2] == ["x", "v", "v0", "a", "b", "x_out", "g", "eps", "scale", "partial", "out", "ld", "col", "rows",
                                               "chw", "stream"]
    assert protos["dl_hutchinson_step"][1][3:5] == [ctypes.c_float, ctypes.c_float]
    assert protos["dl_hutchinson_step"][1][8] is ctypes.c_float
    assert protos["dl_normal_nll_rows"][2] == ["x", "partial", "out", "rows", "chw", "stream"]
    tree = ast.parse(open(os.path.join(ROOT, "diffulab_amd", "ops.py")).read())
    bound = {n.args[0].value: len(n.args) - 1 for n in ast.walk(tree)
             if isinstance(n, ast.Call) and getattr(n.func, "id", "") == "_call" and n.args and isinstance(n.args[0], ast.Constant)}
    for name in NEW:
        assert bound[name] == len(protos[name][2]), (name, bound[name])
        assert not name.startswith("dl_f32_")
    exported = _lib.lib().cdll
    for name in NEW:
        assert getattr(exported, name) is not None


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from diffulab_amd import _lib

    L = _lib.lib()
    c = L.cdll
    assert set(NEW) <= set(L.protos)
    buf = ctypes.create_string_buffer(1024)
    P = ctypes.c_void_p(ctypes.addressof(buf))  # a non-null dummy, never dereferenced: the calls below are refused on the host
    i64, F = ctypes.c_int64, ctypes.c_float

    def refused(name, *args):
        assert getattr(c, name)(*args) == -1 and name in c.dl_last_error().decode(), (name, c.dl_last_error().decode())

    def dg(dtok=P, dtype=0, ld=64, w=P, dimg=P, B=2, C=4, H=16, W=16, p=2, D=64):
        refused("dl_patch_embed_dgrad", dtok, dtype, i64(ld), w, dimg, i64(B), i64(C), i64(H), i64(W), i64(p), i64(D), None)

    for k in ("dtok", "w", "dimg"):
        dg(**{k: None})
    dg(dtype=2)
    dg(dtype=-1)
    dg(H=15)          # p does not divide H
    dg(W=18, p=4)     # p does not divide W
    dg(p=0)
    dg(ld=63)         # ld < D
    dg(B=0)
    dg(D=0)
    dg(B=1 << 20, C=4, H=32, W=32)           # the image: 2^32 elements
    dg(B=1 << 14, C=1, H=64, W=64, p=1, D=64, ld=64)  # the tokens: 2^26 rows of 64 = 2^32 elements
    dg(B=1 << 32)

    def hs(x=P, v=P, v0=None, x_out=P, g=P, eps=P, partial=None, out=P, ld=4, col=1, R=2, chw=64):
        refused("dl_hutchinson_step", x, v, v0, F(0.5), F(0.5), x_out, g, eps, F(1.0), partial, out, i64(ld), i64(col), i64(R), i64(chw), None)

    for k in ("g", "eps", "out", "x", "v"):
        hs(**{k: None})
    hs(x_out=None, v0=P)  # v0 without an update
    hs(R=0)
    hs(chw=0)
    hs(ld=0)
    hs(col=4)
    hs(col=-1)
    hs(chw=4097)  # a second share per row needs the scratch
    hs(R=1 << 31, chw=8192, partial=P)  # rows x shares past the grid limit

    def nr(x=P, partial=None, out=P, R=2, chw=64):
        refused("dl_normal_nll_rows", x, partial, out, i64(R), i64(chw), None)

    nr(x=None)
    nr(out=None)
    nr(R=0)
    nr(chw=0)
    nr(chw=4097)
    nr(R=1 << 31, chw=8192, partial=P)


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _grid(n: int, shift: float | None = None) -> list[float]:
    g = torch.linspace(1, 0, n + 1, dtype=torch.float64).tolist()
    return g if shift is None else [shift * t / (1 + (shift - 1) * t) for t in g]


def _closed_form_error(method: str, n: int, shift: float | None = None) -> float:
    """worst of 8 samples, |estimate - exact| in bits per dimension, fp64; the Jacobian is diagonal, so Rademacher probes are exact"""
    g = torch.Generator().manual_seed(11)
    x0 = mc.M + mc.S * torch.randn(8, 1, 8, 8, generator=g, dtype=torch.float64)
    out = fn.nll_loop(mc.flow_field, x0, _grid(n, shift), method, fn.rademacher((1, 8, 1, 8, 8), 3))
    return ((out["nll"] - fn.gaussian_nll(x0)).abs().max() / fn.LN2).item()


def test_restatement_converges_to_the_exact_gaussian_likelihood():
    heun = {n: _closed_form_error("heun", n) for n in (20, 40)}
    euler = {n: _closed_form_error("euler", n) for n in (20, 40)}
    shifted = {n: _closed_form_error("heun", n, shift=3.0) for n in (20, 40)}
    print(f"closed-form model, error in bits/dim: heun {heun}, euler {euler}, heun shift=3 {shifted}")
    assert heun[40] <= 1e-3
    assert heun[20] / heun[40] >= 3.0 and shifted[20] / shifted[40] >= 3.0  # second order
    assert 1.5 <= euler[20] / euler[40] <= 2.5                               # first order


def test_restatement_result_dict_is_consistent():
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(3, 2, 4, 4, generator=g, dtype=torch.float64).clamp(-1, 1)
    stub = gc.Stub(1.0).double()
    y = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    field = lambda x, t: stub(x=x, timesteps=torch.full((x.shape[0],), t, dtype=torch.float64), y=y.repeat(x.shape[0] // 3))["x"]  # noqa: E731
    probes = fn.rademacher((2, 3, 2, 4, 4), 9)
    u = torch.rand(3, 2, 4, 4, generator=g, dtype=torch.float64)
    for method, per in (("euler", 1), ("heun", 2)):
        out = fn.nll_loop(field, x0, _grid(4), method, probes, dequant_noise=u)
        assert out["div_terms"].shape == (3, 4 * per) and out["x1"].shape == x0.shape
        assert torch.allclose(out["nll"], out["prior"] - out["div"])
        assert torch.allclose(out["total_bpd"], out["nll"] / math.log(2.0) + math.log2(127.5))
    # one probe set against the other: the stub's Jacobian is not diagonal, so the estimate depends on the probe
    a = fn.nll_loop(field, x0, _grid(4), "heun", probes[:1])["div"]
    b = fn.nll_loop(field, x0, _grid(4), "heun", probes[1:])["div"]
    assert not torch.allclose(a, b)


# ------------------------------------------------------------------------------------------------------------------ bounds
def test_patch_embed_dgrad_bound_rejects_wrong_layouts():
    B, C, H, W, p, D = 2, 3, 8, 12, 2, 40
    g = torch.Generator().manual_seed(2)
    dtok = torch.randn(B * (H // p) * (W // p), D + 5, generator=g)
    w = torch.randn(D, C * p * p, generator=g)
    ref, mag = fn.patch_embed_dgrad(dtok, w, B, C, H, W, p)
    bound = fn.patch_embed_dgrad_bound(mag, D)
    f32 = (dtok[:, :D].float() @ w.float()).double()  # the same sums in f32, in token-major layout
    img32 = f32.view(B, H // p, W // p, C, p, p).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)
    assert bool(((img32 - ref).abs() <= bound).all())  # an f32 evaluation passes

    def rejected(img):
        return bool(((img - ref).abs() > bound).any())

    dropped = dtok.clone()
    dropped[7, 3] = 0.0  # one element of one token's sum
    assert rejected(fn.patch_embed_dgrad(dropped, w, B, C, H, W, p)[0])
    neighbour = ref.clone()
    neighbour[0, :, 2:4, 4:6], neighbour[0, :, 2:4, 6:8] = ref[0, :, 2:4, 6:8], ref[0, :, 2:4, 4:6]  # a patch in its neighbour's place
    assert rejected(neighbour)
    assert rejected(fn.patch_embed_dgrad(dtok, w, B, C, H, W, p, order="swap")[0])
    assert rejected(fn.patch_embed_dgrad(dtok, w, B, C, H, W, p, order="ppc")[0])


def test_row_bounds_reject_a_dropped_element_and_a_dropped_share():
    g = torch.Generator().manual_seed(4)
    R, n = 3, 2 * fn.SHARE + 101
    gt, eps = torch.randn(R, n, generator=g), fn.rademacher((R, n), 6).float()
    x, v, v0 = (torch.randn(R, n, generator=g) for _ in range(3))
    xo, xb, sums, sb = fn.hutchinson_step(x, v, v0, 0.25, 0.125, gt, eps, 1.0 / n)
    s32 = ((gt * eps).sum(1) * torch.tensor(1.0 / n)).double()
    assert bool(((s32 - sums).abs() <= sb).all())
    x32 = (x + torch.tensor(0.25) * v + torch.tensor(0.125) * v0).double()
    assert bool(((x32 - xo).abs() <= xb).all())
    assert bool(((x.double() + 0.25 * v.double() - xo).abs() > xb).any())  # v0 left out
    # (k grows with the row: one element of 8293 is inside the bound of the long row, so the single drop is shown on a row of 63)
    gs, es = gt[:, :63].contiguous(), eps[:, :63].contiguous()
    _, _, small, smb = fn.hutchinson_step(None, None, None, 0, 0, gs, es, 1.0 / 63)
    one = gs.clone()
    one[1, 17] = 0.0
    assert bool(((fn.hutchinson_step(None, None, None, 0, 0, one, es, 1.0 / 63)[2] - small).abs() > smb)[1])
    share = gt.clone()
    share[:, fn.SHARE: 2 * fn.SHARE] = 0.0
    assert bool(((fn.hutchinson_step(None, None, None, 0, 0, share, eps, 1.0 / n)[2] - sums).abs() > sb).all())
    val, nb = fn.normal_nll_rows(x)
    assert bool(((0.5 * (x * x).mean(1) + torch.tensor(fn.HALF_LOG_2PI, dtype=torch.float32)).double() - val).abs().le(nb).all())
    xs = x[:, :63].contiguous()
    xs[2, 5] = 1.5
    sval, snb = fn.normal_nll_rows(xs)
    big = xs.clone()
    big[2, 5] = 0.0
    assert bool(((fn.normal_nll_rows(big)[0] - sval).abs() > snb)[2])
    cut = x.clone()
    cut[:, :fn.SHARE] = 0.0
    assert bool(((fn.normal_nll_rows(cut)[0] - val).abs() > nb).all())


# ------------------------------------------------------------------------------------------------------------------ validation
def test_every_refusal_is_raised_before_any_device_work(tmp_path):
    from diffulab_amd import Diffuser
    from diffulab_amd.networks.denoisers import DDT, SprintDiT, UNetModel
    from diffulab_amd.networks.denoisers.common import FlatArenaDenoiser
    from diffulab_amd.diffuse.modelizations.flow import NO_VARIATIONAL_BOUND, Flow
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import NO_ODE_LIKELIHOOD, GaussianDiffusion
    from diffulab_amd.training import BaseTrainer

    assert "evaluate_nll" in NO_VARIATIONAL_BOUND and "evaluate_bpd" in NO_ODE_LIKELIHOOD
    x = torch.zeros(2, 3, 8, 8)
    m = gc.Stub(1.0)
    fl = Flow(n_steps=4)
    inputs = {"x": x, "y": torch.tensor([1, 2])}
    for kw, name, exc in (({"method": "rk4"}, "method", ValueError), ({"probe": "sphere"}, "probe", ValueError),
                          ({"n_probes": 0}, "n_probes", ValueError), ({"n_probes": 1.5}, "n_probes", ValueError),
                          ({"probes": torch.zeros(2, 3, 8, 8)}, "probes", ValueError),
                          ({"probes": torch.zeros(1, 2, 3, 8, 4)}, "probes", ValueError),
                          ({"dequant_noise": torch.zeros(2, 3, 8)}, "dequant_noise", ValueError),
                          ({"dequant_noise": torch.ones(2, 3, 8, 8)}, "dequant_noise", ValueError),
                          ({"dequant_noise": -0.1 * torch.ones(2, 3, 8, 8)}, "dequant_noise", ValueError)):
        with pytest.raises(exc, match=name):
            fl.calc_nll_loop(m, inputs, **kw)
    with pytest.raises(NotImplementedError, match="prediction_type"):
        Flow(n_steps=4, prediction_type="x").calc_nll_loop(m, inputs)
    with torch.inference_mode():
        with pytest.raises(RuntimeError, match="inference_mode"):
            fl.calc_nll_loop(m, inputs)
    for cls in (UNetModel, SprintDiT, DDT):
        assert cls.input_grad_capable is False

    class Opaque(FlatArenaDenoiser):  # an engine-driven denoiser without the input gradient (what UNetModel, SprintDiT and DDT are)
        def forward(self, x, timesteps, **kw):
            raise AssertionError("refused before any forward")

    with pytest.raises(NotImplementedError, match="Opaque"):
        fl.calc_nll_loop(Opaque(), inputs)
    with pytest.raises(NotImplementedError, match="evaluate_bpd"):
        GaussianDiffusion(n_steps=8).calc_nll_loop(m, inputs)
    d = Diffuser(m, sampling_method="ddim", model_type="gaussian_diffusion", n_steps=8)
    with pytest.raises(NotImplementedError, match="evaluate_bpd"):
        d.evaluate_nll(inputs)
    df = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=4)
    with pytest.raises(ValueError, match="method"):
        df.evaluate_nll(inputs, method="midpoint")
    assert list(inputs) == ["x", "y"] and inputs["x"] is x and not x.requires_grad
    tr = BaseTrainer(n_epoch=1, save_path=tmp_path, project_name="p")
    with pytest.raises(NotImplementedError) as e:
        tr.train(d, None, [], val_dataloader=[], val_nll_batches=1)
    assert str(e.value) == NO_ODE_LIKELIHOOD and "val_bpd_batches" in NO_ODE_LIKELIHOOD
    with pytest.raises(ValueError, match="val_nll_batches"):
        tr.train(df, None, [], val_nll_batches=-1)


def test_capability_flag():
    from diffulab_amd import MMDiT
    from diffulab_amd.networks.denoisers.common import FlatArenaDenoiser

    assert FlatArenaDenoiser.input_grad_capable is False
    kw = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2, depth=1,
              n_classes=10, classifier_free=True)
    m = MMDiT(simple_dit=True, **kw)
    assert m.input_grad_capable is True
    with m.input_grad_only():
        assert m.__dict__["_input_grad_only"] is True
        with m.input_grad_only():
            pass
        assert m.__dict__["_input_grad_only"] is True
    assert m.__dict__["_input_grad_only"] is False


# ------------------------------------------------------------------------------------------------------------------ fixture
def test_oracle_input_gradient_equals_the_reference_fixture():
    """tests/golden/dit_input_grad.npz (make_input_grad_golden.py: the imported reference's d loss / d z_t on the `pb.small` inputs): the
    oracle's autograd gradient is the fp32 entry to 1e-6 relative (SURVEY 8(c)'s bar for the restatement)"""
    import numpy as np

    from oracle import diffusion as od
    from oracle import dit as odit
    from oracle import synth

    g = np.load(os.path.join(ROOT, "tests", "golden", "dit_input_grad.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "dit_input_grad.npz")) < 100 * 1024
    kw = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2, depth=2,
              n_classes=10, classifier_free=True)
    cfg = odit.DiTConfig(**kw)
    P = synth.dit_params(odit.param_shapes(cfg), seed=5)
    x0, noise = synth.normal("pb.small.x0", (4, 4, 16, 16)), synth.normal("pb.small.noise", (4, 4, 16, 16))
    t, y = synth.uniform("pb.small.t", (4,), lo=0.05, hi=0.95), synth.integers("pb.small.y", (4,), 10)
    z = od.flow_add_noise(x0, t, noise).requires_grad_(True)
    loss = od.flow_loss(odit.dit_forward(P, z, t, y, cfg), x0, noise)
    (dz,) = torch.autograd.grad(loss, z)
    ref = torch.from_numpy(g["dz_fp32"]).double()
    assert ((z.detach().double() - torch.from_numpy(g["z"]).double()).norm() / ref.new_tensor(g["z"]).norm()).item() <= 1e-6
    assert abs(loss.item() - float(g["loss_fp32"])) <= 1e-6 * float(g["loss_fp32"])
    assert ((dz.double() - ref).norm() / ref.norm()).item() <= 1e-6
    ac = torch.from_numpy(g["dz_autocast"]).double()
    assert abs(((ac - ref).norm() / ref.norm()).item() - float(g["autocast_err"])) <= 1e-9 and 1e-3 < float(g["autocast_err"]) < 5e-2
