"""CPU checks of image-to-image and inpainting sampling (`Diffuser.generate(init_image=, strength=, mask=, resample=)`): the step-count
rule, the argument validation (before any device work), the new C entry point's declaration, export and refusals, and the semantics
themselves on the f64 restatement of tests/image_cond_common.py."""

import ctypes
import inspect
import re

import pytest
import torch

import image_cond_common as ic
from diffulab_amd import _lib, ops
from oracle import diffusion as od
from oracle import synth

SHAPE = (2, 3, 5, 7)


# ------------------------------------------------------------------------------------------------------------------ step count
def test_strength_to_steps_table():
    from diffulab_amd.diffuse.utils import strength_to_steps

    for (steps, strength), k in ic.STEP_TABLE:
        assert strength_to_steps(steps, strength) == k == ic.strength_steps(steps, strength), (steps, strength)
    for steps in (1, 4, 6, 50, 1000):  # never outside 1 .. steps, monotone in strength
        ks = [strength_to_steps(steps, s / 64) for s in range(1, 65)]
        assert ks[0] >= 1 and ks[-1] == steps and ks == sorted(ks), steps


# ------------------------------------------------------------------------------------------------------------------ validation
def _diffusers():
    from diffulab_amd import Diffuser

    flow = Diffuser(ic.Mixer(), sampling_method="euler", model_type="rectified_flow", n_steps=6)
    gd = Diffuser(ic.Mixer(), sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=6, extra_args={"schedule": "cosine"})
    return flow, gd


BAD = [
    ("strength", dict(strength=0.0)), ("strength", dict(strength=-0.5)), ("strength", dict(strength=1.5)),
    ("strength", dict(strength=float("nan"))), ("strength", dict(strength="0.5")),
    ("init_image", dict(strength=0.5, init_image=None)),
    ("init_image", dict(mask=torch.ones(2, 1, 5, 7), init_image=None)),
    ("resample", dict(resample=0)), ("resample", dict(resample=-2)), ("resample", dict(resample=1.5)), ("resample", dict(resample=True)),
    ("mask", dict(resample=2)), ("mask", dict(resample=2, init_image=None)),
    ("init_image", dict(init_image=torch.zeros(2, 3, 5, 8))), ("init_image", dict(init_image=torch.zeros(1, 3, 5, 7))),
    ("init_image", dict(init_image=torch.zeros(2, 3, 35))),
    ("mask", dict(mask=torch.ones(2, 2, 5, 7))), ("mask", dict(mask=torch.ones(2, 5, 7))), ("mask", dict(mask=torch.ones(1, 1, 5, 7))),
    ("mask", dict(mask=torch.ones(2, 1, 7, 5))),
    ("mask", dict(mask=torch.full((2, 1, 5, 7), 1.5))), ("mask", dict(mask=torch.full((2, 1, 5, 7), -0.25))),
    ("mask", dict(mask=torch.full((2, 3, 5, 7), float("nan")))), ("mask", dict(mask=torch.ones(2, 1, 5, 7, dtype=torch.int32))),
]


@pytest.mark.parametrize("which", ["flow", "gaussian"])
def test_bad_arguments_raise_a_value_error_naming_them_before_any_device_work(which, monkeypatch):
    """ops.lib is the only door to the device library: with it barred, a call that passed validation would raise RuntimeError"""
    def barred():
        raise RuntimeError("the device library was reached before the arguments were validated")

    monkeypatch.setattr(ops, "lib", barred)
    monkeypatch.setattr(ops, "_LIB", None)
    d = dict(zip(("flow", "gaussian"), _diffusers()))[which]
    for name, kw in BAD:
        kw = {"init_image": torch.zeros(SHAPE), **kw}
        for entry in (lambda **a: d.generate({}, data_shape=SHAPE, use_tqdm=False, **a),
                      lambda **a: d.diffusion.denoise(d.denoiser, {}, data_shape=SHAPE, use_tqdm=False, **a)):
            with pytest.raises(ValueError, match=name):
                entry(**kw)
    # a valid call gets past the validation and then needs the device library (CPU tensors here)
    with pytest.raises(RuntimeError):
        d.generate({}, data_shape=SHAPE, use_tqdm=False, init_image=torch.zeros(SHAPE), strength=0.5)
    # the shape of the generated tensor is that of model_inputs["x"] when it is given
    with pytest.raises(ValueError, match="init_image"):
        d.generate({"x": torch.zeros(2, 3, 5, 6)}, use_tqdm=False, init_image=torch.zeros(SHAPE))


def test_the_new_arguments_follow_the_existing_ones_with_inert_defaults():
    from diffulab_amd import Diffuser
    from diffulab_amd.diffuse.modelizations.diffusion import Diffusion
    from diffulab_amd.diffuse.modelizations.flow import Flow
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion

    new = [("init_image", None), ("strength", 1.0), ("mask", None), ("resample", 1)]
    for fn in (Diffuser.generate, Diffusion.denoise, Flow.denoise, GaussianDiffusion.denoise):
        ps = list(inspect.signature(fn).parameters.values())
        assert [(p.name, p.default) for p in ps[-4:]] == new, fn.__qualname__
        assert ps[-5].name in ("return_intermediates", "return_latents"), fn.__qualname__


# ------------------------------------------------------------------------------------------------------------------ ABI
ARGS = ["x", "ref", "noise", "mask", "a", "b", "out", "batch", "channels", "hw", "mask_channels", "stream"]


def test_header_declares_library_exports_and_ops_wraps_the_entry_point():
    text = open(_lib.HEADER_PATH).read()
    steps = text[text.index("sampler steps"):text.index("GEMMs (bf16 in")]
    assert re.search(r"DL_API\s+int\s+dl_inpaint_blend\(", steps)
    comment = steps[:steps.index("DL_API int dl_inpaint_blend")]
    for cited in ("SDEdit", "RePaint", "Meng et al.", "Lugmayr et al.", "flow.py", "gaussian_diffusion.py"):
        assert cited in comment[comment.rindex("/*"):], cited
    restype, argtypes, names = _lib.parse_header()["dl_inpaint_blend"]
    assert names == ARGS and restype is ctypes.c_int
    assert argtypes == [ctypes.c_void_p] * 4 + [ctypes.c_float] * 2 + [ctypes.c_void_p] + [ctypes.c_int64] * 4 + [ctypes.c_void_p]
    L = _lib.lib()
    assert "dl_inpaint_blend" in L.protos and callable(L.cdll.dl_inpaint_blend)  # (exported by the built library)
    assert callable(ops.inpaint_blend)
    assert list(inspect.signature(ops.inpaint_blend).parameters) == ["x", "ref", "noise", "mask", "a", "b", "out"]


def test_entry_point_refuses_out_of_contract_arguments_before_any_launch():
    """dummy non-null pointers are never dereferenced: every case is refused by DL_CHECK_ARG"""
    buf = ctypes.create_string_buffer(256)
    P = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    L = _lib.lib()
    f, i64 = ctypes.c_float, ctypes.c_int64

    def call(x=P, ref=P, noise=P, mask=P, a=0.75, b=0.25, out=P, batch=2, channels=3, hw=5, mc=1):
        rc = L.cdll.dl_inpaint_blend(x, ref, noise, mask, f(a), f(b), out, i64(batch), i64(channels), i64(hw), i64(mc), None)
        return rc, L.cdll.dl_last_error().decode()

    bad = [dict(ref=None), dict(out=None), dict(noise=None),  # (b != 0 without noise)
           dict(x=None),  # a mask and no x
           dict(mask=None),  # x and no mask
           dict(mc=2), dict(mc=0), dict(mc=6), dict(mc=-1),
           dict(batch=0), dict(channels=0), dict(hw=0), dict(batch=-1), dict(hw=-3),
           dict(x=None, mask=None, ref=None, mc=0), dict(x=None, mask=None, noise=None, mc=0)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc < 0 and re.search(r"\bdl_inpaint_blend\b", msg), (kw, rc, msg)
    assert "mask_channels" in call(mc=2)[1] and "noise" in call(noise=None)[1] and "mask" in call(x=None)[1]
    del buf


# ------------------------------------------------------------------------------------------------------------------ semantics (f64)
def _k(steps: int, strength: float) -> int:
    """the number of steps to run: the product's rule and the restatement's agree"""
    from diffulab_amd.diffuse.utils import strength_to_steps

    k = strength_to_steps(steps, strength)
    assert k == ic.strength_steps(steps, strength)
    return k


def _case(seed: str):
    init = synth.uniform(f"ic.init.{seed}", SHAPE, lo=-1.0, hi=1.0)
    mask = torch.zeros(SHAPE[0], 1, *SHAPE[2:])
    mask[..., 4:] = 1.0  # generate the right half-plane, keep the left
    noises = [synth.normal(f"ic.nz.{seed}.{i}", SHAPE) for i in range(40)]
    return init, mask, noises


def test_blend_ref_selects_and_mixes():
    """the restatement of `ops.inpaint_blend` (same operands, in the same order)"""
    assert list(inspect.signature(ic.blend_ref).parameters)[:6] == list(inspect.signature(ops.inpaint_blend).parameters)[:6]
    x, ref, nz = (synth.normal(f"ic.b.{k}", SHAPE).double() for k in "xrn")
    m = torch.tensor([0.0, 1.0, 0.25, 0.5, 1.0, 0.0, 0.75]).view(1, 1, 1, 7).expand(2, 1, 5, 7)
    known = 0.75 * ref + 0.25 * nz
    out = ic.blend_ref(x, ref, nz, m, 0.75, 0.25)
    hard1, hard0 = (m >= 1).expand_as(out), (m <= 0).expand_as(out)
    assert torch.equal(out[hard1], x[hard1]) and torch.equal(out[hard0], known[hard0])
    soft = ~(hard1 | hard0)
    mm = m.double().expand_as(out)
    assert torch.equal(out[soft], (mm * x + (1 - mm) * known)[soft])
    # selects: nothing non-finite crosses from the discarded side
    xn, rn = x.clone(), ref.clone()
    xn[hard0] = float("nan")
    rn[hard1] = float("inf")
    assert bool(torch.isfinite(ic.blend_ref(xn, rn, nz, m, 0.75, 0.25)).all())
    assert torch.equal(ic.blend_ref(None, ref, None, None, 1.0, 0.0), ref) and torch.equal(ic.blend_ref(None, ref, nz, None, 0.75, 0.25), known)


@pytest.mark.parametrize("sampler", ["euler", "euler_maruyama"])
@pytest.mark.parametrize("strength,resample", [(1.0, 1), (0.5, 1), (0.7, 3)])
def test_flow_restatement_known_region_follows_one_trajectory_and_ends_at_the_image(sampler, strength, resample):
    init, mask, noises = _case("flow")
    ts = od.flow_timesteps(6, shift=3.0)
    model = ic.Mixer()
    out = ic.flow_loop(model, ts, init, noises, mask, strength, resample, sampler)
    keep = (mask <= 0).expand(SHAPE)
    assert torch.equal(out["x"][keep], init.double()[keep])
    k = _k(6, strength)
    assert len(out["xt"]) == k + 1 and model.calls == ic.n_model_calls(6, strength, resample, False)
    eps0 = noises[0].double()
    for i, x in zip(range(6 - k, 7), out["xt"]):
        want = (1 - ts[i]) * init.double() + ts[i] * eps0
        assert torch.equal(x[keep], want[keep]), i
    assert not torch.equal(out["x"][~keep], init.double()[~keep])


@pytest.mark.parametrize("sampler", ["ddpm", "ddim"])
@pytest.mark.parametrize("strength,resample", [(1.0, 1), (0.5, 2)])
def test_gaussian_restatement_known_region_ends_at_the_image(sampler, strength, resample):
    init, mask, noises = _case("gd")
    T = od.GaussianTables(6, schedule="cosine")
    model = ic.Mixer()
    out = ic.gaussian_loop(model, T, init, noises, mask, strength, resample, sampler)
    keep = (mask <= 0).expand(SHAPE)
    assert torch.equal(out["x"][keep], init.double()[keep]) and bool(torch.isfinite(out["x"]).all())
    k = _k(6, strength)
    assert len(out["xt"]) == k + 1 and model.calls == ic.n_model_calls(6, strength, resample, False)
    assert not torch.equal(out["x"][~keep], init.double()[~keep])


def test_point_mass_flow_fills_the_generated_region_with_c():
    init, mask, noises = _case("pm")
    gen = (mask >= 1).expand(SHAPE)
    for strength, resample in ((1.0, 1), (0.5, 1), (1.0, 2)):
        _k(6, strength)
        for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 1e-6)):
            out = ic.flow_loop(ic.PointMass(0.25), od.flow_timesteps(6), init, noises, mask, strength, resample, "euler", dtype=dtype)
            assert float((out["x"][gen] - 0.25).abs().max()) <= tol, (strength, resample, dtype)
            assert torch.equal(out["x"][~gen], init.to(dtype)[~gen])


def test_renoise_keeps_the_marginal():
    """algebra, not sampling: the re-noised x_t has the mean coefficient and the variance of the marginal at t_curr"""
    from diffulab_amd.diffuse.utils import flow_renoise_coefs

    for steps in (4, 6, 50):
        for shift in (None, 3.0):
            ts = od.flow_timesteps(steps, shift)
            for t_curr, t_prev in zip(ts[:-2], ts[1:-1]):  # (the last step is never repeated)
                a, s = flow_renoise_coefs(t_curr, t_prev)
                assert (a, s) == ic.flow_renoise_coefs(t_curr, t_prev)
                assert 0.0 <= a <= 1.0 and t_curr * t_curr - a * a * t_prev * t_prev > 0.0
                assert abs(a * (1 - t_prev) - (1 - t_curr)) <= 1e-12
                assert abs(a * a * t_prev * t_prev + s * s - t_curr * t_curr) <= 1e-12
    for T in (od.GaussianTables(1000), od.GaussianTables(1000, 6), od.GaussianTables(6, schedule="cosine")):
        ab = T.alphas_bar
        for t in range(1, T.steps):
            a, s = ic.gaussian_renoise_coefs(T.betas, t)
            assert abs(a * a * float(ab[t - 1]) - float(ab[t])) <= 1e-12
            assert abs(a * a * (1 - float(ab[t - 1])) + s * s - (1 - float(ab[t]))) <= 1e-12
