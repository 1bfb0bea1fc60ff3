"""GPU tests of image-to-image and inpainting sampling: the blend kernel (dl_inpaint_blend) element by element against fp64, the
loops of `Flow.denoise` / `GaussianDiffusion.denoise` against the restatement of tests/image_cond_common.py, the properties of the
product path, and two end-to-end runs on the real engines.

Kernel bound, per element: 6 * 2^-24 * (|m x| + |1 - m| (|a ref| + |b noise|)) + 2^-149.  No term passes through more than five
roundings (1 - m, a product, the sum inside `known`, the blend product, the final sum); the sixth unit holds the second-order terms.

Loop tolerance.  The product and the f32 evaluation of the restatement are both f32 evaluations of the same formulas on the same
inputs and noises; they differ by FMA contraction and by the operation order of the fused step kernels.  So the f32 restatement's own
distance from the f64 restatement is computed per run, and the product may be 4 x as far from f64 as that (the largest |f32 - f64|
over the starting x, every step's x_prev and the final sample).  Both figures come from the restatement, never from the product; the
test prints them.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

import elementwise_bounds as eb  # noqa: E402
import image_cond_common as ic  # noqa: E402
from oracle import diffusion as od  # noqa: E402
from oracle import synth  # noqa: E402

DEV = "cuda"
U = eb.U32
TINY = 2.0**-149


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as _ops

    return _ops


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ the kernel
KERNEL_SHAPES = [(1, 1, 1), (2, 3, 35), (3, 4, 257)]
MASK_VALUES = (0.0, 1.0, 0.25, 0.7)


def kernel_inputs(B, C, hw, mc, off=0):
    x, ref, nz = (synth.normal(f"icg.{k}.{B}.{C}.{hw}", (B, C, hw)) for k in ("x", "ref", "nz"))
    idx = (torch.arange(B * mc * hw) * 7 + off) % len(MASK_VALUES)  # exact 0s, exact 1s and fractions, in every channel and row
    mask = torch.tensor(MASK_VALUES)[idx].view(B, mc, hw).contiguous()
    return x, ref, nz, mask


def bound_of(x, ref, nz, mask, a, b):
    m = torch.zeros_like(ref, dtype=torch.float64) if mask is None else mask.double().expand_as(ref)
    xx = torch.zeros_like(m) if x is None else x.double()
    return 6 * U * ((m * xx).abs() + (1 - m).abs() * ((a * ref.double()).abs() + (b * nz.double()).abs())) + TINY


@pytest.mark.parametrize("a,b", [(0.75, 0.25), (1.0, 0.0)])
@pytest.mark.parametrize("full_mask", [False, True])
@pytest.mark.parametrize("B,C,hw", KERNEL_SHAPES)
def test_blend_kernel_against_fp64_element_by_element(ops, B, C, hw, full_mask, a, b):
    mc = C if full_mask else 1
    for off in (range(len(MASK_VALUES)) if hw == 1 else (0,)):
        x, ref, nz, mask = kernel_inputs(B, C, hw, mc, off)
        want = ic.blend_ref(x, ref, nz, mask, a, b, torch.float64)
        bound = bound_of(x, ref, nz, mask, a, b)
        d = [v.to(DEV) for v in (x, ref, nz, mask)]
        out = ops.inpaint_blend(d[0], d[1], d[2], d[3], a, b)
        assert out.shape == ref.shape and out.dtype == torch.float32
        err = (out.double().cpu() - want).abs()
        worst = float((err / bound).max())
        print(f"\n({B}, {C}, {hw}) mask_channels {mc} (a, b) ({a}, {b}) offset {off}: worst |diff| / bound {worst:.3f}")
        assert bool(torch.isfinite(out).all()) and int((err > bound).sum()) == 0, worst
        # the hard cases are selects: the kept side arrives bit for bit
        m = mask.expand_as(ref).to(DEV)
        known = ops.inpaint_blend(None, d[1], d[2], None, a, b)
        if b == 0.0 and a == 1.0:
            assert torch.equal(bits(known), bits(d[1]))
        assert torch.equal(bits(out)[m >= 1], bits(d[0])[m >= 1]) and torch.equal(bits(out)[m <= 0], bits(known)[m <= 0])
        # ... and nothing non-finite crosses from the discarded side; with b == 0 the noise is not read at all
        xp, rp, npz = d[0].clone(), d[1].clone(), d[2].clone()
        xp[m <= 0] = float("nan")
        rp[m >= 1] = float("nan")
        npz[m >= 1] = float("nan")
        if b == 0.0:
            npz.fill_(float("nan"))
        again = ops.inpaint_blend(xp, rp, npz, d[3], a, b)
        assert torch.equal(bits(again), bits(out))
        if b == 0.0:
            assert torch.equal(bits(ops.inpaint_blend(d[0], d[1], None, d[3], a, b)), bits(out))


@pytest.mark.parametrize("B,C,hw", KERNEL_SHAPES)
def test_renoise_form_without_a_mask_against_fp64(ops, B, C, hw):
    _, ref, nz, _ = kernel_inputs(B, C, hw, 1)
    dr, dn = ref.to(DEV), nz.to(DEV)
    for a, b, noise in ((0.75, 0.25, dn), (0.6, 0.8, dn), (1.0, 0.0, None), (0.5, 0.0, None), (0.5, 0.0, torch.full_like(dn, float("nan")))):
        out = ops.inpaint_blend(None, dr, noise, None, a, b)
        want = ic.blend_ref(None, ref, nz, None, a, b, torch.float64)
        err = (out.double().cpu() - want).abs()
        assert int((err > bound_of(None, ref, nz, None, a, b)).sum()) == 0, (a, b, float(err.max()))


@pytest.mark.parametrize("full_mask", [False, True])
def test_in_place_gives_the_same_bits(ops, full_mask):
    B, C, hw = 3, 4, 257
    x, ref, nz, mask = (v.to(DEV) for v in kernel_inputs(B, C, hw, C if full_mask else 1))
    out = ops.inpaint_blend(x, ref, nz, mask, 0.75, 0.25)
    xi, ri = x.clone(), ref.clone()
    assert ops.inpaint_blend(xi, ref, nz, mask, 0.75, 0.25, out=xi) is xi and torch.equal(bits(xi), bits(out))
    assert ops.inpaint_blend(x, ri, nz, mask, 0.75, 0.25, out=ri) is ri and torch.equal(bits(ri), bits(out))
    known = ops.inpaint_blend(None, ref, nz, None, 0.75, 0.25)
    ri = ref.clone()
    ops.inpaint_blend(None, ri, nz, None, 0.75, 0.25, out=ri)
    assert torch.equal(bits(ri), bits(known))


@pytest.mark.parametrize("hw", [1, 63, 257])
def test_output_stays_inside_its_window(ops, hw):
    B, C = 2, 3
    n = B * C * hw
    for mc in (1, C):
        x, ref, nz, mask = (v.to(DEV) for v in kernel_inputs(B, C, hw, mc))
        g = eb.Guarded(1, n, torch.float32, DEV)
        ops.inpaint_blend(x, ref, nz, mask, 0.75, 0.25, out=g.win.view(B, C, hw))
        g.check(f"dl_inpaint_blend hw {hw} mask_channels {mc}")
    g = eb.Guarded(1, n, torch.float32, DEV)
    ops.inpaint_blend(None, ref, nz, None, 0.75, 0.25, out=g.win.view(B, C, hw))
    g.check(f"dl_inpaint_blend hw {hw} no mask")


# ------------------------------------------------------------------------------------------------------------------ the loops
STEPS = 6
SHAPE = (2, 3, 5, 7)
FLOW, GAUSSIAN = ("euler", "euler_maruyama"), ("ddpm", "ddim")
DDIM_ETA = 0.5


def loop_inputs():
    init = synth.uniform("icg.init", SHAPE, lo=-1.0, hi=1.0)
    mask = torch.zeros(SHAPE[0], 1, *SHAPE[2:])
    mask[..., 4:] = 1.0  # generate the right half-plane, keep the left
    noises = [synth.normal(f"icg.nz.{i}", SHAPE) for i in range(40)]
    return init, mask, noises


def diffuser(sampler, model):
    from diffulab_amd import Diffuser

    if sampler in FLOW:
        return Diffuser(model, sampling_method=sampler, model_type="rectified_flow", n_steps=STEPS)
    return Diffuser(model, sampling_method=sampler, model_type="gaussian_diffusion", n_steps=STEPS, extra_args={"schedule": "cosine"})


def restate(sampler, init, noises, mask, strength, resample, guidance, dtype):
    if sampler in FLOW:
        return ic.flow_loop(ic.Mixer(), od.flow_timesteps(STEPS), init, noises, mask, strength, resample, sampler, 0.7, guidance, dtype)
    return ic.gaussian_loop(ic.Mixer(), od.GaussianTables(STEPS, schedule="cosine"), init, noises, mask, strength, resample, sampler,
                            DDIM_ETA if sampler == "ddim" else 0.0, guidance, dtype)


def hand_out(monkeypatch, noises):
    """torch.randn / torch.randn_like hand out the pre-drawn tensors, in order"""
    it = iter(noises)
    monkeypatch.setattr(torch, "randn_like", lambda ref, **kw: next(it).to(device=ref.device, dtype=ref.dtype))
    monkeypatch.setattr(torch, "randn", lambda *size, device=None, dtype=None, **kw: next(it).to(device=device, dtype=dtype or torch.float32))


LOOP_CASES = [(s, strength, 1, 0.0) for s in FLOW + GAUSSIAN for strength in (0.5, 1.0)]
LOOP_CASES += [(s, 1.0, 1, 2.0) for s in FLOW + GAUSSIAN] + [(s, 1.0, 2, 0.0) for s in FLOW + GAUSSIAN]


@pytest.mark.parametrize("sampler,strength,resample,guidance", LOOP_CASES)
def test_loops_against_the_restatement(sampler, strength, resample, guidance, monkeypatch):
    init, mask, noises = loop_inputs()
    ref64 = restate(sampler, init, noises, mask, strength, resample, guidance, torch.float64)
    ref32 = restate(sampler, init, noises, mask, strength, resample, guidance, torch.float32)
    assert ref32["x"].dtype == torch.float32
    want = torch.stack(ref64["xt"], dim=1)
    dist = max(float((torch.stack(ref32["xt"], dim=1).double() - want).abs().max()), float((ref32["x"].double() - ref64["x"]).abs().max()))
    assert dist > 0.0

    model = ic.Mixer().to(DEV)
    d = diffuser(sampler, model)
    hand_out(monkeypatch, noises)
    out = d.generate({}, data_shape=SHAPE, use_tqdm=False, guidance_scale=guidance, init_image=init.to(DEV), strength=strength,
                     mask=mask.to(DEV), resample=resample, return_intermediates=True,
                     sampler_args={"eta": DDIM_ETA} if sampler == "ddim" else {})
    k = ic.strength_steps(STEPS, strength)
    assert out["xt"].shape == (SHAPE[0], k + 1) + SHAPE[1:] and out["estimated_x0"].shape == (SHAPE[0], k) + SHAPE[1:]
    got = max(float((out["xt"].double().cpu() - want).abs().max()), float((out["x"].double().cpu() - ref64["x"]).abs().max()))
    print(f"\n{sampler} strength {strength} resample {resample} guidance {guidance}: max|x| {float(want.abs().max()):.3e}  "
          f"f32 restatement vs f64 {dist:.3e}  product vs f64 {got:.3e}  tolerance {4 * dist:.3e}")
    assert got <= 4 * dist, (got, dist)
    # properties of the product path
    keep = (mask <= 0).expand(SHAPE)
    x = out["x"].cpu()
    assert torch.equal(bits(x[keep]), bits(init[keep])) and torch.equal(bits(out["xt"][:, -1]), bits(out["x"]))
    assert not torch.equal(x[~keep], init[~keep])
    assert model.calls == ic.n_model_calls(STEPS, strength, resample, guidance > 0)


@pytest.mark.parametrize("sampler", FLOW)
def test_flow_from_an_image_at_full_strength_without_a_mask_is_the_plain_call(sampler):
    init, _, noises = loop_inputs()
    eps0 = noises[0].to(DEV)
    d = diffuser(sampler, ic.Mixer().to(DEV))
    torch.manual_seed(3)
    plain = d.generate({"x": eps0.clone()}, use_tqdm=False)["x"]
    torch.manual_seed(3)
    img = d.generate({"x": eps0.clone()}, use_tqdm=False, init_image=init.to(DEV), strength=1.0)["x"]
    assert torch.equal(bits(plain), bits(img))


@pytest.mark.parametrize("sampler", FLOW + GAUSSIAN)
def test_a_plain_call_stays_on_its_path(sampler, ops, monkeypatch):
    def never(*a, **k):
        raise AssertionError("ops.inpaint_blend was called by a plain generate")

    monkeypatch.setattr(ops, "inpaint_blend", never)
    model = ic.Mixer().to(DEV)
    d = diffuser(sampler, model)
    outs = []
    for _ in range(2):
        torch.manual_seed(5)
        outs.append(d.generate({}, data_shape=SHAPE, use_tqdm=False, return_intermediates=True))
    assert set(outs[0]) == set(outs[1]) and all(torch.equal(bits(outs[0][k_]), bits(outs[1][k_])) for k_ in outs[0])
    assert outs[0]["xt"].shape[1] == STEPS + 1 and model.calls == 2 * STEPS
    # ... and is the loop the sampler's own steps make from the same draws
    torch.manual_seed(5)
    x = torch.randn(SHAPE, device=DEV, dtype=torch.float32)
    with torch.no_grad():
        if sampler in FLOW:
            for t_curr, t_prev in zip(d.diffusion.timesteps[:-1], d.diffusion.timesteps[1:]):
                x = d.diffusion.one_step_denoise(model, {"x": x}, t_curr=t_curr, t_prev=t_prev, guidance_scale=0)["x_prev"]
        else:
            for t in range(STEPS - 1, -1, -1):
                x = d.diffusion.one_step_denoise(model, {"x": x}, t=t)["x_prev"]
    assert torch.equal(bits(x), bits(outs[0]["x"]))


# ------------------------------------------------------------------------------------------------------------------ end to end
def _unet(out_channels):  # the smallest shapes the engines accept, as tests/test_learned_variance_gpu.py sizes them
    from diffulab_amd.networks.denoisers import UNetModel

    return UNetModel(image_size=[16, 16], in_channels=1, model_channels=32, out_channels=out_channels, num_res_blocks=1,
                     attention_resolutions=[2], channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True,
                     n_classes=10, classifier_free=True)


def _dit(output_channels):
    from diffulab_amd import MMDiT

    return MMDiT(simple_dit=True, input_channels=4, output_channels=output_channels, inner_dim=128, embedding_dim=64, num_heads=2,
                 mlp_ratio=4, patch_size=2, depth=2, n_classes=10, classifier_free=True)


def _engines():
    return {"unet": (_unet, 1, "out.2.weight", "ddpm", "gaussian_diffusion", 1000),
            "dit": (_dit, 4, "last_layer.linear.weight", "euler", "rectified_flow", 4)}


@pytest.mark.parametrize("family", ["unet", "dit"])
def test_end_to_end_on_the_real_engines(family):
    from diffulab_amd import Diffuser

    torch.manual_seed(0)
    make, C, head, sampler, model_type, n_steps = _engines()[family]
    m = make(C)
    with torch.no_grad():  # the output heads start at zero
        dict(m.named_parameters())[head].normal_(std=0.02)
    m = m.to(DEV).eval()
    assert m.precision == "bf16"
    d = Diffuser(m, sampling_method=sampler, model_type=model_type, n_steps=n_steps)
    d.set_steps(4)
    B = 4
    init = synth.uniform(f"ice.{family}", (B, C, 16, 16), lo=-1.0, hi=1.0).to(DEV)
    y = synth.integers("ice.y", (B,), 10).to(DEV)
    mask = torch.zeros(B, 1, 16, 16, device=DEV)
    mask[:, :, 4:12, 4:12] = 1.0  # fill a centre box
    keep = (mask <= 0).expand_as(init)
    for intermediates in (False, True):
        out = d.generate({"y": y}, use_tqdm=False, guidance_scale=2, init_image=init, mask=mask, strength=0.5,
                         return_intermediates=intermediates)
        x = out["x"]
        assert x.shape == init.shape and bool(torch.isfinite(x).all())
        assert torch.equal(bits(x[keep]), bits(init[keep])) and not torch.equal(x[~keep], init[~keep])
        if intermediates:
            k = ic.strength_steps(4, 0.5)
            assert k == 2 and out["xt"].shape == (B, k + 1, C, 16, 16) and out["estimated_x0"].shape == (B, k, C, 16, 16)
            assert bool(torch.isfinite(out["xt"]).all())
