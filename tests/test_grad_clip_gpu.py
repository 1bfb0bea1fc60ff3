"""GPU tests of gradient clipping by global norm: the fixed-order sum of squares and the f64 fold against float64 with write guards,
the fused AdamW update against the existing kernel bit for bit, ``FusedAdamW(max_grad_norm=...)``, the in-place
``clip_grad_norm_`` and the trainer.

The error bound is DERIVED, not tuned: the sum of squares adds non-negative f32 terms, the longest serial chain of additions has
``ops.grad_sumsq_chain(n)`` terms, every term is one rounded square, so the relative error of the sum is at most
``(chain + 2) * 2**-24`` (the workgroup sums are then folded in f64, which adds nothing at this scale), and half of that on the
norm (the square root halves a relative error; the ``+ 2`` covers the final rounding of the norm to f32)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import synth  # noqa: E402

from diffulab_amd import ops  # noqa: E402

DEV = "cuda"
U = 2.0**-24
GUARD = 8  # canary floats on either side of every buffer (8 floats keep the 16-byte phase of the allocation)
CANARY = 1234.5
F32 = np.float32


def sum_bound(n):
    return (ops.grad_sumsq_chain(n) + 2) * U


def torch_rule(norm_f32, max_norm):
    """clip_grad_norm_'s coefficient in f32 arithmetic on the f32 norm: clamp(max_norm / (norm + 1e-6), max=1)"""
    with np.errstate(all="ignore"):
        c = F32(max_norm) / (F32(norm_f32) + F32(1e-6))
    return c if np.isnan(c) else min(c, F32(1.0))


class Guarded:
    """an f32 device buffer of n floats starting `phase` floats past a 16-byte boundary, with canaries on both sides"""

    def __init__(self, n, phase=0, fill=CANARY):
        self.base = torch.full((GUARD + phase + n + GUARD,), CANARY, device=DEV)
        assert self.base.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + phase, GUARD + phase + n
        self.view = self.base[self.lo : self.hi]
        self.view.fill_(fill)
        assert (self.view.data_ptr() % 16) // 4 == phase % 4

    def snapshot(self):
        self.saved = self.base.clone()

    def intact_outside(self, lo=0, hi=0):
        """bit-unchanged since snapshot() except view[lo:hi]"""
        a, b = self.base.view(torch.int32), self.saved.view(torch.int32)
        return torch.equal(a[: self.lo + lo], b[: self.lo + lo]) and torch.equal(a[self.lo + hi :], b[self.lo + hi :])


def run_norm(x: Guarded, max_norm, grad_scale=1.0, slot=3, spare=5):
    """grad_sumsq + clip_coef on guarded buffers; checks every write guard; -> (f64 sum of the written slots, norm, coef) on the host"""
    n = x.view.numel()
    k_expect = ops.grad_sumsq_slots(n)
    part, out = Guarded(slot + k_expect + spare), Guarded(2)
    x.snapshot(), part.snapshot(), out.snapshot()
    k = ops.grad_sumsq(x.view, part.view, slot)
    assert k == k_expect
    ops.clip_coef(part.view[slot:], k, max_norm, out.view, grad_scale)
    torch.cuda.synchronize()
    assert x.intact_outside(), "the sum of squares wrote to the gradient buffer or its guards"
    assert part.intact_outside(slot, slot + k), "a partial was written outside the slots the call reported"
    assert out.intact_outside(0, 2), "the {norm, coef} pair overran"
    slots = part.view[slot : slot + k].double().cpu()
    norm, coef = out.view.cpu().numpy()
    return slots.sum().item(), norm, coef, part.view[slot : slot + k].clone(), out.view.clone()


CASES = [(1, 0), (3, 0), (63, 0), (257, 0), (64 * 1024 + 3, 0), (3_000_001, 0),
         (64 * 1024 + 3, 1), (64 * 1024 + 3, 2), (64 * 1024 + 3, 3),
         (1, 1), (3, 2), (257, 3), (3_000_001, 1)]  # (head longer than the buffer, head + tail without a body vector, ...)


@pytest.mark.parametrize("n,phase", CASES)
def test_sumsq_and_coef_against_float64_with_write_guards(n, phase):
    x = Guarded(n, phase)
    x.view.copy_(synth.normal(f"clip.x{n}", (n,)).to(DEV) if n < 100_000 else
                 torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(n)))
    ref = (x.view.double().cpu() ** 2).sum().item()
    ref_norm = ref**0.5
    # standard normal: one bound that clips, one that does not
    for max_norm, gs in ((0.5 * ref_norm, 1.0), (2.0 * ref_norm, 1.0), (0.125 * ref_norm, 0.5)):
        s, norm, coef, _, _ = run_norm(x, max_norm, gs)
        print(f"n={n} phase={phase}: sum rel err {abs(s - ref) / ref:.3e} (bound {sum_bound(n):.3e}), "
              f"norm rel err {abs(norm - gs * ref_norm) / (gs * ref_norm):.3e}")
        assert abs(s - ref) <= sum_bound(n) * ref
        assert abs(float(norm) - gs * ref_norm) <= 0.5 * sum_bound(n) * gs * ref_norm
        assert coef == torch_rule(norm, max_norm), (coef, torch_rule(norm, max_norm))
        assert (coef < 1) == (max_norm < gs * ref_norm)
    # all zeros: norm 0, nothing to clip
    x.view.zero_()
    s, norm, coef, _, _ = run_norm(x, 1.0)
    assert s == 0 and norm == 0 and coef == 1.0
    # one huge element among ones.  1e18 squares to 1e36, which f32 still holds (its largest finite value is 3.4e38): the norm is
    # finite and the tiny coefficient follows torch's rule; 1e20 squares to inf in f32, as in torch on the same f32 tensor, so the
    # norm is inf and the coefficient exactly 0
    for big in (1e18, 1e20):
        x.view.fill_(1.0)
        x.view[n // 2] = big
        s, norm, coef, _, _ = run_norm(x, 1.0)
        t_norm = torch.linalg.vector_norm(x.view)  # (what clip_grad_norm_ computes for a single f32 tensor)
        t_coef = torch.clamp(1.0 / (t_norm + 1e-6), max=1.0).item()
        if big == 1e18:
            want = ((x.view.double().cpu() ** 2).sum().item()) ** 0.5
            assert np.isfinite(norm) and abs(float(norm) - want) <= 0.5 * sum_bound(n) * want
            assert coef == torch_rule(norm, 1.0) and 0 < coef < 1e-17 and abs(coef - t_coef) <= 4 * sum_bound(n) * t_coef
        else:
            # (torch.linalg.vector_norm returns |x| for a one-element tensor without squaring it, so its norm stays finite there;
            # wherever torch's own f32 accumulation overflows it ends at the same coefficient)
            assert np.isinf(norm) and coef == 0.0
            assert n == 1 or (torch.isinf(t_norm) and t_coef == 0.0), (t_norm, t_coef)
    # one NaN: the norm and the coefficient are NaN (not special-cased, as with error_if_nonfinite=False)
    x.view.fill_(1.0)
    x.view[n - 1] = float("nan")
    s, norm, coef, _, _ = run_norm(x, 1.0)
    assert np.isnan(norm) and np.isnan(coef)


def test_chain_length_stays_below_4096_terms():
    """host arithmetic only: the 2^31 - 1 case is NOT run on the device (an 8 GiB buffer has no place in a quick suite); what the
    device test above pins is that the kernel's partition is the one this arithmetic describes (slots written == slots predicted)"""
    for n in (1, 2**20, 2**28, 2**31 - 1):
        assert ops.grad_sumsq_chain(n) <= 4096, n


def test_norm_is_bit_reproducible():
    n = 3_000_001
    x = Guarded(n)
    x.view.copy_(torch.randn(n, device=DEV, generator=torch.Generator(DEV).manual_seed(7)))
    a, b = run_norm(x, 1.0), run_norm(x, 1.0)
    assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32)) and torch.equal(a[4].view(torch.int32), b[4].view(torch.int32))
    assert ops.grad_sumsq_slots(n) == 512 and ops.grad_sumsq_chain(n) == 15  # (more than one grid pass)


@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_scale_inplace_with_write_guards(phase):
    n = 64 * 1024 + 3
    for m in (n, 2, 5):
        g = Guarded(m, phase)
        g.view.copy_(synth.normal("clip.scale", (n,))[:m].to(DEV))
        want = g.view * torch.tensor(0.37, device=DEV)
        g.snapshot()
        ops.scale_inplace(g.view, torch.tensor([0.37], device=DEV))
        assert g.intact_outside(0, m) and torch.equal(g.view.view(torch.int32), want.view(torch.int32))
        g.snapshot()
        ops.scale_inplace(g.view, torch.tensor([1.0], device=DEV))
        assert g.intact_outside()


# ---------------------------------------------------------------- the fused update against the existing kernel
HYP = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2)
STEP = 3


def _adam_state(n):
    p, g, m = (synth.normal(f"clip.adam.{k}", (n,)).to(DEV) for k in "pgm")
    v = synth.normal("clip.adam.v", (n,)).to(DEV).square() * 1e-2
    return p, g, m, v


def _bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_clipped_update_equals_the_existing_kernel_bit_for_bit(coef, grad_scale):
    """adamw_step_clip(grad_scale, device coef) == adamw_step(float32(grad_scale * coef)): no tolerance, the existing kernel has its
    own parity tests.  Same for the variants that read their scalars from a device buffer."""
    n = 64 * 1024 + 3
    p, g, m, v = _adam_state(n)
    fused = float(F32(grad_scale) * F32(coef))
    cdev = Guarded(1, fill=coef)
    cdev.snapshot()
    g0 = g.clone()
    a, b = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
    ops.adamw_step_clip(a[0], g, a[1], a[2], HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], HYP["wd"], STEP, cdev.view, grad_scale)
    ops.adamw_step(b[0], g, b[1], b[2], HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], HYP["wd"], STEP, fused)
    assert _bits_equal(a, b) and not torch.equal(a[0], p)
    assert torch.equal(g, g0) and cdev.intact_outside()
    if coef == 1.0:  # *coef == 1: the plain update with the caller's grad_scale itself
        c = [t.clone() for t in (p, m, v)]
        ops.adamw_step(c[0], g, c[1], c[2], HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], HYP["wd"], STEP, grad_scale)
        assert _bits_equal(a, c)

    def hyper(gs):
        bc1, bc2 = 1.0 - HYP["beta1"] ** STEP, 1.0 - HYP["beta2"] ** STEP
        return torch.tensor([HYP["lr"], HYP["beta1"], HYP["beta2"], HYP["eps"], HYP["wd"], HYP["lr"] / bc1, bc2**-0.5, gs],
                            dtype=torch.float32, device=DEV)

    a, b = [t.clone() for t in (p, m, v)], [t.clone() for t in (p, m, v)]
    ops.adamw_step_dev_clip(a[0], g, a[1], a[2], hyper(grad_scale), cdev.view)
    ops.adamw_step_dev(b[0], g, b[1], b[2], hyper(fused))
    assert _bits_equal(a, b) and not torch.equal(a[0], p)
    assert torch.equal(g, g0) and cdev.intact_outside()


# ---------------------------------------------------------------- FusedAdamW / clip_grad_norm_ / trainer on the smallest DiT
SMALL = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4,
             patch_size=2, depth=1, n_classes=10, classifier_free=True)


def small_dit(seed=5):
    from diffulab_amd import MMDiT
    from oracle import dit as odit

    m = MMDiT(simple_dit=True, **SMALL)
    m.load_state_dict(synth.dit_params(odit.param_shapes(odit.DiTConfig(**SMALL)), seed=seed))
    return m.to(DEV)


class Bench:
    """the DiT (64 tokens, B = 2) after ONE forward and backward, plus a loose tensor with a gradient outside the arena (the shape
    of the REPA projector's tensors sharing the denoiser's parameter group).  `step(make)` restores the initial parameters, steps
    a fresh optimizer on the SAME gradients (the fused path never rewrites them) and returns the new parameters."""

    def __init__(self):
        from diffulab_amd import Diffuser

        self.model = small_dit()
        d = Diffuser(self.model, sampling_method="euler", model_type="rectified_flow", n_steps=4)
        B = 2
        x0, noise = synth.normal("clip.x0", (B, 4, 16, 16)).to(DEV), synth.normal("clip.noise", (B, 4, 16, 16)).to(DEV)
        y, t = synth.integers("clip.y", (B,), 10).to(DEV), synth.uniform("clip.t", (B,), lo=0.05, hi=0.95)
        d.compute_loss({"x": x0, "y": y, "p": 0.0}, timesteps=t, noise=noise)["loss"].backward()
        self.loose = torch.nn.Parameter(synth.normal("clip.loose", (37, 5)).to(DEV))
        self.loose.grad = synth.normal("clip.loose.grad", (37, 5)).to(DEV) * 0.1
        self.params = [p for p in self.model.parameters() if p.grad is not None] + [self.loose]
        self.init = [p.detach().clone() for p in self.params]
        self.grads = [p.grad.detach().clone() for p in self.params]
        self.norm64 = sum((g.double() ** 2).sum() for g in self.grads).sqrt().item()
        # the same number from torch's own function on f64 copies (one global norm over the arena AND the loose tensor)
        copies = [torch.nn.Parameter(p.detach().double()) for p in self.params]
        for c, g in zip(copies, self.grads):
            c.grad = g.double()
        self.torch_norm = torch.nn.utils.clip_grad_norm_(copies, 1e30).item()
        assert abs(self.torch_norm - self.norm64) <= 1e-12 * self.norm64
        assert (self.loose.grad.double() ** 2).sum().item() > 1e-4 * self.norm64**2, "the loose tensor must matter to the norm"
        self.bound = 0.5 * (max(ops.grad_sumsq_chain(self.model._flat_grad.numel()), ops.grad_sumsq_chain(self.loose.numel())) + 2) * U

    def restore(self):
        with torch.no_grad():
            for p, w, g in zip(self.params, self.init, self.grads):
                p.copy_(w)
                p.grad.copy_(g)

    def step(self, grad_scale=1.0, **kw):
        from diffulab_amd.training import FusedAdamW

        self.restore()
        opt = FusedAdamW(self.params, lr=1e-3, **kw)
        opt.grad_scale = grad_scale
        opt.step()
        assert all(torch.equal(p.grad, g) for p, g in zip(self.params, self.grads)), "step() rewrote a gradient"
        return opt, [p.detach().clone() for p in self.params]


@pytest.fixture(scope="module")
def bench():
    return Bench()


def test_fused_adamw_clips_by_one_global_norm(bench):
    mx = 0.5 * bench.norm64
    opt, clipped = bench.step(max_grad_norm=mx)
    norm, coef = opt._clip_out.cpu().numpy()
    assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.is_cuda and opt.last_grad_norm.item() == norm
    print(f"norm rel err {abs(norm - bench.norm64) / bench.norm64:.3e} (bound {bench.bound:.3e}), coef {coef}")
    assert abs(float(norm) - bench.torch_norm) <= bench.bound * bench.torch_norm
    assert coef < 1 and coef == torch_rule(norm, mx) and abs(coef - 0.5) < 1e-3
    _, manual = bench.step(grad_scale=float(coef))  # the existing update with the coefficient as its gradient scale
    assert _bits_equal(clipped, manual)
    # a bound that does not clip: the plain update, bit for bit
    opt, loose_bound = bench.step(max_grad_norm=1e9)
    assert opt._clip_out[1].item() == 1.0
    _, plain = bench.step()
    assert _bits_equal(loose_bound, plain) and not _bits_equal(plain, clipped)
    # data parallel, world 2: grad_scale = 0.5 halves the reported norm and the clip follows
    opt, dp = bench.step(grad_scale=0.5, max_grad_norm=0.25 * bench.norm64)
    norm2, coef2 = opt._clip_out.cpu().numpy()
    assert abs(float(norm2) - 0.5 * bench.torch_norm) <= bench.bound * 0.5 * bench.torch_norm
    assert coef2 == torch_rule(norm2, 0.25 * bench.norm64) and abs(coef2 - 0.5) < 1e-3
    _, manual = bench.step(grad_scale=float(F32(0.5) * coef2))
    assert _bits_equal(dp, manual)


def test_fused_adamw_default_issues_todays_launches(bench, monkeypatch):
    calls = []
    for name in ("grad_sumsq", "clip_coef", "adamw_step_clip", "adamw_step_dev_clip", "scale_inplace", "adamw_step"):
        monkeypatch.setattr(ops, name, (lambda f, nm: lambda *a, **k: (calls.append(nm), f(*a, **k))[1])(getattr(ops, name), name))
    bench.step()
    assert calls == ["adamw_step", "adamw_step"]  # the arena, the loose tensor
    del calls[:]
    bench.step(max_grad_norm=1.0)
    assert calls == ["grad_sumsq", "grad_sumsq", "clip_coef", "adamw_step_clip", "adamw_step_clip"]


def test_fused_adamw_clips_in_graph_mode(bench):
    """the device-scalar update (what a captured step replays): the clipped step equals the unclipped one whose hyper buffer
    carries float32(grad_scale * coef), bit for bit, and the clip buffers keep their addresses across begin_graph_mode calls"""
    mx = 0.5 * bench.norm64
    opt_a, _ = bench.step(max_grad_norm=mx)  # (one eager step creates the moments: identical in both, by the test above)
    coef = opt_a._clip_out[1].item()
    opt_b, _ = bench.step(grad_scale=coef)
    addr = (opt_a._clip_partials.data_ptr(), opt_a._clip_out.data_ptr())
    outs = []
    for o, gs in ((opt_a, 1.0), (opt_b, coef)):
        bench.restore()
        o.grad_scale = gs
        o.begin_graph_mode()
        o.advance()
        o.step()
        o.end_graph_mode()
        outs.append([p.detach().clone() for p in bench.params])
    assert opt_a._clip_out[1].item() == coef and (opt_a._clip_partials.data_ptr(), opt_a._clip_out.data_ptr()) == addr
    assert _bits_equal(outs[0], outs[1]) and not _bits_equal(outs[0], bench.init)
    assert all(torch.equal(p.grad, g) for p, g in zip(bench.params, bench.grads))


def test_clip_grad_norm_in_place(bench):
    from diffulab_amd.training.utils import clip_grad_norm_

    bench.restore()
    mx = 0.5 * bench.norm64
    norm = clip_grad_norm_(bench.params, mx)
    assert norm.is_cuda and norm.dim() == 0
    assert abs(norm.item() - bench.torch_norm) <= bench.bound * bench.torch_norm
    coef = torch.tensor(float(torch_rule(F32(norm.item()), mx)), device=DEV)
    assert coef.item() < 1
    for p, g in zip(bench.params, bench.grads):
        assert torch.equal(p.grad.view(torch.int32), (g * coef).view(torch.int32))
    scaled = [p.grad.clone() for p in bench.params]
    norm2 = clip_grad_norm_(bench.params, 1e9)
    assert abs(norm2.item() - coef.item() * bench.torch_norm) <= 2 * bench.bound * bench.torch_norm
    assert _bits_equal([p.grad for p in bench.params], scaled)
    # two views of an arena they do not fill: taken tensor by tensor, nothing else in the arena is touched
    bench.restore()
    two = list({id(p): p for p in [q for q in bench.params[:-1] if q.grad.storage_offset() % 4][:1] + bench.params[:2]}.values())[:2]
    want = sum((p.grad.double() ** 2).sum() for p in two).sqrt().item()
    norm3 = clip_grad_norm_(two, 0.25 * want, grad_scale=0.5)
    assert abs(norm3.item() - 0.5 * want) <= bench.bound * 0.5 * want
    c3 = torch.tensor(float(torch_rule(F32(norm3.item()), 0.25 * want)), device=DEV)
    ids = {id(p) for p in two}
    for p, g in zip(bench.params, bench.grads):
        assert torch.equal(p.grad.view(torch.int32), ((g * c3) if id(p) in ids else g).view(torch.int32))
    bench.restore()


def test_trainer_clips_once_per_accumulation_window(tmp_path, monkeypatch):
    """two micro-steps of a k = 2 window: ONE norm computation, `train/grad_norm` in the meter, and the parameters after the window
    are, bit for bit, those of FusedAdamW(max_grad_norm) stepped by hand on the gradient the trainer's optimizer saw.  (The gradient
    is captured at step() rather than recomputed by a second pair of backwards: the weight-gradient reductions of the engine use f32
    atomics, so two backward passes agree to ~1e-3, not bit for bit -- tests/test_trainer_gpu.py pins that side.)"""
    from diffulab_amd import Diffuser
    from diffulab_amd.training import BaseTrainer, FusedAdamW
    from diffulab_amd.training.utils import AverageMeter

    def run(max_grad_norm):
        m = small_dit()
        d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=4)
        opt = FusedAdamW(m.parameters(), lr=1e-3)
        tr = BaseTrainer(n_epoch=1, gradient_accumulation_step=2, save_path=tmp_path, project_name=f"clip{max_grad_norm}",
                         max_grad_norm=max_grad_norm)
        counts = {"grad_sumsq": 0, "clip_coef": 0}
        for name in counts:
            monkeypatch.setattr(ops, name, (lambda f, nm: lambda *a, **k: (counts.__setitem__(nm, counts[nm] + 1), f(*a, **k))[1])(
                getattr(ops, name), name))
        seen = []
        orig_step = opt.step
        opt.step = lambda *a, **k: (seen.append((m._flat.clone(), m._flat_grad.clone())), orig_step(*a, **k))[1]
        meter = AverageMeter()
        torch.manual_seed(3)
        for i in range(2):
            batch = {"model_inputs": {"x": synth.normal(f"clip.tr.x{i}", (2, 4, 16, 16)), "y": synth.integers(f"clip.tr.y{i}", (2,), 10)}}
            tr.training_step(d, opt, batch, meter, p_classifier_free_guidance=0.1)
            if i == 0:
                assert not seen and sum(counts.values()) == 0, "nothing happens on the non-synchronising micro-step"
        monkeypatch.undo()
        assert len(seen) == 1
        return m, opt, meter, counts, seen[0]

    m, opt, meter, counts, (w0, g0) = run(None)
    assert counts == {"grad_sumsq": 0, "clip_coef": 0} and "train/grad_norm" not in meter.keys and opt.max_grad_norm is None
    norm64 = (g0.double() ** 2).sum().sqrt().item()
    mx = 0.5 * norm64  # (the same inputs and seed give the same gradient up to the atomics' reordering: this bound clips)
    m, opt, meter, counts, (w0, g0) = run(mx)
    assert counts == {"grad_sumsq": 1, "clip_coef": 1}
    assert opt.max_grad_norm == mx and opt._clip_out[1].item() < 1
    norm64 = (g0.double() ** 2).sum().sqrt().item()
    logged = meter.avg["train/grad_norm"]
    assert meter.count["train/grad_norm"] == 1
    assert abs(logged - norm64) <= 0.5 * sum_bound(g0.numel()) * norm64
    after = m._flat.clone()
    with torch.no_grad():
        m._flat.copy_(w0)
        m._flat_grad.copy_(g0)
    manual = FusedAdamW(m.parameters(), lr=1e-3, max_grad_norm=mx)
    manual.step()
    assert torch.equal(m._flat.view(torch.int32), after.view(torch.int32)) and not torch.equal(after, w0)


def test_trainer_clips_in_place_for_another_optimizer(tmp_path, monkeypatch):
    """configs/optimizer/sgd.yaml: torch.optim.SGD gets its gradients scaled in place before step(), once per window"""
    from diffulab_amd import Diffuser
    from diffulab_amd.training import BaseTrainer
    from diffulab_amd.training.utils import AverageMeter

    m = small_dit()
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=4)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    tr = BaseTrainer(n_epoch=1, gradient_accumulation_step=2, save_path=tmp_path, project_name="sgd", max_grad_norm=1e-3)
    calls = []
    for name in ("grad_sumsq", "clip_coef", "scale_inplace"):
        monkeypatch.setattr(ops, name, (lambda f, nm: lambda *a, **k: (calls.append(nm), f(*a, **k))[1])(getattr(ops, name), name))
    seen = []
    orig_step = opt.step
    opt.step = lambda *a, **k: (seen.append(m._flat_grad.clone()), orig_step(*a, **k))[1]
    meter = AverageMeter()
    torch.manual_seed(3)
    for i in range(2):
        batch = {"model_inputs": {"x": synth.normal(f"clip.tr.x{i}", (2, 4, 16, 16)), "y": synth.integers(f"clip.tr.y{i}", (2,), 10)}}
        tr.training_step(d, opt, batch, meter, p_classifier_free_guidance=0.1)
    assert calls == ["grad_sumsq", "clip_coef", "scale_inplace"] and len(seen) == 1
    clipped_norm = (seen[0].double() ** 2).sum().sqrt().item()
    assert abs(clipped_norm - 1e-3) <= 1e-5 * 1e-3 + 1e-6 * 1e-3 / meter.avg["train/grad_norm"]  # |g| * max / (|g| + 1e-6)
    assert meter.avg["train/grad_norm"] > 1e-3
