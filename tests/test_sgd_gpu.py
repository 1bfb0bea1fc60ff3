"""GPU tests of the fused SGD: the `dl_sgd_step` kernel against ``torch.optim.SGD`` on the CPU, its write guards at every 16-byte
phase, the bit identities between its forms (plain / clipped, scalars from the launch / from device memory, vector / scalar path),
``FusedSGD`` on the smallest DiT (parity, launches, clipping, graph mode, checkpoints), the trainer and the UNet.

The parity measure and bar are those of test_adamw_and_casts: ``max|p - p_ref| / max|p_ref| < 1e-6``.  torch's own f32 run on the
CPU is within 1.4e-7 of its f64 run on the kernel test's inputs and settings (lr 0.05, five steps), so two correct f32
implementations stay far inside the bar."""

import copy

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
BAR = 1e-6
LR = 0.05


def err(a, b):
    """max|a - b| / max|b| in f64 (both zero everywhere: 0)"""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    top = b.abs().max().item()
    d = (a - b).abs().max().item()
    return d / top if top > 0 else d


def bits_equal(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


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


# ---------------------------------------------------------------- the kernel against torch.optim.SGD on the CPU
HYPERS = {
    "plain": dict(momentum=0),
    "momentum_wd": dict(momentum=0.9, weight_decay=1e-4),
    "nesterov_wd": dict(momentum=0.9, nesterov=True, weight_decay=1e-4),
    "dampening_maximize": dict(momentum=0.9, dampening=0.1, maximize=True),
    "dampening_wd": dict(momentum=0.5, dampening=0.3, weight_decay=0.01),
}


def kernel_step(p, g, buf, h, first, lr=LR, grad_scale=1.0, coef=None):
    ops.sgd_step(p, g, buf, lr, h.get("momentum", 0), h.get("dampening", 0), h.get("weight_decay", 0), grad_scale, coef,
                 h.get("nesterov", False), first, h.get("maximize", False))


@pytest.mark.parametrize("name", list(HYPERS))
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 10007])
def test_kernel_against_torch_sgd_on_the_cpu(n, name):
    """five steps with grad = g * step; the parameters and the momentum buffer against torch's f32 run on the CPU"""
    h = HYPERS[name]
    p0, g = synth.normal(f"sgd.p{n}", (n,)), synth.normal(f"sgd.g{n}", (n,))
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([ref], lr=LR, **h)
    p = p0.to(DEV)
    buf = torch.full((n,), float("nan"), device=DEV) if h["momentum"] else None  # (the first step must not read it)
    for step in range(1, 6):
        gk = g * step
        ref.grad = gk.clone()
        opt.step()
        kernel_step(p, gk.to(DEV), buf, h, first=step == 1)
    e_p = err(p, ref)
    e_b = err(buf, opt.state[ref]["momentum_buffer"]) if buf is not None else 0.0
    print(f"n={n} {name}: p err {e_p:.3e}, buf err {e_b:.3e} (bar {BAR:.0e})")
    assert not torch.equal(p.cpu(), p0)
    assert e_p < BAR and e_b < BAR


# ---------------------------------------------------------------- write guards, every phase; vector path == scalar path
SIZES = [1, 3, 257, 64 * 1024 + 3]
PHASES = [(0, 0, 0), (1, 1, 1), (2, 2, 2), (3, 3, 3), (0, 1, 2), (1, 1, 3), (2, 0, 2)]  # (p, g, buf); the last three: scalar loop
H_GUARD = HYPERS["nesterov_wd"]


@pytest.fixture(scope="module")
def plain_results():
    """per n: the inputs and what the update gives on ordinary allocations (phase 0: the vector path), first step and a later one"""
    out = {}
    for n in SIZES:
        p, g, b = (synth.normal(f"sgd.guard.{k}{n}", (n,)).to(DEV) for k in "pgb")
        res = {}
        for first in (True, False):
            pp, bb = p.clone(), b.clone()
            kernel_step(pp, g, bb, H_GUARD, first)
            res[first] = (pp, bb)
        pp = p.clone()
        kernel_step(pp, g, None, HYPERS["plain"], False)
        out[n] = (p, g, b, res, pp)
    return out


@pytest.mark.parametrize("phases", PHASES)
@pytest.mark.parametrize("n", SIZES)
def test_write_guards_at_every_phase(plain_results, n, phases):
    p0, g0, b0, want, want_plain = plain_results[n]
    for first in (True, False):
        p, g, b = (Guarded(n, ph) for ph in phases)
        p.view.copy_(p0), g.view.copy_(g0), b.view.copy_(b0)
        p.snapshot(), g.snapshot(), b.snapshot()
        kernel_step(p.view, g.view, b.view, H_GUARD, first)
        torch.cuda.synchronize()
        assert p.intact_outside(0, n) and b.intact_outside(0, n), "the update wrote outside [0, n)"
        assert g.intact_outside(), "the update wrote to the gradient or its guards"
        assert bits_equal((p.view, b.view), want[first]), "the result depends on the buffers' phases (vector / scalar path)"
        assert not torch.equal(p.view, p0) and not torch.equal(b.view, b0)
    # momentum == 0: a buffer that is passed all the same is neither read nor written; without one the result is the same
    p, g, b = (Guarded(n, ph) for ph in phases)
    p.view.copy_(p0), g.view.copy_(g0), b.view.fill_(float("nan"))
    p.snapshot(), g.snapshot(), b.snapshot()
    kernel_step(p.view, g.view, b.view, HYPERS["plain"], False)
    torch.cuda.synchronize()
    assert p.intact_outside(0, n) and g.intact_outside() and b.intact_outside()
    assert bits_equal((p.view,), (want_plain,))


# ---------------------------------------------------------------- bit identities between the kernel's forms
def hyper_dev(h, gs, lr=LR):
    return torch.tensor([lr, h.get("momentum", 0), h.get("dampening", 0), h.get("weight_decay", 0), gs, 0, 0, 0], dtype=torch.float32,
                        device=DEV)


@pytest.mark.parametrize("name", ["plain", "nesterov_wd", "dampening_maximize", "dampening_wd"])
@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_forms_of_the_update_agree_bit_for_bit(name, coef, grad_scale):
    """sgd_step(grad_scale, device coef) == sgd_step(float32(grad_scale * coef)); sgd_step_dev == sgd_step on the same scalars"""
    h = HYPERS[name]
    n = 64 * 1024 + 3
    p, g, b = (synth.normal(f"sgd.forms.{k}", (n,)).to(DEV) for k in "pgb")
    mom = bool(h["momentum"])
    fused = float(F32(grad_scale) * F32(coef))
    cdev = Guarded(1, fill=coef)
    cdev.snapshot()
    g0 = g.clone()

    def run(fn):
        pp, bb = p.clone(), (b.clone() if mom else None)
        fn(pp, bb)
        return (pp, bb) if mom else (pp,)

    clipped = run(lambda pp, bb: kernel_step(pp, g, bb, h, False, grad_scale=grad_scale, coef=cdev.view))
    plain = run(lambda pp, bb: kernel_step(pp, g, bb, h, False, grad_scale=fused))
    assert bits_equal(clipped, plain) and not torch.equal(clipped[0], p)
    if coef == 1.0:  # *coef == 1: the plain update with the caller's grad_scale itself
        assert bits_equal(clipped, run(lambda pp, bb: kernel_step(pp, g, bb, h, False, grad_scale=grad_scale)))
    flags = dict(nesterov=h.get("nesterov", False), maximize=h.get("maximize", False))
    dev_clipped = run(lambda pp, bb: ops.sgd_step_dev(pp, g, bb, hyper_dev(h, grad_scale), cdev.view, **flags))
    dev_plain = run(lambda pp, bb: ops.sgd_step_dev(pp, g, bb, hyper_dev(h, fused), None, **flags))
    assert bits_equal(dev_clipped, plain) and bits_equal(dev_plain, plain)
    assert torch.equal(g, g0) and cdev.intact_outside()


# ---------------------------------------------------------------- FusedSGD on the smallest DiT
SMALL = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4,
             patch_size=2, depth=1, n_classes=10, classifier_free=True)
NESTEROV = dict(lr=LR, momentum=0.9, nesterov=True, weight_decay=1e-4)
NO_MOMENTUM = dict(lr=LR, momentum=0.0, weight_decay=1e-4)


def small_dit(seed=5):
    from diffulab_amd import MMDiT
    from oracle import dit as odit

    m = MMDiT(simple_dit=True, **SMALL)
    m.load_state_dict(synth.dit_params(odit.param_shapes(odit.DiTConfig(**SMALL)), seed=seed))
    return m.to(DEV)


class Bench:
    """the DiT (64 tokens, B = 2) after ONE forward and backward, plus a loose tensor with a gradient outside the arena.  The
    gradients stay fixed (the fused path never rewrites them): `run(k)` restores the initial parameters and takes k steps of a fresh
    FusedSGD on them; `torch_run(k)` does the same with torch.optim.SGD on CPU copies."""

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
        assert (self.loose.grad.double() ** 2).sum().item() > 1e-4 * self.norm64**2, "the loose tensor must matter to the norm"
        self.bound = 0.5 * (max(ops.grad_sumsq_chain(self.model._flat_grad.numel()), ops.grad_sumsq_chain(self.loose.numel())) + 2) * U
        self._torch_runs = {}

    def restore(self, weights=None):
        with torch.no_grad():
            for p, w, g in zip(self.params, weights or self.init, self.grads):
                p.copy_(w)
                p.grad.copy_(g)

    def snapshot(self):
        return [p.detach().clone() for p in self.params]

    def make(self, grad_scale=1.0, **kw):
        from diffulab_amd.training import FusedSGD

        opt = FusedSGD(self.params, **kw)
        opt.grad_scale = grad_scale
        return opt

    def run(self, steps=1, grad_scale=1.0, **kw):
        self.restore()
        opt = self.make(grad_scale, **kw)
        for _ in range(steps):
            opt.step()
        assert all(torch.equal(p.grad, g) for p, g in zip(self.params, self.grads)), "step() rewrote a gradient"
        return opt, self.snapshot()

    def torch_run(self, steps, **kw):
        """-> (the CPU parameters after `steps` steps of torch.optim.SGD, its state dict then); computed once per setting"""
        key = (steps, tuple(sorted(kw.items())))
        if key not in self._torch_runs:
            ps = [torch.nn.Parameter(w.cpu().clone()) for w in self.init]
            opt = torch.optim.SGD(ps, **kw)
            for _ in range(steps):
                for p, g in zip(ps, self.grads):
                    p.grad = g.cpu().clone()
                opt.step()
            self._torch_runs[key] = ([p.detach().clone() for p in ps], copy.deepcopy(opt.state_dict()))
        return self._torch_runs[key]


@pytest.fixture(scope="module")
def bench():
    return Bench()


def worst_err(got, want):
    return max(err(a, b) for a, b in zip(got, want))


@pytest.mark.parametrize("kw", [NESTEROV, NO_MOMENTUM], ids=["nesterov", "no_momentum"])
def test_fused_sgd_against_torch_sgd(bench, kw):
    opt, got = bench.run(3, **kw)
    want, _ = bench.torch_run(3, **kw)
    e = worst_err(got, want)
    print(f"three steps, {kw}: worst per-tensor err {e:.3e} (bar {BAR:.0e})")
    assert e < BAR and not bits_equal(got, bench.init)
    key = bench.params[0]
    if kw["momentum"]:
        assert set(opt.state[key]) == {"step", "buf"} and opt.state[key]["buf"].numel() == bench.model._flat.numel()
        assert set(opt.state[bench.loose]) == {"step", "buf"} and opt.state[key]["step"] == 3
        assert len(opt.state) == 2, "one arena entry and one per loose tensor"
    else:
        assert all("buf" not in st for st in opt.state.values())


def test_fused_sgd_issues_one_launch_per_arena_and_loose_tensor(bench, monkeypatch):
    calls = []
    for name in ("grad_sumsq", "clip_coef", "sgd_step", "sgd_step_dev", "scale_inplace", "adamw_step", "adamw_step_clip"):
        monkeypatch.setattr(ops, name, (lambda f, nm: lambda *a, **k: (calls.append(nm), f(*a, **k))[1])(getattr(ops, name), name))
    bench.run(2, **NESTEROV)
    assert calls == ["sgd_step", "sgd_step"] * 2  # the arena, the loose tensor
    del calls[:]
    bench.run(1, **NO_MOMENTUM)
    assert calls == ["sgd_step", "sgd_step"]
    del calls[:]
    bench.run(1, max_grad_norm=1.0, **NESTEROV)
    assert calls == ["grad_sumsq", "grad_sumsq", "clip_coef", "sgd_step", "sgd_step"]


def test_fused_sgd_clips_by_one_global_norm(bench):
    mx = 0.5 * bench.norm64
    opt, clipped = bench.run(max_grad_norm=mx, **NESTEROV)
    norm, coef = opt._clip_out.cpu().numpy()
    assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.is_cuda and opt.last_grad_norm.item() == norm
    print(f"norm rel err {abs(norm - bench.norm64) / bench.norm64:.3e} (bound {bench.bound:.3e}), coef {coef}")
    assert abs(float(norm) - bench.norm64) <= bench.bound * bench.norm64
    assert coef < 1 and coef == torch_rule(norm, mx) and abs(coef - 0.5) < 1e-3
    _, manual = bench.run(grad_scale=float(coef), **NESTEROV)  # the unclipped update with the coefficient as its gradient scale
    assert bits_equal(clipped, manual)
    # a bound that does not clip: the plain update, bit for bit
    opt, loose_bound = bench.run(max_grad_norm=1e9, **NESTEROV)
    assert opt._clip_out[1].item() == 1.0
    _, plain = bench.run(**NESTEROV)
    assert bits_equal(loose_bound, plain) and not bits_equal(plain, clipped)
    # data parallel, world 2: grad_scale = 0.5 halves the reported norm and the clip follows
    opt, dp = bench.run(grad_scale=0.5, max_grad_norm=0.25 * bench.norm64, **NESTEROV)
    norm2, coef2 = opt._clip_out.cpu().numpy()
    assert abs(float(norm2) - 0.5 * bench.norm64) <= bench.bound * 0.5 * bench.norm64
    assert coef2 == torch_rule(norm2, 0.25 * bench.norm64) and abs(coef2 - 0.5) < 1e-3
    _, manual = bench.run(grad_scale=float(F32(0.5) * coef2), **NESTEROV)
    assert bits_equal(dp, manual)


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip_world2"])
@pytest.mark.parametrize("kw", [NESTEROV, NO_MOMENTUM], ids=["nesterov", "no_momentum"])
def test_fused_sgd_graph_mode_equals_the_eager_second_step(bench, kw, clip):
    """the device-scalar update (what a captured step replays) after one eager step == the second eager step, bit for bit"""
    extra = dict(grad_scale=0.5, max_grad_norm=0.25 * bench.norm64) if clip else {}
    _, eager = bench.run(2, **kw, **extra)
    opt, first = bench.run(1, **kw, **extra)
    calls = []
    orig = ops.sgd_step_dev
    ops.sgd_step_dev = lambda *a, **k: (calls.append("sgd_step_dev"), orig(*a, **k))[1]
    try:
        opt.begin_graph_mode()
        assert opt.in_graph_mode()
        opt.advance()
        opt.step()
        opt.end_graph_mode()
    finally:
        ops.sgd_step_dev = orig
    assert calls == ["sgd_step_dev"] * 2 and not opt.in_graph_mode()
    assert bits_equal(bench.snapshot(), eager) and not bits_equal(eager, first)
    assert opt.state[bench.params[0]]["step"] == 2
    assert all(torch.equal(p.grad, g) for p, g in zip(bench.params, bench.grads))
    if clip:
        assert opt._clip_out[1].item() < 1
    if kw["momentum"]:  # a fresh optimizer has no momentum buffer yet: graph mode refuses instead of reading one
        fresh = bench.make(**kw)
        fresh.begin_graph_mode()
        fresh.advance()
        with pytest.raises(RuntimeError, match="eager step"):
            fresh.step()


def test_fused_sgd_resumes_from_a_torch_sgd_checkpoint(bench):
    (after2, sd), (after3, _) = bench.torch_run(2, **NESTEROV), bench.torch_run(3, **NESTEROV)
    bench.restore([w.to(DEV) for w in after2])
    opt = bench.make(lr=123.0)  # (the checkpoint's param_groups replace the constructor's)
    opt.load_state_dict(copy.deepcopy(sd))
    opt.step()
    e = worst_err(bench.snapshot(), after3)
    print(f"third step after a torch.optim.SGD checkpoint: worst per-tensor err {e:.3e}")
    assert e < BAR and worst_err(after2, after3) > 1e-4
    assert set(opt.state[bench.params[0]]) == {"step", "buf"} and len(opt.state) == 2  # packed: one arena buffer, one loose
    assert not any("momentum_buffer" in st for st in opt.state.values())
    # a checkpoint taken before torch's first step (no buffers): the first step, which copies the gradient
    _, sd0 = bench.torch_run(0, **NESTEROV)
    bench.restore()
    opt = bench.make(lr=123.0)
    opt.load_state_dict(copy.deepcopy(sd0))
    opt.step()
    assert worst_err(bench.snapshot(), bench.torch_run(1, **NESTEROV)[0]) < BAR
    # an arena parameter with a buffer beside one without
    bad = copy.deepcopy(sd)
    del bad["state"][1]
    bad["state"][2]["momentum_buffer"] = None
    bench.restore()
    opt = bench.make(lr=123.0)
    opt.load_state_dict(bad)
    with pytest.raises(RuntimeError, match=r"momentum_buffer.*positions \[1, 2\]"):
        opt.step()
    bench.restore()


def test_fused_sgd_resumes_from_its_own_state_dict(bench):
    _, straight = bench.run(3, **NESTEROV)
    opt, after2 = bench.run(2, **NESTEROV)
    sd = copy.deepcopy(opt.state_dict())
    assert len(sd["state"]) == 2
    bench.restore(after2)
    fresh = bench.make(lr=123.0)
    fresh.load_state_dict(sd)
    fresh.step()
    assert bits_equal(bench.snapshot(), straight)
    assert fresh.state[bench.params[0]]["step"] == 3


# ---------------------------------------------------------------- the trainer
def test_trainer_clips_inside_the_fused_sgd_update_once_per_window(tmp_path, monkeypatch):
    """two micro-steps of a k = 2 window: ONE norm computation, no in-place scaling, `train/grad_norm` in the meter, and the
    parameters after the window are, bit for bit, those of FusedSGD(max_grad_norm) stepped by hand on the gradient the trainer's
    optimizer saw"""
    from diffulab_amd import Diffuser
    from diffulab_amd.training import BaseTrainer, FusedSGD
    from diffulab_amd.training.utils import AverageMeter

    def run(max_grad_norm):
        m = small_dit()
        d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=4)
        opt = FusedSGD(m.parameters(), **NESTEROV)
        tr = BaseTrainer(n_epoch=1, gradient_accumulation_step=2, save_path=tmp_path, project_name=f"sgd{max_grad_norm}",
                         max_grad_norm=max_grad_norm)
        counts = {"grad_sumsq": 0, "clip_coef": 0, "scale_inplace": 0, "sgd_step": 0}
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
    assert counts == {"grad_sumsq": 0, "clip_coef": 0, "scale_inplace": 0, "sgd_step": 1}
    assert "train/grad_norm" not in meter.keys and opt.max_grad_norm is None
    norm64 = (g0.double() ** 2).sum().sqrt().item()
    mx = 0.5 * norm64  # (the same inputs and seed give the same gradient up to the atomics' reordering: this bound clips)
    m, opt, meter, counts, (w0, g0) = run(mx)
    assert counts == {"grad_sumsq": 1, "clip_coef": 1, "scale_inplace": 0, "sgd_step": 1}
    assert opt.max_grad_norm == mx and opt._clip_out[1].item() < 1
    norm64 = (g0.double() ** 2).sum().sqrt().item()
    assert meter.count["train/grad_norm"] == 1
    assert abs(meter.avg["train/grad_norm"] - norm64) <= 0.5 * (ops.grad_sumsq_chain(g0.numel()) + 2) * U * norm64
    after = m._flat.clone()
    with torch.no_grad():
        m._flat.copy_(w0)
        m._flat_grad.copy_(g0)
    manual = FusedSGD(m.parameters(), max_grad_norm=mx, **NESTEROV)
    manual.step()
    assert torch.equal(m._flat.view(torch.int32), after.view(torch.int32)) and not torch.equal(after, w0)


# ---------------------------------------------------------------- the UNet: the engines see the update
@pytest.mark.parametrize("regime", ["bf16", "fp32"])
def test_unet_forward_sees_the_fused_sgd_update(regime):
    """one FusedSGD step on the tiny UNet: the next forward on the same inputs gives another loss, so the engine's copies of the
    weights (bf16 shadows / packed f32 forms) were refreshed -- the raw-pointer update announces itself through bump_param_epoch"""
    from diffulab_amd import Diffuser
    from diffulab_amd.networks.denoisers import UNetModel
    from diffulab_amd.training import FusedSGD
    from oracle import unet as ounet

    kw = dict(image_size=(16, 16), in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(2,),
              channel_mult=(1, 2), num_heads=2, use_scale_shift_norm=True, resblock_updown=True, n_classes=10, classifier_free=True)
    m = UNetModel(**dict(kw, image_size=[16, 16], attention_resolutions=[2], channel_mult="1, 2"))
    m.load_state_dict(synth.generic_params(ounet.param_shapes(ounet.UNetConfig(**kw)), seed=23))
    m = m.set_precision(regime).to(DEV)
    gd = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    B = 4
    x0, noise = synth.normal("un.x0", (B, 1, 16, 16)).to(DEV), synth.normal("un.noise", (B, 1, 16, 16)).to(DEV)
    y, ti = synth.integers("un.y", (B,), 10).to(DEV), torch.tensor([3, 500, 999, 0], dtype=torch.int32, device=DEV)

    def loss():
        return gd.compute_loss({"x": x0.clone(), "y": y, "p": 0.0}, timesteps=ti, noise=noise)["loss"]

    opt = FusedSGD(m.parameters(), **NESTEROV)
    opt.zero_grad()
    l0 = loss()
    l0.backward()
    w0 = m._flat.clone()
    opt.step()
    assert not torch.equal(m._flat, w0)
    with torch.no_grad():
        l1 = loss()
    print(f"UNet {regime}: loss {l0.item():.6f} -> {l1.item():.6f}")
    assert np.isfinite(l1.item()) and l1.item() != l0.item()
