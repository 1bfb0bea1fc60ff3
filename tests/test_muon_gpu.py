"""GPU tests of the fused Muon: the grouped Newton-Schulz kernels against an fp64 restatement of torch's
``_zeropower_via_newtonschulz``, their write guards and bit identities, and ``FusedMuon`` on the depth-2 DiT (parity with
``torch.optim.Muon`` + ``torch.optim.AdamW`` on the CPU, launches, clipping, checkpoints, the trainer).

Newton-Schulz bar.  Oracle: `ns64`, the iteration in fp64 on the bf16-rounded input.  Measure: ``||O - O64||_F / ||O64||_F``.  Bar:
1.5 x the same measure of torch's own bf16 run on the CPU on the same input (the project's rule for bf16 against the reference);
torch lands at 1.1e-2 .. 1.5e-2 on the Gaussian inputs used here.  The inputs are standard normal: the iteration amplifies
perturbations of small singular values, so nearly rank-deficient inputs separate two correct bf16 implementations by more than
the factor.

f32 bar: test_sgd_gpu's, ``max|a - b| / max|b| < 1e-6``.

Full step.  The per-tensor change ``p_after - p_before`` of three steps.  Muon matrices: the change is measured against `step64` (the
step in fp64 with the bf16 rounding of the Newton-Schulz input) and the bar is 1.5 x the same measure of ``torch.optim.Muon``'s
change on the CPU -- the Newton-Schulz bar carried to the update; the figure against torch's run itself is printed beside it.
Everything else: the change against ``torch.optim.AdamW``'s on the CPU under the f32 bar.  That bar is on a DIFFERENCE of f32
numbers, so the inputs keep it meaningful: parameters of standard deviation 0.02 and learning rates of 0.2 make three steps move
an auxiliary parameter by about 0.6, 1e7 ulps of the parameter, where two correct f32 implementations that round a few ulps apart
stay inside 1e-6 (at lr = 1e-3 and gains of 1.0 a single ulp of the parameter is 4e-5 of the change).  And the auxiliary betas of
that test are ones f32 holds exactly, (0.875, 1 - 2^-10): `dl_adamw_step`, whose update the auxiliary ranges must reproduce bit for
bit, forms 1 - beta2 in f32, which at beta2 = 0.999 is 1.3e-5 off the 0.001 torch passes from f64 -- 6.7e-6 of the change (measured),
FusedAdamW's figure as much as FusedMuon's, and invisible in the measure on the parameters the project's AdamW tests use.  The
default betas are covered on the parameters (three steps at the default learning rate) and by the bit identity with FusedAdamW.

Measured on the MI355X (figures printed by the tests): see DESIGN.md, section "Muon"."""

import copy
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from torch.optim._muon import _zeropower_via_newtonschulz  # noqa: E402

from diffulab_amd import ops  # noqa: E402

DEV = "cuda"
GUARD = 8
CANARY = 1234.5
BAR = 1e-6
COEF = (3.4445, -4.7750, 2.0315)
EPS = 1e-7
SHAPES = [(64, 128), (128, 64), (64, 64), (192, 448), (448, 192), (128, 1024)]
IDS = [f"{r}x{c}" for r, c in SHAPES]


def err(a, b):
    """max|a - b| / max|b| in f64 (both zero everywhere: 0)"""
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    top = b.abs().max().item()
    d = (a - b).abs().max().item()
    return d / top if top > 0 else d


def fro(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm()).item()


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def bits_equal(a, b):
    return all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def ns64(u_bf16, steps, coef=COEF, eps=EPS):
    """torch's _zeropower_via_newtonschulz restated in fp64 on the bf16-rounded input `u_bf16`"""
    a, b, c = coef
    x = u_bf16.double()
    tall = x.shape[0] > x.shape[1]
    if tall:
        x = x.T
    x = x / x.norm().clamp(min=eps)
    for _ in range(steps):
        A = x @ x.T
        P = b * A + c * (A @ A)
        x = a * x + P @ x
    return x.T if tall else x


class Guarded:
    """a device buffer of n elements starting `phase` elements past a 16-byte boundary (f32) with canaries on both sides"""

    def __init__(self, n, phase=0, fill=0.0, dtype=torch.float32):
        self.base = torch.full((GUARD + phase + n + GUARD,), CANARY, device=DEV, dtype=dtype)
        assert self.base.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + phase, GUARD + phase + n
        self.view = self.base[self.lo : self.hi]
        self.view.fill_(fill)
        if dtype == torch.float32:
            assert (self.view.data_ptr() % 16) // 4 == phase % 4

    def snapshot(self):
        self.saved = self.base.clone()

    def intact_outside(self, lo=0, hi=0):
        """bit-unchanged since snapshot() except view[lo:hi]"""
        a, b = bits(self.base), bits(self.saved)
        return torch.equal(a[: self.lo + lo], b[: self.lo + lo]) and torch.equal(a[self.lo + hi :], b[self.lo + hi :])


def guard_workspaces(plan):
    """replace the plan's workspaces by guarded ones of the same sizes -> the guards"""
    out = {}
    for name in ("xws", "aws", "partials", "norms"):
        t = getattr(plan, name)
        gd = Guarded(t.numel(), 0, 0.0, t.dtype)
        setattr(plan, name, gd.view)
        out[name] = gd
    return out


def orthogonalize(plan, g, m, steps, p=None, v=None):
    """bf16(g) of every matrix of the plan through the kernels: with momentum 0 and no Nesterov the pre pass leaves U = m = g"""
    p = torch.zeros_like(g) if p is None else p
    v = torch.zeros_like(g) if v is None else v
    ops.muon_pre(plan, p, g, m, v, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0.0, False)
    return ops.muon_orthogonalize(plan, EPS, COEF, steps)


@pytest.fixture(scope="module")
def cases():
    """per shape: the Gaussian input, torch's bf16 run on the CPU and the fp64 oracle at 1 and 5 steps, and what the kernels give for
    the matrix launched alone on ordinary allocations (0, 1 and 5 steps)"""
    gen = torch.Generator().manual_seed(1234)
    out = {}
    for shape in SHAPES:
        g = torch.randn(shape, generator=gen)
        rec = {"g": g, "torch": {}, "o64": {}, "gpu": {}, "norm": None}
        for k in (1, 5):
            rec["torch"][k] = _zeropower_via_newtonschulz(g, COEF, k, EPS).float()
            rec["o64"][k] = ns64(g.bfloat16(), k)
        n = g.numel()
        plan = ops.MuonPlan(n, [(0, shape[0], shape[1], 1.0)], 0, DEV)
        gd = g.to(DEV).reshape(-1)
        for k in (0, 1, 5):
            m = torch.zeros(n, device=DEV)
            launches = orthogonalize(plan, gd, m, k)
            assert launches == 2 + 3 * k
            rec["gpu"][k] = plan.result(0, k).clone()
            assert torch.equal(m, gd)
        rec["norm"] = plan.norms[0].item()
        out[shape] = rec
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------- Newton-Schulz against fp64
@pytest.mark.parametrize("steps", [1, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_newton_schulz_against_fp64(cases, shape, steps):
    rec = cases[shape]
    e_torch = fro(rec["torch"][steps], rec["o64"][steps])
    e_gpu = fro(rec["gpu"][steps].float(), rec["o64"][steps])
    print(f"{shape} ns_steps={steps}: kernels {e_gpu:.3e}, torch bf16 on the CPU {e_torch:.3e}, ratio {e_gpu / e_torch:.2f} (bar 1.5)")
    assert rec["gpu"][steps].shape == shape and bool(torch.isfinite(rec["gpu"][steps].float()).all())
    assert e_gpu < 1.5 * e_torch


def test_zero_steps_return_the_normalised_bf16_input(cases):
    """X = bf16(bf16(g) / norm) exactly, with the norm the kernels folded; that norm against fp64: per-thread chains of 8 terms, an
    8-level tree in f32, the fold in f64, the square root and the rounding to f32 -- (8 + 8 + 2) * 2^-24"""
    for shape, rec in cases.items():
        gb = rec["g"].bfloat16()
        norm64 = gb.double().norm().item()
        assert abs(rec["norm"] - norm64) <= 18 * 2.0**-24 * norm64, shape
        want = (gb.float() / np.float32(rec["norm"])).bfloat16()
        assert torch.equal(bits(rec["gpu"][0].cpu()), bits(want)), shape


def test_zero_gradient_gives_a_zero_update_without_nan():
    shape = (192, 448)
    n = shape[0] * shape[1]
    plan = ops.MuonPlan(n, [(0, *shape, 1.0)], 0, DEV)
    g, m = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    orthogonalize(plan, g, m, 5)
    o = plan.result(0, 5)
    assert plan.norms[0].item() == np.float32(EPS) and torch.equal(o.float(), torch.zeros(shape, device=DEV))
    p = torch.randn(n, device=DEV)
    p0 = p.clone()
    ops.muon_post(plan, p, 0.1, 0.0, 5)
    assert torch.equal(p, p0)


def test_two_runs_on_the_same_input_are_bit_identical(cases):
    shape = (192, 448)
    n = shape[0] * shape[1]
    g = cases[shape]["g"].to(DEV).reshape(-1)
    for _ in range(2):
        plan = ops.MuonPlan(n, [(0, *shape, 1.0)], 0, DEV)
        orthogonalize(plan, g, torch.zeros(n, device=DEV), 5)
        assert torch.equal(bits(plan.result(0, 5)), bits(cases[shape]["gpu"][5]))


# ---------------------------------------------------------------- one grouped call: every phase, guards, == launched alone
@pytest.mark.parametrize("phases", [(0, 0, 0, 0), (1, 1, 1, 1), (1, 2, 3, 0)], ids=["aligned", "phase1", "mixed"])
def test_grouped_call_equals_every_matrix_alone_and_writes_nothing_else(cases, phases):
    """the six matrices in one buffer at offsets whose 16-byte phases are 0, 1, 2, 3, 0, 2 (auxiliary gaps between them), p / g / m / v
    at the 16-byte phases `phases`, every buffer and workspace between canaries: one pre / orthogonalize / post sequence"""
    gaps = [4, 5, 9, 13, 5, 6, 3]  # before each matrix and after the last: offsets 4, 8201, 16402, 20511, ... of phase 0, 1, 2, 3, 0, 2
    lr, wd, steps = 0.25, 0.1, 5
    mats, off = [], 0
    for shape, gap in zip(SHAPES, gaps):
        off += gap
        mats.append((off, shape[0], shape[1], ops.muon_ratio(*shape, None)))
        off += shape[0] * shape[1]
    n = off + gaps[-1]
    assert [m[0] % 4 for m in mats] == [0, 1, 2, 3, 0, 2]
    gen = torch.Generator().manual_seed(99)
    p0, g0 = torch.randn(n, generator=gen).to(DEV), torch.randn(n, generator=gen).to(DEV)
    for (o, r, c, _), shape in zip(mats, SHAPES):
        g0[o : o + r * c] = cases[shape]["g"].to(DEV).reshape(-1)
    P, G, M, V = (Guarded(n, ph) for ph in phases)
    P.view.copy_(p0), G.view.copy_(g0)
    plan = ops.MuonPlan(n, mats, phases[0], DEV)
    ws = guard_workspaces(plan)
    for b in (P, G, M, V, *ws.values()):
        b.snapshot()
    ops.muon_pre(plan, P.view, G.view, M.view, V.view, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0.0, False)
    assert ops.muon_orthogonalize(plan, EPS, COEF, steps) == 2 + 3 * steps
    ops.muon_post(plan, P.view, lr, wd, steps)
    torch.cuda.synchronize()
    assert G.intact_outside(), "the gradient or its guards were written"
    assert all(b.intact_outside(0, n) for b in (P, M, V)), "a write outside [0, n)"
    assert all(gd.intact_outside(0, gd.hi - gd.lo) for gd in ws.values()), "a write outside a workspace"
    # auxiliary ranges: dl_adamw_step's update of the whole buffer, bit for bit; v is untouched on the Muon ranges
    pa, ma, va = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    ops.adamw_step(pa, g0, ma, va, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1)
    aux = torch.ones(n, dtype=torch.bool, device=DEV)
    for i, ((o, r, c, ratio), shape) in enumerate(zip(mats, SHAPES)):
        aux[o : o + r * c] = False
        alone = cases[shape]["gpu"][steps]
        assert torch.equal(bits(plan.result(i, steps)), bits(alone)), f"{shape}: grouped != alone"
        assert torch.equal(M.view[o : o + r * c], g0[o : o + r * c]) and not V.view[o : o + r * c].any()
        # the post pass alone on an ordinary allocation
        solo = ops.MuonPlan(r * c, [(0, r, c, ratio)], 0, DEV)
        orthogonalize(solo, g0[o : o + r * c].clone(), torch.zeros(r * c, device=DEV), steps)
        ps = p0[o : o + r * c].clone()
        ops.muon_post(solo, ps, lr, wd, steps)
        assert torch.equal(bits(P.view[o : o + r * c]), bits(ps)) and not torch.equal(ps, p0[o : o + r * c])
    assert int(aux.sum()) == sum(gaps)
    for got, want in ((P.view, pa), (M.view, ma), (V.view, va)):
        assert torch.equal(bits(got[aux]), bits(want[aux]))


# ---------------------------------------------------------------- FusedMuon on the depth-2 DiT
FULL = dict(lr=0.2, aux_lr=0.2, aux_betas=(0.875, 1 - 2.0**-10))  # (the module docstring says why)


def make_dit(depth=2):
    """the depth-2 DiT at DiT-S/2's widths (six heads of 64, embedding_dim 384, a null class), parameters of standard deviation 0.02"""
    from diffulab_amd import MMDiT

    m = MMDiT(simple_dit=True, inner_dim=384, embedding_dim=384, num_heads=6, depth=depth, n_classes=10, classifier_free=True,
              patch_size=2, input_channels=4)
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.02)
    m = m.to(DEV)
    m.flatten_parameters()
    return m


class Bench:
    """the model with three fixed synthetic gradients per parameter, plus two loose tensors outside the arena (one Muon matrix, one
    37 x 5 auxiliary tensor).  `run(k)` restores the parameters and takes k steps of a fresh FusedMuon; `torch_run(k)` does the same
    with torch.optim.Muon on the Muon matrices and torch.optim.AdamW on the rest, on CPU copies; `step64` in fp64.  Keyword arguments
    are FusedMuon's: the `aux_*` ones go to AdamW, the others to Muon."""

    STEPS = 3

    def __init__(self):
        from diffulab_amd.training import FusedMuon

        self.model = make_dit()
        gen = torch.Generator().manual_seed(11)
        self.loose = [torch.nn.Parameter((torch.randn(s, generator=gen) * 0.02).to(DEV)) for s in ((128, 64), (37, 5))]
        self.params = list(self.model.parameters()) + self.loose
        self.names = [n for n, _ in self.model.named_parameters()] + ["loose.matrix", "loose.aux"]
        self.is_muon = [FusedMuon.qualifies(p) for p in self.params]
        self.init = [p.detach().clone() for p in self.params]
        self.grads = [[torch.randn(p.shape, generator=gen) for p in self.params] for _ in range(self.STEPS)]
        self.grads_dev = [[g.to(DEV) for g in gs] for gs in self.grads]
        for p in self.loose:
            p.grad = torch.zeros_like(p)
        self._torch_runs = {}

    def restore(self, weights=None):
        with torch.no_grad():
            for p, w in zip(self.params, weights or self.init):
                p.copy_(w)

    def set_grads(self, s):
        with torch.no_grad():
            for p, g in zip(self.params, self.grads_dev[s]):
                p.grad.copy_(g)

    def snapshot(self):
        return [p.detach().clone() for p in self.params]

    def make(self, grad_scale=1.0, **kw):
        from diffulab_amd.training import FusedMuon

        opt = FusedMuon(self.params, **kw)
        opt.grad_scale = grad_scale
        return opt

    def run(self, steps=STEPS, grad_scale=1.0, first=0, opt=None, **kw):
        if opt is None:
            self.restore()
            opt = self.make(grad_scale, **kw)
        for s in range(first, first + steps):
            self.set_grads(s)
            opt.step()
            assert all(torch.equal(p.grad, g) for p, g in zip(self.params, self.grads_dev[s])), "step() rewrote a gradient"
        return opt, self.snapshot()

    def torch_run(self, steps=STEPS, **kw):
        """-> (CPU parameters after the steps, the Muon momentum buffers, fp64 parameters of `step64`); once per setting"""
        key = (steps, tuple(sorted(kw.items())))
        if key not in self._torch_runs:
            ps = [torch.nn.Parameter(w.cpu().clone()) for w in self.init]
            mu = [p for p, q in zip(ps, self.is_muon) if q]
            au = [p for p, q in zip(ps, self.is_muon) if not q]
            mkw = {k: v for k, v in kw.items() if not k.startswith("aux_")}
            lr = mkw.get("lr", 1e-3)
            o1 = torch.optim.Muon(mu, **mkw)
            o2 = torch.optim.AdamW(au, lr=kw.get("aux_lr", lr), betas=kw.get("aux_betas", (0.9, 0.999)))
            p64 = [w.cpu().double() for w in self.init]
            b64 = [torch.zeros_like(w) for w in p64]
            for s in range(steps):
                for p, g in zip(ps, self.grads[s]):
                    p.grad = g.clone()
                o1.step(), o2.step()
                for i, q in enumerate(self.is_muon):
                    if q:
                        p64[i], b64[i] = self.step64(p64[i], self.grads[s][i].double(), b64[i], **mkw)
            bufs = [o1.state[p]["momentum_buffer"].clone() if q else None for p, q in zip(ps, self.is_muon)]
            self._torch_runs[key] = ([p.detach().clone() for p in ps], bufs, p64)
        return self._torch_runs[key]

    @staticmethod
    def step64(p, g, buf, lr=1e-3, weight_decay=0.1, momentum=0.95, nesterov=True, adjust_lr_fn=None):
        """torch's single-tensor Muon step in fp64, the Newton-Schulz input rounded to bf16 as torch rounds it"""
        buf = buf + (g - buf) * (1 - momentum)
        u = g + (buf - g) * momentum if nesterov else buf
        o = ns64(u.float().bfloat16(), 5)
        return p * (1 - lr * weight_decay) - lr * ops.muon_ratio(*p.shape, adjust_lr_fn) * o, buf


@pytest.fixture(scope="module")
def bench():
    return Bench()


def muon_ranges(bench, opt):
    """[(parameter index, lo, hi)] of the arena's Muon matrices in the arena state, and the arena state"""
    st = opt.state[bench.params[0]]
    base = bench.model._flat.data_ptr()
    out = []
    for i, (p, q) in enumerate(zip(bench.params[:-2], bench.is_muon)):
        if q:
            lo = (p.data_ptr() - base) // 4
            out.append((i, lo, lo + p.numel()))
    return out, st


@pytest.mark.parametrize("adjust", [None, "match_rms_adamw"], ids=["original", "match_rms_adamw"])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_full_step_against_torch_muon_and_adamw_on_the_cpu(bench, wd, adjust):
    kw = dict(FULL, weight_decay=wd, adjust_lr_fn=adjust)
    opt, got = bench.run(**kw)
    want, _, p64 = bench.torch_run(**kw)
    worst_ns, worst_aux = 0.0, 0.0
    for name, q, p0, a, b, c in zip(bench.names, bench.is_muon, bench.init, got, want, p64):
        d_got, d_torch = a.double().cpu() - p0.double().cpu(), b.double() - p0.double().cpu()
        if q:
            d64 = c - p0.double().cpu()
            e_gpu, e_torch = fro(d_got, d64), fro(d_torch, d64)
            print(f"{name} {tuple(p0.shape)}: kernels {e_gpu:.3e}, torch {e_torch:.3e} against fp64 (ratio {e_gpu / e_torch:.2f}, bar "
                  f"1.5); kernels against torch {fro(d_got, d_torch):.3e}")
            worst_ns = max(worst_ns, e_gpu / e_torch)
            assert e_gpu < 1.5 * e_torch, name
        else:
            e = err(d_got, d_torch)
            worst_aux = max(worst_aux, e)
            assert e < BAR, (name, e)
    print(f"wd={wd} adjust_lr_fn={adjust}: worst Muon ratio {worst_ns:.2f} (bar 1.5), worst auxiliary change err {worst_aux:.3e} (bar {BAR:.0e})")
    assert not bits_equal(got, bench.init)
    key = bench.params[0]
    n = bench.model._flat.numel()
    assert set(opt.state[key]) == {"step", "m", "v"} and opt.state[key]["m"].numel() == n and opt.state[key]["step"] == 3
    assert set(opt.state[bench.loose[0]]) == {"step", "m"} and set(opt.state[bench.loose[1]]) == {"step", "m", "v"}
    assert len(opt.state) == 3, "one arena entry and one per loose tensor"


@pytest.mark.parametrize("nesterov", [True, False])
def test_momentum_buffer_and_auxiliary_ranges_after_three_steps(bench, nesterov):
    """every default (lr 1e-3, betas (0.9, 0.999)): the momentum buffers against torch.optim.Muon's, the auxiliary parameters
    against torch.optim.AdamW's, both on the CPU"""
    kw = dict(nesterov=nesterov)
    opt, got = bench.run(**kw)
    want, bufs, _ = bench.torch_run(**kw)
    ranges, st = muon_ranges(bench, opt)
    assert len(ranges) == 13
    worst = 0.0
    for i, lo, hi in ranges:
        worst = max(worst, err(st["m"][lo:hi], bufs[i]))
    worst = max(worst, err(opt.state[bench.loose[0]]["m"], bufs[-2]))
    worst_p = max(err(a, b) for a, b, q in zip(got, want, bench.is_muon) if not q)
    print(f"nesterov={nesterov}: momentum buffers err {worst:.3e}, auxiliary parameters err {worst_p:.3e} (bar {BAR:.0e})")
    assert worst < BAR and worst_p < BAR


def test_without_a_qualifying_matrix_the_update_is_fused_adamws(bench):
    """use_muon=False leaves no Muon matrix: three steps, bit for bit FusedAdamW's parameters and moments -- the arena (float4 loop)
    and the loose tensors (37 x 5: one element in the loop over the last n % 4)"""
    from diffulab_amd.training import FusedAdamW, FusedMuon

    results = []
    for cls in (FusedAdamW, FusedMuon):
        bench.restore()
        if cls is FusedMuon:
            opt = FusedMuon([{"params": bench.params, "use_muon": False}], lr=1e-3, aux_weight_decay=0.05, aux_betas=(0.8, 0.99))
        else:
            opt = FusedAdamW(bench.params, lr=1e-3, weight_decay=0.05, betas=(0.8, 0.99))
        for s in range(3):
            bench.set_grads(s)
            opt.step()
        sts = [opt.state[k] for k in (bench.params[0], *bench.loose)]
        results.append(bench.snapshot() + [st[k].clone() for st in sts for k in ("m", "v")])
        assert all(st["step"] == 3 for st in sts)
    assert bits_equal(*results) and not bits_equal(results[0][: len(bench.init)], bench.init)


def test_clipping_and_grad_scale_act_before_the_momentum(bench):
    norm64 = sum((g.double() ** 2).sum() for g in bench.grads[0]).sqrt().item()
    tol = 0.5 * (ops.grad_sumsq_chain(bench.model._flat_grad.numel()) + 2) * 2.0**-24  # (test_sgd_gpu's bound on the norm)
    _, plain = bench.run(1)
    # a bound that does not clip: the plain update, bit for bit
    opt, loose_bound = bench.run(1, max_grad_norm=1e9)
    assert opt._clip_out[1].item() == 1.0 and bits_equal(loose_bound, plain)
    assert abs(opt.last_grad_norm.item() - norm64) <= tol * norm64
    # coefficient c: the plain update with grad_scale * c
    opt, clipped = bench.run(1, grad_scale=0.5, max_grad_norm=0.125 * norm64)
    norm, coef = opt._clip_out.cpu().numpy()
    assert abs(float(norm) - 0.5 * norm64) <= tol * 0.5 * norm64 and abs(coef - 0.25) < 1e-3
    _, manual = bench.run(1, grad_scale=float(np.float32(0.5) * coef))
    assert bits_equal(clipped, manual) and not bits_equal(clipped, plain)


def test_launches_do_not_depend_on_the_number_of_matrices(monkeypatch):
    """19 library launches per arena step at ns_steps = 5 (pre, fold, scale, 5 x 3 GEMM phases, post), at depth 2 and at depth 3"""
    from diffulab_amd.training import FusedMuon

    counts = {}
    for depth in (2, 3):
        m = make_dit(depth)
        m._flat_grad.normal_()
        opt = FusedMuon(m.parameters(), max_grad_norm=1.0)
        calls, launches = [], []
        with monkeypatch.context() as mp:
            for name in ("grad_sumsq", "clip_coef", "muon_pre", "muon_post", "adamw_step", "adamw_step_clip", "sgd_step", "scale_inplace"):
                mp.setattr(ops, name, (lambda f, nm: lambda *a, **k: (calls.append(nm), launches.append(1), f(*a, **k))[2])(
                    getattr(ops, name), name))
            orig = ops.muon_orthogonalize
            mp.setattr(ops, "muon_orthogonalize", lambda *a, **k: (calls.append("muon_orthogonalize"), launches.append(orig(*a, **k)))[0])
            opt.step()
            opt.step()
        n_mat = sum(FusedMuon.qualifies(p) for p in m.parameters())
        counts[depth] = (calls, sum(launches), n_mat)
    assert counts[2][2] == 13 and counts[3][2] == 18
    assert counts[2][0] == ["grad_sumsq", "clip_coef", "muon_pre", "muon_orthogonalize", "muon_post"] * 2
    assert counts[2][:2] == counts[3][:2] and counts[2][1] == 2 * (2 + 19)


def test_resumes_from_its_own_state_dict(bench):
    ref, straight = bench.run(3)
    opt, after2 = bench.run(2)
    sd = copy.deepcopy(opt.state_dict())
    assert len(sd["state"]) == 3
    bench.restore(after2)
    fresh = bench.make(lr=123.0)  # (the checkpoint's param_groups replace the constructor's)
    fresh.load_state_dict(sd)
    bench.run(1, first=2, opt=fresh)
    assert bits_equal(bench.snapshot(), straight)
    key = bench.params[0]
    assert fresh.state[key]["step"] == 3 and fresh.param_groups[0]["lr"] == 1e-3
    assert bits_equal([fresh.state[key]["m"], fresh.state[key]["v"]], [ref.state[key]["m"], ref.state[key]["v"]])


# ---------------------------------------------------------------- the trainer
def test_trainer_descends_with_optimizer_muon(tmp_path):
    """optimizer=muon through the config and BaseTrainer on the smallest DiT of test_trainer_gpu: a finite loss that falls.  A
    descent test only, no claim about Muon against AdamW."""
    import os

    from torch.utils.data import DataLoader

    from diffulab_amd import Diffuser, MMDiT
    from diffulab_amd.config import instantiate, load_config
    from diffulab_amd.datasets import SyntheticDataset
    from diffulab_amd.training import BaseTrainer, FusedMuon

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    c = load_config(os.path.join(root, "configs"), "train_mnist_flow_matching", ["optimizer=muon"])
    torch.manual_seed(0)
    m = MMDiT(simple_dit=True, input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4,
              patch_size=2, depth=2, n_classes=10, classifier_free=True)
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=8, extra_args={"logits_normal": True})
    opt = instantiate(c.optimizer, params=m.parameters(), lr=0.02, aux_lr=2e-3, weight_decay=0.0, aux_weight_decay=0.0)
    assert type(opt) is FusedMuon
    mk = lambda n, seed: DataLoader(SyntheticDataset(n, (4, 16, 16), 10, seed), batch_size=16, drop_last=True)  # noqa: E731
    tr = BaseTrainer(n_epoch=3, gradient_accumulation_step=1, save_path=tmp_path, project_name="mu")
    tr.train(diffuser=d, optimizer=opt, train_dataloader=mk(128, 1), val_dataloader=mk(32, 2), val_steps=4, p_classifier_free_guidance=0.1)
    rows = [json.loads(l) for l in (tmp_path / "mu" / "metrics.jsonl").read_text().splitlines()]
    train = [r["train/loss"] for r in rows if "train/loss" in r]
    print(f"train/loss per epoch: {train}")
    assert len(train) == 3 and all(np.isfinite(v) for v in train) and train[-1] < train[0]
    key = next(p for p in m.parameters())
    assert opt.state[key]["step"] == 24 and any(opt.is_muon(p, opt.param_groups[0]) for p in m.parameters())
