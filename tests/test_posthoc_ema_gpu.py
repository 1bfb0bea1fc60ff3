"""Post-hoc EMA on the GPU: the two kernels of csrc/ema.hip element by element against fp64 with write guards, then PowerEMA,
snapshots, posthoc_ema.synthesize and the trainer on the smallest class-conditional MMDiT and UNetModel the other GPU tests build.

Kernel cases run through the C ABI.  Every buffer a launch may write sits between two runs of NaN-poisoned guard elements that are
checked afterwards; every read-only input is compared bit for bit with what was put there.  Bounds come from
tests/posthoc_ema_common.py (three roundings of the update as written; the standard bound of a length-K multiply-add chain)."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

import posthoc_ema_common as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024          # poisoned f32 elements on each side of a buffer (a multiple of 4: the window keeps the allocation's alignment)
POISON = 0x7FC1DEAD   # a quiet NaN with a payload no kernel produces
BIG = 2 ** 21 + 3075  # past one pass of the capped grid (2048 blocks x 256 threads x 4 floats), with a scalar tail of 3
INVALID = -1          # DL_ERR_INVALID
ACCUMULATE = 1        # DL_LINCOMB_ACCUMULATE
WEIGHTS = (1.0, 0.0, 0.25, 1.7e-5)


# ------------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    return _lib.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def raw(L, name, *args) -> int:
    """the entry point's return value (L.call would raise on a refusal)"""
    return L._fns[name][0](*args)


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def same_bits(a, b) -> bool:
    if a.dtype != torch.float32:
        return bool(torch.equal(a, b.to(a.device)))
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b.to(a.device))))


def randn(n, seed, scale=1.0) -> torch.Tensor:
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


class Buf:
    """n f32 elements between two runs of GUARD poisoned ones; init None: the window starts poisoned too (an output)"""

    def __init__(self, n: int, init: torch.Tensor | None = None):
        self.buf = torch.empty(n + 2 * GUARD, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(POISON)
        self.t = self.buf[GUARD:GUARD + n]
        self.init = init
        if init is not None:
            assert init.dtype == torch.float32 and init.numel() == n
            self.t.copy_(init)
        assert self.t.data_ptr() % 16 == 0

    def ptr(self) -> int:
        return self.t.data_ptr()

    def guards(self, what):
        g = self.buf.view(torch.int32)
        assert bool((g[:GUARD] == POISON).all()) and bool((g[-GUARD:] == POISON).all()), f"{what}: guard written"

    def unchanged(self, what):
        self.guards(what)
        assert same_bits(self.t, self.init), f"{what}: a buffer the call must not write was written"

    def np64(self) -> np.ndarray:
        return self.t.cpu().numpy().astype(np.float64)


def within(got: np.ndarray, ref: np.ndarray, bound: np.ndarray, what: str) -> float:
    err = np.abs(got - ref)
    bad = ~(err <= bound)  # (NaN fails)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements outside the bound, worst ratio {np.nanmax(err / bound):.3f}"
    return float((err / bound).max())


# ------------------------------------------------------------------------------------------------------------------ dl_ema_update_multi
def update_multi(L, emas, p, K, weights, n, check=True):
    w = list(weights) + [0.5] * (4 - len(weights))
    rc = raw(L, "dl_ema_update_multi", *(e.ptr() if e is not None else None for e in emas), p.ptr() if p is not None else None, K,
             *w, n, _s())
    if check:
        assert rc == 0, (rc, L.cdll.dl_last_error().decode())
    return rc


@pytest.mark.parametrize("n", [1, 7, 1027, BIG])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_update_multi_element_by_element(lib, K, n):
    """every rotation of the weight set over the K profiles; the profile slots beyond K hold real buffers that must stay as they are"""
    p0 = randn(n, seed=n)
    e0 = [randn(n, seed=n + 1 + k, scale=1.5) for k in range(4)]
    for rot in range(0, 4, K):
        weights = [WEIGHTS[(rot + k) % 4] for k in range(K)]
        cid = f"ema_multi-K{K}-n{n}-w{weights}"
        runs = []
        for _ in range(2):
            P, E = Buf(n, p0), [Buf(n, e) for e in e0]
            update_multi(lib, E, P, K, weights, n)
            torch.cuda.synchronize()
            P.unchanged(f"{cid}: p")
            for k in range(K, 4):
                E[k].unchanged(f"{cid}: unused profile {k}")
            for k in range(K):
                E[k].guards(f"{cid}: profile {k}")
            runs.append([E[k].t.clone() for k in range(K)])
        assert all(same_bits(a, b) for a, b in zip(*runs)), f"{cid}: two runs differ"
        worst = 0.0
        for k, w in enumerate(weights):
            got = runs[0][k]
            if w == 1.0:
                assert same_bits(got, p0), f"{cid}: w = 1 must give p's bits"
            if w == 0.0:
                assert same_bits(got, e0[k]), f"{cid}: w = 0 must leave the EMA's bits"
            w32 = float(np.float32(w))
            ref, bound = pc.ema_step_ref(e0[k].numpy(), p0.numpy(), w32)
            worst = max(worst, within(got.cpu().numpy().astype(np.float64), ref, bound, f"{cid}: profile {k}"))
        print(f"{cid}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("n", [1, 7, 1027, BIG])
def test_update_multi_with_one_profile_gives_the_bits_of_dl_ema_update(lib, n):
    """w = 1.0f - beta, as dl_ema_update forms it.  For 0 < w < 1 the two entry points agree on every element.  At beta = 0 (w = 1) and
    beta = 1 (w = 0) the new entry point is exact by contract (p's bits, the EMA's bits) while dl_ema_update evaluates
    e + 1 * (p - e) and e + 0 * (p - e), which are p and e only where the difference is exact: there the two agree on exactly the
    elements where dl_ema_update is itself exact, which is asserted, and nowhere else."""
    p0, e0 = randn(n, seed=3 * n), randn(n, seed=3 * n + 1, scale=1.5)
    for beta in (0.75, 0.9999, float(np.float32(1.0 - 1.7e-5)), 0.0, 1.0):
        w = float(np.float32(1.0) - np.float32(beta))
        A, B, P = Buf(n, e0), Buf(n, e0), Buf(n, p0)
        update_multi(lib, [A, None, None, None], P, 1, [w], n)
        assert raw(lib, "dl_ema_update", B.ptr(), P.ptr(), beta, n, _s()) == 0
        torch.cuda.synchronize()
        A.guards("multi"), B.guards("single"), P.unchanged("p")
        if 0.0 < w < 1.0:
            assert same_bits(A.t, B.t), f"n {n} beta {beta}: K = 1 differs from dl_ema_update"
        else:
            exact = p0 if w == 1.0 else e0
            assert same_bits(A.t, exact)
            old_exact = bits(B.t).cpu() == bits(exact)
            agree = bits(A.t).cpu() == bits(B.t).cpu()
            assert bool(torch.equal(old_exact, agree))
            print(f"n {n} beta {beta}: dl_ema_update is exact on {int(old_exact.sum())} of {n} elements")


def test_update_multi_refusals_write_nothing(lib):
    n = 64
    p0, e0 = randn(n, 1), [randn(n, 2 + k) for k in range(4)]
    P, E = Buf(n, p0), [Buf(n, e) for e in e0]
    inf, nan = float("inf"), float("nan")
    cases = [dict(K=0), dict(K=5), dict(K=-2), dict(emas=[None, E[1], E[2], E[3]]), dict(emas=[E[0], None, E[2], E[3]]),
             dict(K=4, emas=[E[0], E[1], E[2], None]), dict(p=None), dict(n=0), dict(n=-n), dict(weights=[inf, 0.5]),
             dict(weights=[0.5, nan]), dict(weights=[-inf, 0.5]), dict(emas=[E[0], E[0], E[2], E[3]]),
             dict(K=4, emas=[E[0], E[1], E[2], E[0]]), dict(K=3, emas=[E[0], E[1], E[1], E[3]])]
    for kw in cases:
        a = dict(emas=E, p=P, K=2, weights=[0.5, 0.5], n=n)
        a.update(kw)
        rc = update_multi(lib, a["emas"], a["p"], a["K"], a["weights"], a["n"], check=False)
        assert rc == INVALID and "dl_ema_update_multi" in lib.cdll.dl_last_error().decode(), (kw, rc)
    torch.cuda.synchronize()
    P.unchanged("refusals: p")
    for k in range(4):
        E[k].unchanged(f"refusals: profile {k}")
    # what is beyond K is not looked at: NULL pointers and non-finite weights there are accepted
    assert update_multi(lib, [E[0], None, None, None], P, 1, [0.5, nan, inf, nan], n) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ dl_arena_lincomb
def lincomb(L, out, srcs, weights, n, flags=0, check=True):
    ptr_host = torch.tensor([s.ptr() for s in srcs], dtype=torch.int64)
    w_host = torch.tensor(np.asarray(weights, dtype=np.float32))
    ptr_dev, w_dev = ptr_host.to(DEV), w_host.to(DEV)
    rc = raw(L, "dl_arena_lincomb", out.ptr(), ptr_host.data_ptr(), ptr_dev.data_ptr(), w_host.data_ptr(), w_dev.data_ptr(), len(srcs), n,
             flags, _s())
    torch.cuda.synchronize()  # (the tables live until the kernel has read them)
    if check:
        assert rc == 0, (rc, L.cdll.dl_last_error().decode())
    return rc


LINCOMB_CASES = [(K, n) for K in (1, 3, 8, 33) for n in (5, 1027)] + [(3, BIG)]


@pytest.mark.parametrize("K,n", LINCOMB_CASES)
def test_lincomb_element_by_element(lib, K, n):
    """weights of alternating sign with sum |w| = 10; bound (K + 1) u S / (1 - (K + 1) u), S = sum_k |w_k src_k[i]|, u = 2^-24: the
    standard bound of a length-K chain of fused multiply-adds (one rounding per step; derivation in posthoc_ema_common.lincomb_ref)"""
    w = pc.alternating_weights(K)
    assert abs(float(np.abs(w.astype(np.float64)).sum()) - 10.0) < 1e-4
    src0 = [randn(n, seed=100 * K + k) for k in range(K)]
    S, O = [Buf(n, s) for s in src0], Buf(n)
    cid = f"lincomb-K{K}-n{n}"
    lincomb(lib, O, S, w, n)
    O.guards(cid)
    for k, s in enumerate(S):
        s.unchanged(f"{cid}: source {k}")
    ref, bound = pc.lincomb_ref([s.numpy() for s in src0], w)
    print(f"{cid}: worst error / bound {within(O.np64(), ref, bound, cid):.3f}")
    first = O.t.clone()
    O2 = Buf(n)
    lincomb(lib, O2, S, w, n)
    assert same_bits(O2.t, first), f"{cid}: two runs differ"
    if K == 33:  # consecutive groups of 8 (the last one of 1) continue one chain: the bits of the single launch
        G = Buf(n)
        for g0 in range(0, K, 8):
            lincomb(lib, G, S[g0:g0 + 8], w[g0:g0 + 8], n, flags=ACCUMULATE if g0 else 0)
        G.guards(f"{cid}: grouped")
        assert same_bits(G.t, first), f"{cid}: groups of 8 with ACCUMULATE differ from one launch"
        for k, s in enumerate(S):
            s.unchanged(f"{cid}: source {k} after the grouped run")


def test_lincomb_accumulate_starts_from_out(lib):
    n, K = 1027, 3
    w = pc.alternating_weights(K)
    src0, start = [randn(n, seed=7 + k) for k in range(K)], randn(n, seed=99)
    S, O = [Buf(n, s) for s in src0], Buf(n, start)
    lincomb(lib, O, S, w, n, flags=ACCUMULATE)
    O.guards("accumulate")
    ref, bound = pc.lincomb_ref([s.numpy() for s in src0], w, start=start.numpy())
    within(O.np64(), ref, bound, "lincomb accumulate")


def test_lincomb_refusals_write_nothing(lib):
    n, K = 64, 4
    src0, out0 = [randn(n, seed=k) for k in range(K)], randn(n, seed=50)
    S, O = [Buf(n, s) for s in src0], Buf(n, out0)
    ptr_host = torch.tensor([s.ptr() for s in S], dtype=torch.int64)
    w_host = torch.tensor([1.0, -1.0, 0.5, 0.25])
    ptr_dev, w_dev = ptr_host.to(DEV), w_host.to(DEV)

    def call(out=O.ptr(), ph=ptr_host, pd=ptr_dev.data_ptr(), wh=w_host.data_ptr(), wd=w_dev.data_ptr(), K=K, n=n, flags=0):
        return raw(lib, "dl_arena_lincomb", out, ph.data_ptr() if ph is not None else None, pd, wh, wd, K, n, flags, _s())

    def table(**change):
        t = ptr_host.clone()
        for k, v in change.items():
            t[int(k[1:])] = v
        return t

    cases = [dict(K=0), dict(K=257), dict(K=-1), dict(out=None), dict(ph=None), dict(pd=None), dict(wh=None), dict(wd=None), dict(n=0),
             dict(n=-3), dict(flags=2), dict(flags=3), dict(flags=-1), dict(ph=table(s1=0)), dict(ph=table(s2=S[2].ptr() + 4)),
             dict(ph=table(s3=O.ptr())), dict(out=O.ptr() + 4)]
    for kw in cases:
        rc = call(**kw)
        assert rc == INVALID and "dl_arena_lincomb" in lib.cdll.dl_last_error().decode(), (kw, rc)
    torch.cuda.synchronize()
    O.unchanged("refusals: out")
    for k, s in enumerate(S):
        s.unchanged(f"refusals: source {k}")
    assert call() == 0
    torch.cuda.synchronize()
    O.guards("after the refusals")


# ------------------------------------------------------------------------------------------------------------------ classes
DIT = dict(input_channels=4, output_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, mlp_ratio=4, patch_size=2, depth=2,
           n_classes=10, classifier_free=True)
UNET = dict(image_size=[16, 16], in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=[2],
            channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True, n_classes=10, classifier_free=True)
FAMILIES = ("dit", "unet")


def build(family: str, seed: int, precision: str | None = None, **change):
    from diffulab_amd import MMDiT, UNetModel

    torch.manual_seed(seed)
    m = MMDiT(simple_dit=True, **{**DIT, **change}) if family == "dit" else UNetModel(**{**UNET, **change})
    with torch.no_grad():
        for q in m.parameters():  # (zero-initialised output layers would make every forward 0)
            q.add_(0.02 * torch.randn(q.shape))
    if precision:
        m.set_precision(precision)
    return m.to(DEV)


def inputs(family: str):
    c = 4 if family == "dit" else 1
    return dict(x=randn(2 * c * 256, seed=11).view(2, c, 16, 16).to(DEV), timesteps=torch.tensor([0.3, 0.7], device=DEV),
                y=torch.tensor([1, 2], device=DEV))


class CallLog:
    """names of the C entry points called while it is installed"""

    def __init__(self, monkeypatch):
        from diffulab_amd import _lib

        self.names: list[str] = []
        L = _lib.lib()
        orig = L.call

        def spy(name, *args):
            self.names.append(name)
            return orig(name, *args)

        monkeypatch.setattr(L, "call", spy)

    def count(self, name: str) -> int:
        return self.names.count(name)


def arena(m) -> torch.Tensor:
    m.engine  # noqa: B018 -- flattens if needed
    return m._flat


@pytest.mark.parametrize("family", FAMILIES)
def test_power_ema_tracks_the_fp64_recursion(family, monkeypatch):
    """40 updates with the online arena perturbed in between.  Reference R_t = R_{t-1} + w_t (p_t - R_{t-1}) in fp64 on the same f32
    parameters p_t and the same f32 weights.  Bound: the device computes D_t = F_t(D_{t-1}) + delta_t with F_t(x) = (1 - w_t) x + w_t p_t
    and |delta_t| <= b_t, the three-rounding bound of one update evaluated at the device's own D_{t-1}; F_t is affine with slope
    1 - w_t in [0, 1], so |D_t - R_t| <= (1 - w_t) |D_{t-1} - R_{t-1}| + b_t.  B_1 = 0: the first update (w = 1) is an exact copy."""
    from diffulab_amd.training import PowerEMA

    m = build(family, seed=1)
    ema = PowerEMA(m, sigma_rels=(0.05, 0.10))
    flat = arena(m)
    n = flat.numel()
    gammas = [pc.gamma_of(s) for s in ema.sigma_rels]
    R = [None, None]
    B = [torch.zeros(n, dtype=torch.float64, device=DEV) for _ in gammas]
    log = CallLog(monkeypatch)
    gen = torch.Generator().manual_seed(2)
    u = pc.U
    for t in range(1, 41):
        flat.add_((torch.randn(n, generator=gen) * 1e-2).to(DEV))
        P = flat.double()
        prev = [arena(e).double() for e in ema.ema_models]
        ema.update()
        for k, g in enumerate(gammas):
            w = pc.weight32(t, g)
            if t == 1:
                assert w == 1.0
                R[k] = P.clone()
                continue
            d = w * (P - prev[k])
            b = u * (2.0 * d.abs() + (prev[k] + d).abs()) * (1.0 + u) ** 2 + 2.0 ** -149
            B[k] = (1.0 - w) * B[k] + b
            R[k] = R[k] + w * (P - R[k])
    assert ema.t == 40 and ema.calls == 40
    assert log.count("dl_ema_update_multi") == 40 and log.count("dl_ema_update") == 0
    for k, e in enumerate(ema.ema_models):
        err = (arena(e).double() - R[k]).abs()
        assert bool((err <= B[k]).all()), (family, k, float((err / B[k]).max()))
        print(f"{family} profile {ema.sigma_rels[k]}: worst error / bound {float((err / B[k].clamp_min(1e-300)).max()):.3f}, "
              f"worst error {float(err.max()):.2e}")
    assert not same_bits(arena(ema.ema_models[0]), arena(ema.ema_models[1]))


def test_power_ema_update_every_and_state_round_trip():
    from diffulab_amd.training import PowerEMA

    m = build("dit", seed=3)
    ema = PowerEMA(m, sigma_rels=(0.05, 0.10, 0.2), update_every=3, eval_sigma_rel=0.10)
    flat = arena(m)
    for i in range(10):
        flat.add_(randn(flat.numel(), seed=20 + i, scale=1e-2).to(DEV))
        ema.update()
    assert ema.calls == 10 and ema.t == 4  # calls 0, 3, 6, 9
    sd = ema.state_dict()
    sd = {**sd, "profiles": [{k: v.detach().cpu().clone() for k, v in p.items()} for p in sd["profiles"]]}
    other = PowerEMA(build("dit", seed=4), sigma_rels=(0.05, 0.10, 0.2), update_every=3, eval_sigma_rel=0.10)
    assert not same_bits(arena(other.ema_models[0]), arena(ema.ema_models[0]))
    other.load_state_dict(sd)
    assert other.t == 4 and other.calls == 10
    for a, b in zip(other.ema_models, ema.ema_models):
        arena(a)  # (every parameter is a view of the arena again; the alignment gaps between them belong to no profile's state)
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and same_bits(va, vb), ka
    assert other.ema_model is other.ema_models[1]


_SNAP: dict = {}


@pytest.fixture
def snapshots(tmp_path_factory):
    """per family, once: 64 updates of a PowerEMA(0.05, 0.10) over a perturbed model with a snapshot every 8 -> (directory, PowerEMA)"""
    def get(family: str):
        if family not in _SNAP:
            from diffulab_amd.training import PowerEMA

            d = tmp_path_factory.mktemp(f"phema_{family}")
            m = build(family, seed=5)
            ema = PowerEMA(m, sigma_rels=(0.05, 0.10))
            flat = arena(m)
            gen = torch.Generator().manual_seed(6)
            for _ in range(64):
                flat.add_((torch.randn(flat.numel(), generator=gen) * 1e-2).to(DEV))
                ema.update()
                if ema.t % 8 == 0:
                    ema.snapshot(d)
            _SNAP[family] = (d, ema)
        return _SNAP[family]
    return get


@pytest.mark.parametrize("family", FAMILIES)
def test_snapshots_and_synthesis(family, snapshots, monkeypatch):
    from diffulab_amd.training import posthoc_ema as ph

    d, ema = snapshots(family)
    rows = [json.loads(line) for line in (d / "phema_index.jsonl").read_text().splitlines()]
    assert len(rows) == 16 and sorted({r["t"] for r in rows}) == list(range(8, 65, 8))
    assert all(set(r) == {"t", "sigma_rel", "file"} and r["file"] == f"phema_{r['t']:09d}_{r['sigma_rel']:.3f}.pt" and (d / r["file"]).exists()
               for r in rows)
    last = torch.load(d / "phema_000000064_0.100.pt", weights_only=True)
    assert set(last) == set(ema.ema_models[1].state_dict())  # the checkpoint keys of ema.pt
    assert all(torch.equal(v, ema.ema_models[1].state_dict()[k].cpu()) for k, v in last.items())

    target = build(family, seed=7)
    log = CallLog(monkeypatch)
    coef = ph.synthesize(target, d, 0.075, group=3)
    assert log.count("dl_arena_lincomb") == 6  # 16 snapshots, 3 at a time
    used, t = ph.select_snapshots(ph.read_index(d), None)
    assert t == 64 and len(used) == 16 and coef.shape == (16,) and coef.dtype == np.float64
    want = pc.coefficients([r["t"] for r in used], [r["sigma_rel"] for r in used], 64, 0.075)[0]
    files = [torch.load(d / r["file"], weights_only=True) for r in used]
    assert np.abs(coef - want).max() <= 1e-6 * np.abs(want).max()
    got = {k: v.detach().cpu() for k, v in target.state_dict().items()}
    params = {k for k, _ in target.named_parameters()}
    worst = 0.0
    for name in got:
        if name in params:
            ref, bound = pc.lincomb_ref([f[name].numpy().reshape(-1) for f in files], coef)
            worst = max(worst, within(got[name].numpy().astype(np.float64).reshape(-1), ref, bound, f"{family}: {name}"))
        else:
            assert torch.equal(got[name], files[-1][name]), f"{family}: buffer {name} is not the latest snapshot's"
    print(f"{family}: synthesis worst error / bound {worst:.3f}, sum |coef| {np.abs(coef).sum():.3f}")
    first = arena(target).clone()
    target16 = build(family, seed=8)
    coef16 = ph.synthesize(target16, d, 0.075, group=16)
    assert np.array_equal(coef, coef16) and same_bits(arena(target16), first), "group 3 and group 16 differ"
    # a stored snapshot is reproduced exactly up to the coefficients' rounding: the one-hot case through the whole path
    ph.synthesize(target16, d, 0.10, t=32)
    stored = torch.load(d / "phema_000000032_0.100.pt", weights_only=True)
    for name in params:
        assert torch.allclose(target16.state_dict()[name].cpu(), stored[name], rtol=0, atol=1e-6 * float(stored[name].abs().max()) + 1e-12)
    with pytest.raises(ValueError, match="later than the last snapshot"):
        ph.synthesize(target, d, 0.075, t=65)
    other = dict(mlp_ratio=2) if family == "dit" else dict(model_channels=64)
    with pytest.raises(ValueError, match="snapshot_dir.*does not match the model"):
        ph.synthesize(build(family, seed=9, **other), d, 0.075)
    assert same_bits(arena(target), first)  # the refused calls wrote nothing


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("family", FAMILIES)
def test_forward_after_synthesis_sees_the_new_weights(family, precision, snapshots):
    """the arena is written through a raw pointer: bf16 weight shadows and captured graphs of the forwards made BEFORE the synthesis
    must not survive it.  Bit for bit against a fresh model that received the same weights through load_state_dict."""
    from diffulab_amd.training import posthoc_ema as ph

    d, _ = snapshots(family)
    kw = inputs(family)
    target = build(family, seed=10, precision=precision).eval()
    with torch.no_grad():
        before = target(**kw)["x"].clone()
        assert torch.equal(target(**kw)["x"], before)  # (a second call: whatever the module caches is now live)
    ph.synthesize(target, d, 0.075)
    fresh = build(family, seed=12, precision=precision).eval()
    fresh.load_state_dict({k: v.detach().cpu() for k, v in target.state_dict().items()})
    with torch.no_grad():
        got, want = target(**kw)["x"].clone(), fresh(**kw)["x"].clone()
        again = target(**kw)["x"].clone()
    assert bool(torch.isfinite(want).all()) and not torch.equal(got, before)
    assert same_bits(got, want), f"{family} {precision}: max difference {float((got - want).abs().max()):.3e}"
    assert same_bits(again, want)


# ------------------------------------------------------------------------------------------------------------------ trainer
def run_trainer(tmp_path, **kw):
    from diffulab_amd import Diffuser, MMDiT
    from diffulab_amd.datasets import SyntheticDataset
    from diffulab_amd.training import BaseTrainer, FusedAdamW

    torch.manual_seed(0)
    m = MMDiT(simple_dit=True, **DIT)
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=8, extra_args={"logits_normal": True})
    opt = FusedAdamW(m.parameters(), lr=2e-3, weight_decay=0.0)
    mk = lambda n, seed: DataLoader(SyntheticDataset(n, (4, 16, 16), 10, seed), batch_size=16, drop_last=True)  # noqa: E731
    tr = BaseTrainer(n_epoch=1, save_path=tmp_path, project_name="t", use_ema=True, ema_update_every=1, **kw)
    tr.train(diffuser=d, optimizer=opt, train_dataloader=mk(128, 1), val_dataloader=mk(32, 2), log_validation_images=False,
             p_classifier_free_guidance=0.1)
    return tmp_path / "t", m


def test_trainer_with_power_ema_writes_snapshots_and_checkpoints(tmp_path, monkeypatch):
    from diffulab_amd import MMDiT
    from diffulab_amd.training import PowerEMA

    log = CallLog(monkeypatch)
    out, m = run_trainer(tmp_path, ema_type="power", ema_snapshot_every=4)
    assert log.count("dl_ema_update_multi") == 8 and log.count("dl_ema_update") == 0  # 128 samples / 16 per batch
    rows = [json.loads(line) for line in (out / "phema" / "phema_index.jsonl").read_text().splitlines()]
    assert [(r["t"], r["sigma_rel"]) for r in rows] == [(4, 0.05), (4, 0.10), (8, 0.05), (8, 0.10)]
    assert all((out / "phema" / r["file"]).exists() for r in rows)
    metrics = [json.loads(line) for line in (out / "metrics.jsonl").read_text().splitlines()]
    val = [r["val/loss"] for r in metrics if "val/loss" in r]
    assert len(val) == 1 and np.isfinite(val[0])
    ema_sd = torch.load(out / "ema.pt", weights_only=True)
    plain = MMDiT(simple_dit=True, **DIT)
    plain.load_state_dict(ema_sd)  # strict: the denoiser's own keys
    state = torch.load(out / "ema_state.pt", weights_only=True)
    assert state["t"] == 8 and state["calls"] == 8 and state["sigma_rels"] == [0.05, 0.10] and len(state["profiles"]) == 2
    assert all(torch.equal(v, state["profiles"][0][k]) for k, v in ema_sd.items())  # ema.pt is the evaluation profile (the first)
    snap = torch.load(out / "phema" / "phema_000000008_0.050.pt", weights_only=True)
    assert all(torch.equal(v, snap[k]) for k, v in ema_sd.items())
    resumed = PowerEMA(plain.to(DEV))
    resumed.load_state_dict(state)
    assert resumed.t == 8 and all(torch.equal(v.cpu(), state["profiles"][1][k]) for k, v in resumed.ema_models[1].state_dict().items())


def test_trainer_default_keeps_the_classic_ema_calls(tmp_path, monkeypatch):
    log = CallLog(monkeypatch)
    out, _ = run_trainer(tmp_path)
    assert log.count("dl_ema_update") > 0
    assert log.count("dl_ema_update_multi") == 0 and log.count("dl_arena_lincomb") == 0
    assert (out / "ema.pt").exists() and not (out / "ema_state.pt").exists() and not (out / "phema").exists()


def test_example_prints_three_synthesised_widths():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "posthoc_ema.py"), "--train-steps", "48", "--snapshot-every", "8",
                        "--batch", "16"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("sigma_rel ")]
    assert len(lines) == 3, r.stdout
    for ln in lines:
        loss = float(ln.split("validation loss ")[1].split(",")[0])
        norm = float(ln.split("coefficient 1-norm ")[1])
        assert np.isfinite(loss) and np.isfinite(norm) and norm > 0.5, ln
