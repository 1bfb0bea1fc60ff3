"""The activation-stationary GEMMs (csrc/gemm_stationary.hip): dl_gemm_nt_swiglu_stationary and dl_gemm_nt_ssq_stationary.

A workgroup keeps its 256-row activation panel in registers and streams the weight through an LDS ring.  Checked here:
  * bit equality of U, H and C with dl_gemm_nt_swiglu / dl_gemm_nt_ssq (same operand order, same summation order) on shapes both take;
  * every element against the fp64 reference and bounds of tests/elementwise_bounds.py on shapes the older kernels refuse: one panel
    and one stage, a ring that wraps many times, both bank swizzles (row pitch 256-byte aligned or not), both ring depths (K <= 384:
    three slots, above: two);
  * the panel loop of a capped grid, with ragged ownership, bit for bit against one workgroup per panel;
  * refusals that write nothing;
  * one DiT forward through the engine's call sites.
Operands live in poisoned allocations with 8 extra (NaN) columns per row, outputs in guarded windows.

The row statistics: ssq[m, t] = the sum of squares of the ROUNDED outputs of row m inside 384-wide tile t, summed in f32 -- compared
with torch's f32 row sum of the kernel's own C by the criterion of the dl_gemm_nt_ssq test in tests/test_row_gemm_gpu.py (relative
L2 < 1e-6), bit-reproducible run to run, and -- the kernel keeps the older kernel's grouping of the sum -- bit-equal to dl_gemm_nt_ssq
where both run.

The utilisation rule (panels must fill 0.7 of their rounds) applies to max_workgroups == 0; these shapes have far fewer than 256
panels, so the calls size their grid themselves: max_workgroups = the number of panels unless a case says otherwise.
"""

from __future__ import annotations

import ctypes

import pytest
import torch

import elementwise_bounds as eb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
UNSUPPORTED = -3


@pytest.fixture(scope="module")
def L():
    from diffulab_amd import _lib

    return _lib.lib()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _bf(seed, shape, std=1.0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV) * std).to(BF)


def _operands(M, N, K, seed):
    x = eb.operand(_bf(seed, (M, K)), K + 8)
    w = eb.operand(_bf(seed + 1, (N, K), K**-0.5), K + 8)
    return x, w


def Guarded(rows, cols, dtype):
    return eb.Guarded(rows, cols, dtype, DEV)


def swiglu_new(L, x, wp, M, F, K, with_u=True, wgs=None):
    U = Guarded(M, 2 * F, BF) if with_u else None
    H = Guarded(M, F, BF)
    rc = L.cdll.dl_gemm_nt_swiglu_stationary(_p(x), x.stride(0), _p(wp), wp.stride(0), _p(U.win) if U else None, U.buf.stride(0) if U else 0,
                                             _p(H.win), H.buf.stride(0), M, F, K, M // 256 if wgs is None else wgs, _s())
    torch.cuda.synchronize()
    return rc, U, H


def swiglu_old(L, x, wp, M, F, K, with_u=True):
    U = Guarded(M, 2 * F, BF) if with_u else None
    H = Guarded(M, F, BF)
    L.call("dl_gemm_nt_swiglu", _p(x), x.stride(0), _p(wp), wp.stride(0), _p(U.win) if U else None, U.buf.stride(0) if U else 0, _p(H.win),
           H.buf.stride(0), M, F, K, _s())
    torch.cuda.synchronize()
    return U, H


def ssq_new(L, a, w, M, N, K, tiles, wgs=None):
    C = Guarded(M, N, BF)
    S = eb.Guarded(M, tiles, torch.float32, DEV, left=0, right=0, ld=tiles)  # (no zero fill: the kernel stores)
    rc = L.cdll.dl_gemm_nt_ssq_stationary(_p(a), a.stride(0), _p(w), w.stride(0), _p(C.win), C.buf.stride(0), M, N, K, _p(S.win), tiles,
                                          M // 256 if wgs is None else wgs, _s())
    torch.cuda.synchronize()
    return rc, C, S


def ssq_of(C, tiles):
    """torch's f32 row sums of squares of the rounded outputs, per 384-wide tile (the last one may be narrower)"""
    c = C.float()
    return torch.stack([c[:, 384 * t : 384 * (t + 1)].square().sum(1) for t in range(tiles)], 1)


def rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def swiglu_reference(x, wp, F):
    P, E = eb.gemm_ref(x, wp)
    # the weight shadow is row-permuted: 32-column tile t holds x1 of hidden units 16t .. 16t+15, then x3 of the same units
    u = torch.arange(F, device=DEV)
    i1 = 32 * (u // 16) + u % 16
    r1, e1, r3, e3 = P[:, i1], E[:, i1], P[:, i1 + 16], E[:, i1 + 16]
    h, eh = eb.swiglu(r1, e1, r3, e3)
    return (h, eb.store_bf16(h, eh)), (torch.cat([r1, r3], 1), eb.store_bf16(torch.cat([r1, r3], 1), torch.cat([e1, e3], 1)))


# ------------------------------------------------------------------------------------------------- 1. equal to the existing kernels
@pytest.mark.parametrize("M,F,K,with_u", [(2048, 768, 384, True), (2048, 768, 384, False), (16384, 576, 384, True)])
def test_swiglu_outputs_equal_the_persistent_tile_kernels_bit_for_bit(L, M, F, K, with_u):
    x, wp = _operands(M, 2 * F, K, 11)
    U0, H0 = swiglu_old(L, x, wp, M, F, K, with_u)
    rc, U1, H1 = swiglu_new(L, x, wp, M, F, K, with_u)
    assert rc == 0, L.cdll.dl_last_error()
    H1.check("h")
    assert torch.equal(H1.win.view(torch.int16), H0.win.view(torch.int16))
    if with_u:
        U1.check("u")
        assert torch.equal(U1.win.view(torch.int16), U0.win.view(torch.int16))


def test_ssq_product_equals_the_persistent_tile_kernel_bit_for_bit_and_statistics_hold_its_bound(L):
    M, N, K, tiles = 16384, 1152, 384, 2
    a, w = _operands(M, N, K, 21)
    C0 = Guarded(M, N, BF)
    S0 = torch.zeros(M, tiles, device=DEV)
    L.call("dl_gemm_nt_ssq", _p(a), a.stride(0), _p(w), w.stride(0), _p(C0.win), C0.buf.stride(0), M, N, K, _p(S0), tiles, _s())
    rc, C1, S1 = ssq_new(L, a, w, M, N, K, tiles)
    assert rc == 0, L.cdll.dl_last_error()
    C1.check("C")
    S1.check("ssq")
    assert torch.equal(C1.win.view(torch.int16), C0.win.view(torch.int16))
    ref = ssq_of(C0.win, tiles)
    print("rel(ssq_new, ref)", rel(S1.win, ref), "rel(ssq_old, ref)", rel(S0, ref), "rel(new, old)", rel(S1.win, S0))
    assert rel(S1.win, ref) < 1e-6
    # the kernel keeps the grouping of dl_gemm_nt_ssq's sum (192 columns per lane half, the halves, the two 192-column sums): same bits
    assert torch.equal(S1.win.view(torch.int32), S0.view(torch.int32))
    rc, _, S2 = ssq_new(L, a, w, M, N, K, tiles)
    assert rc == 0 and torch.equal(S2.win.view(torch.int32), S1.win.view(torch.int32))  # no atomics: the same bits every run


# ------------------------------------------------------------------------------------------------- 2. against fp64
SHAPES = [(256, 64, 64), (512, 64, 128), (768, 192, 512), (256, 1536, 384)]  # (M, F, K); the ssq form runs (M, N = 2F, K)


@pytest.mark.parametrize("M,F,K", SHAPES)
def test_swiglu_against_fp64_on_shapes_the_tile_kernels_refuse(L, M, F, K):
    x, wp = _operands(M, 2 * F, K, 31)
    rc, U, H = swiglu_new(L, x, wp, M, F, K)
    assert rc == 0, L.cdll.dl_last_error()
    (h, hb), (u, ub) = swiglu_reference(x, wp, F)
    H.check("h")
    U.check("u")
    eb.assert_within(H.win, h, hb, tile=(32, 64), what="h")
    eb.assert_within(U.win, u, ub, tile=(32, 64), what="u")
    rc, U2, H2 = swiglu_new(L, x, wp, M, F, K, with_u=False)
    assert rc == 0 and torch.equal(H2.win.view(torch.int16), H.win.view(torch.int16))


@pytest.mark.parametrize("M,F,K", SHAPES)
def test_ssq_against_fp64_on_shapes_the_tile_kernel_refuses(L, M, F, K):
    N = 2 * F
    tiles = min(2, (N + 383) // 384)
    a, w = _operands(M, N, K, 41)
    rc, C, S = ssq_new(L, a, w, M, N, K, tiles)
    assert rc == 0, L.cdll.dl_last_error()
    C.check("C")
    S.check("ssq")
    ref, err = eb.gemm_ref(a, w)
    eb.assert_within(C.win, ref, eb.store_bf16(ref, err), tile=(32, 128), what="C")
    assert rel(S.win, ssq_of(C.win, tiles)) < 1e-6


# ------------------------------------------------------------------------------------------------- 3. the panel loop
@pytest.mark.parametrize("wgs", [1, 3])
def test_capped_grids_loop_over_their_panels_and_give_the_same_bits(L, wgs):
    """M = 1024 is four panels: one workgroup walks all four, three own 2 + 1 + 1; the weight ring runs on across the panel
    boundary.  The comparison is one workgroup per panel (max_workgroups = 4, no loop): with max_workgroups = 0 four panels do not
    fill 0.7 of a 256-CU round and the call is refused, which is asserted as well."""
    M, F, K = 1024, 192, 384
    x, wp = _operands(M, 2 * F, K, 51)
    rc, U0, H0 = swiglu_new(L, x, wp, M, F, K, wgs=4)
    assert rc == 0
    rc, U1, H1 = swiglu_new(L, x, wp, M, F, K, wgs=wgs)
    assert rc == 0
    U1.check("u")
    H1.check("h")
    assert torch.equal(U1.win.view(torch.int16), U0.win.view(torch.int16)) and torch.equal(H1.win.view(torch.int16), H0.win.view(torch.int16))
    (h, hb), _ = swiglu_reference(x, wp, F)
    eb.assert_within(H1.win, h, hb, tile=(32, 64), what="h")
    rc, C0, S0 = ssq_new(L, x, wp, M, 2 * F, K, 1, wgs=4)
    assert rc == 0
    rc, C1, S1 = ssq_new(L, x, wp, M, 2 * F, K, 1, wgs=wgs)
    assert rc == 0
    C1.check("C")
    assert torch.equal(C1.win.view(torch.int16), C0.win.view(torch.int16)) and torch.equal(S1.win.view(torch.int32), S0.win.view(torch.int32))
    assert swiglu_new(L, x, wp, M, F, K, wgs=0)[0] == UNSUPPORTED


# ------------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("M,F,K", [(256, 64, 576), (384, 64, 384), (256, 48, 384)])
def test_shapes_outside_the_rules_are_refused_and_nothing_is_written(L, M, F, K):
    x, wp = _operands(M, 2 * F, K, 61)
    rc, U, H = swiglu_new(L, x, wp, M, F, K, wgs=1)
    assert rc == UNSUPPORTED
    assert bool(eb.is_poison(U.buf).all()) and bool(eb.is_poison(H.buf).all())
    rc, C, S = ssq_new(L, x, wp, M, 2 * F, K, 1, wgs=1)
    assert rc == UNSUPPORTED
    assert bool(eb.is_poison(C.buf).all()) and bool(eb.is_poison(S.buf).all())


# ------------------------------------------------------------------------------------------------- 5. through the engine
def test_dit_forward_through_the_stationary_kernels_equals_the_present_path(monkeypatch):
    """Two DiT blocks at B = 24, N = 256, D = 384 (the smallest batch on the QK-norm-on-load path), issued from Python so that the
    test can hand the engine's three call sites a grid: 24 panels are far from 0.7 of a 256-CU round, so max_workgroups = 24 makes
    the shape eligible.  With only the MLP-up kernel swapped the prediction is bit-identical; with the qkv kernel swapped too it
    still is (the statistics carry the older kernel's bits), which also holds the bound of the block test in tests/test_dit_gpu.py
    (5e-3, the QK-norm-on-load path against the row-kernel path)."""
    import test_dit_gpu as td
    from diffulab_amd import ops

    kw = dict(input_channels=4, output_channels=4, inner_dim=384, embedding_dim=384, num_heads=6, mlp_ratio=4, patch_size=2, depth=2,
              n_classes=10, classifier_free=True)
    B = 24
    x0 = td.synth.normal("st.x0", (B, 4, 32, 32)).to(DEV)
    t, y = td.synth.uniform("st.t", (B,), lo=0.05, hi=0.95).to(DEV), td.synth.integers("st.y", (B,), 10).to(DEV)
    monkeypatch.setenv("DL_NATIVE_BLOCK", "0")
    swiglu0, ssq0 = ops.gemm_nt_swiglu, ops.gemm_nt_ssq
    took = {"swiglu": 0, "ssq": 0}

    def run(mlp, qkv):
        def swiglu(x, wp, u, h, **kw_):
            if mlp:
                rc = ops.lib().cdll.dl_gemm_nt_swiglu_stationary(_p(x), x.stride(0), _p(wp), wp.stride(0), _p(u), u.stride(0) if u is not None else 0,
                                                                 _p(h), h.stride(0), x.shape[0], h.shape[1], x.shape[1], B, _s())
                assert rc == 0
                took["swiglu"] += 1
                return True
            return swiglu0(x, wp, u, h)

        def ssq(a, w, out, s, **kw_):
            if qkv:
                rc = ops.lib().cdll.dl_gemm_nt_ssq_stationary(_p(a), a.stride(0), _p(w), w.stride(0), _p(out), out.stride(0), a.shape[0], w.shape[0],
                                                              a.shape[1], _p(s), s.shape[1], B, _s())
                assert rc == 0
                took["ssq"] += 1
                return True
            return ssq0(a, w, out, s)

        monkeypatch.setattr(ops, "gemm_nt_swiglu", swiglu)
        monkeypatch.setattr(ops, "gemm_nt_ssq", ssq)
        m, _ = td.build(kw, seed=3)
        m.eval()
        with torch.no_grad():
            pred = m(x=x0, timesteps=t, y=y)["x"].clone()
        torch.cuda.synchronize()
        return pred

    present, mlp_only, both = run(False, False), run(True, False), run(True, True)
    assert took["swiglu"] >= 4 and took["ssq"] >= 2
    assert torch.equal(mlp_only, present)
    print("rel(both, present)", td.rel(both, present))
    assert td.rel(both, present) < 5e-3
    assert torch.equal(both, present)
