"""dl_mlp_dswiglu_recompute (csrc/mlp_bwd.hip) element by element, with write guards.

Every case of the table in tests/mlp_bwd_bounds.py (the smallest shapes with M % 256 == 0, F % 128 == 0 and >= 64 tiles that reach
every situation of the kernel's per-XCD tile ownership, under the workgroup caps a data-parallel host sets as well)
  * reads operands whose leading-dimension gaps and trailing rows hold NaN (ldx != ldt), so a read past K or below M poisons du,
  * writes du into a window at column 8 of a poisoned allocation with lddu = 2F + 136, whose guards must come back bit for bit,
  * compares both halves of du with the fp64 reference within the sound bound of tests/mlp_bwd_bounds.py.
The tight case takes u as dl_gemm_nt_swiglu stored it for the same X and Wp: the recomputed u has to have those bits.
"""

from __future__ import annotations

import ctypes
import os
import re
import zlib

import pytest
import torch

import elementwise_bounds as eb
import mlp_bwd_bounds as mb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIGHT = (8192, 768, 128, 128)
LAUNCHES = [(shape, cap) for shape, _, caps in mb.CASES for cap in caps]


@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    L = _lib.lib()
    L.cdll.dl_lab_last_path.restype = ctypes.c_int
    return L


@pytest.fixture
def wg_cap(lib):
    """sets the thread's workgroup cap; 0 (no cap) again afterwards"""
    yield lambda n: lib.cdll.dl_lab_set_wg_cap(int(n))
    lib.cdll.dl_lab_set_wg_cap(0)


def _s():
    return torch.cuda.current_stream().cuda_stream


def _operands(shape):
    M, F, K1, K2 = shape
    g = torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(shape).encode()))

    def bf(rows, cols, std):
        return (torch.randn(rows, cols, generator=g, device=DEV) * std).to(BF)

    X = eb.operand(bf(M, K1, 1.0), K1 + 8)
    Wp = eb.operand(bf(2 * F, K1, K1**-0.5), K1 + 16)
    dT = eb.operand(bf(M, K2, 1.0), K2 + 24)  # ldx != ldt also where K1 == K2
    W2t = eb.operand(bf(F, K2, F**-0.5), K2 + 8)
    return X, Wp, dT, W2t


_REF = {}


def _case(shape):
    """operands and the sound (ref, bound), built once per shape and left unchanged"""
    if shape not in _REF:
        ops = _operands(shape)
        _REF[shape] = (ops, mb.du_sound(*ops))
    return _REF[shape]


def _window(M, F):
    return eb.Guarded(M, 2 * F, BF, DEV, left=8, ld=2 * F + 136)


def _launch(L, ops, dU, shape):
    M, F, K1, K2 = shape
    X, Wp, dT, W2t = ops
    return L.cdll.dl_mlp_dswiglu_recompute(X.data_ptr(), X.stride(0), Wp.data_ptr(), Wp.stride(0), dT.data_ptr(), dT.stride(0), W2t.data_ptr(),
                                           W2t.stride(0), dU.win.data_ptr(), dU.buf.stride(0), M, F, K1, K2, _s())


def _run(L, shape):
    ops, _ = _case(shape)
    dU = _window(shape[0], shape[1])
    rc = _launch(L, ops, dU, shape)
    assert rc == 0, L.cdll.dl_last_error().decode()
    torch.cuda.synchronize()
    return dU


def _check(dU, ref, bound, F, what):
    dU.check(what)
    eb.assert_within(dU.win[:, :F], ref[:, :F], bound[:, :F], tile=(256, 128), what=what + " du1 = dh x3 silu'(x1)")
    eb.assert_within(dU.win[:, F:], ref[:, F:], bound[:, F:], tile=(256, 128), what=what + " du3 = dh silu(x1)")


@pytest.mark.parametrize("shape,cap", LAUNCHES, ids=[f"{'x'.join(map(str, s))}-cap{c}" for s, c in LAUNCHES])
def test_recompute(lib, wg_cap, shape, cap):
    wg_cap(cap)
    dU = _run(lib, shape)
    _, (ref, bound) = _case(shape)
    _check(dU, ref, bound, shape[1], f"M,F,K1,K2={shape} cap {cap}")


def test_recomputed_u_has_the_bits_of_the_stored_u(lib):
    """the tight bound: x1, x3 exact as dl_gemm_nt_swiglu stored them, only dh inexact -- half a bf16 ulp and a few 2^-24 terms"""
    M, F, K1, K2 = TIGHT
    ops, _ = _case(TIGHT)
    X, Wp, dT, W2t = ops
    U, H = eb.Guarded(M, 2 * F, BF, DEV), eb.Guarded(M, F, BF, DEV)
    lib.call("dl_gemm_nt_swiglu", X.data_ptr(), X.stride(0), Wp.data_ptr(), Wp.stride(0), U.win.data_ptr(), U.buf.stride(0), H.win.data_ptr(),
             H.buf.stride(0), M, F, K1, _s())
    path = lib.cdll.dl_lab_last_path()
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "gemm_paths.h")).read()
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", text[text.index("enum DlGemmPath"):text.index("DL_PATH_COUNT")].split("{", 1)[1], flags=re.M)
    assert names[path].startswith("NT_BIG_"), names[path]
    dU = _run(lib, TIGHT)
    U.check("stored u")
    ref, bound = mb.du_tight(U.win, dT, W2t)
    _check(dU, ref, bound, F, f"tight M,F,K1,K2={TIGHT}")


def test_two_runs_give_the_same_bits(lib):
    shape = mb.CASES[1][0]
    a, b = _run(lib, shape), _run(lib, shape)
    assert torch.equal(a.buf.view(torch.int16), b.buf.view(torch.int16))


def _unsupported() -> int:
    text = open(os.path.join(ROOT, "include", "diffulab_hip.h")).read()
    return int(re.search(r"enum\s*\{[^}]*\bDL_ERR_UNSUPPORTED\s*=\s*(-?\d+)", text).group(1))


@pytest.mark.parametrize("shape", [(2000, 1024, 64, 64), (2048, 1000, 64, 64), (2048, 1024, 96, 64), (2304, 896, 64, 64)],
                         ids=["M2000", "F1000", "K1_96", "63tiles"])
def test_refusals(lib, shape):
    """no kernel for the shape: DL_ERR_UNSUPPORTED, and nothing written"""
    assert not mb.supported(*shape)
    M, F, K1, K2 = shape
    Fa = (F + 7) // 8 * 8  # (lddu and the operand rows stay 16-byte multiples: the refusal is about the shape alone)
    z = lambda r, c: eb.operand(torch.zeros(r, c, dtype=BF, device=DEV), (c + 15) // 8 * 8)  # noqa: E731
    ops = (z(M, K1), z(2 * Fa, K1), z(M, K2), z(Fa, K2))
    dU = eb.Guarded(M, 2 * Fa, BF, DEV, left=8, ld=2 * Fa + 136)
    rc = _launch(lib, ops, dU, shape)
    torch.cuda.synchronize()
    assert rc == _unsupported(), (rc, lib.cdll.dl_last_error().decode())
    assert "dl_mlp_dswiglu_recompute" in lib.cdll.dl_last_error().decode()
    assert bool(eb.is_poison(dU.buf).all()), "a refused call wrote to dU"
