"""Wide row kernels (1024 < D <= 4096, csrc/norm.hip *_rows_k) against fp64 references of the same bf16 / f32 inputs, element by
element: LayerNorm-modulate forward / backward (with and without the fused gated residual and the affine LayerNorm), the per-token
backward of the DDT decoder, the gated-residual backward and QK-RMSNorm + RoPE + head split forward / backward (row windows and
position tables).  Bounds follow the arithmetic, in the style of tests/elementwise_bounds.py: a row statistic over D terms in f32
carries c * D * 2^-24 of the magnitudes it sums, a column sum over R rows c * R * 2^-24, local f32 steps a few 2^-24 of their terms,
and a bf16 store half an ulp.  Outputs sit in NaN-poisoned buffers whose guard regions are checked bit for bit after the call.
The references, bounds and runners live in tests/row_bounds.py, shared with tests/test_row_paths_gpu.py (D <= 1024)."""

from __future__ import annotations

import pytest
import torch

from row_bounds import run_gate_bwd, run_ln_bwd, run_ln_bwd_tok, run_ln_fwd, run_qk

pytestmark = pytest.mark.gpu

WIDTHS = [1088, 1536, 2048, 3072, 4096]


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as o

    return o


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("gated", [False, True])
def test_ln_modulate_fwd(ops, D, affine, gated):
    run_ln_fwd(ops, D, 2, 100, affine, gated, seed=D)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("affine,fused,dres_on", [(False, False, False), (True, False, True), (False, True, True), (True, True, False)])
def test_ln_modulate_bwd(ops, D, affine, fused, dres_on):
    run_ln_bwd(ops, D, 2, 100, affine, fused, dres_on, seed=D + 7)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("affine,fused", [(False, False), (True, True), (True, False)])
def test_ln_modulate_bwd_tok(ops, D, affine, fused):
    run_ln_bwd_tok(ops, D, 200, affine, fused, seed=D + 11)


@pytest.mark.parametrize("D", WIDTHS)
def test_gate_bwd(ops, D):
    run_gate_bwd(ops, D, 3, 100, seed=D + 13)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("window", [False, True])
def test_qk_norm_rope(ops, D, window):
    run_qk(ops, 2, 100, D // 64, 64, 40 if window else 64, window, seed=D + 17, v_on=not window)


@pytest.mark.parametrize("D", [1088, 4096])
def test_one_row(ops, D):
    run_ln_fwd(ops, D, 1, 1, True, True, seed=3)
    run_ln_bwd(ops, D, 1, 1, True, True, True, seed=4)
    run_ln_bwd_tok(ops, D, 1, True, True, seed=5, n_part=1)
    run_gate_bwd(ops, D, 1, 1, seed=6)
    run_qk(ops, 1, 1, D // 64, 64, 64, False, seed=7)


def test_65536_rows_at_2048(ops):
    """256 samples of 256 tokens at D = 2048: grid-stride loops and split backward launches over many workgroups"""
    D, B, N = 2048, 256, 256
    run_ln_fwd(ops, D, B, N, False, True, seed=21)
    run_ln_bwd(ops, D, B, N, True, True, True, seed=22)
    run_gate_bwd(ops, D, B, N, seed=23)
    run_ln_bwd_tok(ops, D, B * N, True, False, seed=24, n_part=8)
    run_qk(ops, B, N, D // 64, 64, 64, False, seed=25)


@pytest.mark.parametrize("D", [1536, 4096])
def test_deterministic_forward_and_dx(ops, D):
    """row statistics are summed in a fixed order: two identical calls give the same bits (forward outputs and dx)"""
    def bits(d):
        return {k: v.clone().view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32) for k, v in d.items() if v is not None}

    for f, kw in ((run_ln_fwd, dict(affine=True, gated=True)), (run_ln_bwd, dict(affine=True, fused=True, dres_on=True))):
        a, b = (bits(f(ops, D, 4, 100, seed=31, check=False, **kw)) for _ in range(2))
        assert all(torch.equal(a[k], b[k]) for k in a), f.__name__
    a, b = (run_qk(ops, 4, 100, D // 64, 64, 64, False, seed=33, check=False) for _ in range(2))
    for k in ("q", "k", "v", "rrms", "dqkv"):
        assert torch.equal(a[k], b[k]), k


def test_narrow_rows_unchanged(ops):
    """D <= 1024 keeps the one-wave-per-row kernels: the same calls at D = 1024 and 512 meet the same bounds"""
    for D in (512, 1024):
        run_ln_fwd(ops, D, 2, 100, True, True, seed=41)
        run_ln_bwd(ops, D, 2, 100, True, True, True, seed=42)
        run_gate_bwd(ops, D, 2, 100, seed=43)
        run_qk(ops, 2, 100, D // 64, 64, 64, False, seed=44)
