"""The one-wave-per-row kernels of csrc/norm.hip (D <= 1024: ln_mod_fwd_k, ln_mod_bwd_k / _wide_k, ln_mod_bwd_tok_k, gate_bwd_k,
qk_norm_rope_fwd_k, qk_norm_rope_bwd_k / _wide_k, qk_norm_rope_bwd_inplace_k + fold_rows_k) element by element against the fp64
references and bounds of tests/row_bounds.py, in NaN-poisoned buffers with checked guards.  (gate_bwd_k runs the row loop it shares
with gate_bwd_rows_k, gate_bwd_rows<64>; the QK kernels rotate through rope_rotate / rope_rotate_t.)

Widths: 64 (8 of a wave's 64 lanes hold a chunk), 384 (48 lanes: the benchmark), 512 (a full wave), 520 (two chunks per lane, one
lane in the second), 576, 768, 1024.  Row counts reach every launch shape of the per-sample backward (rows_wg 32 and 64, split 1, 4,
6, 8 meeting in global atomics, token counts the share does not divide, one row), the grid caps and grid-stride loops of the forward
and the QK kernels, and the per-token backward around one 64-row workgroup."""

from __future__ import annotations

import pytest
import torch

from row_bounds import run_gate_bwd, run_ln_bwd, run_ln_bwd_tok, run_ln_fwd, run_qk, run_qk_inplace

pytestmark = pytest.mark.gpu

WIDTHS = [64, 384, 512, 520, 576, 768, 1024]
HEADS = [(1, 64), (6, 64), (8, 64), (5, 104), (9, 64), (12, 64), (16, 64)]  # (H, dh): the same widths for the QK kernels
FORMS = [(False, False, False), (True, False, True), (False, True, True), (True, True, False)]  # affine, fused gate, dres
# (B, N) of dl_ln_modulate_bwd: rows_wg 32 / split 8, split 6, split 1, not divisible (one workgroup per sample), single rows
BWD_ROWS = [(2, 256), (2, 192), (3, 64), (2, 100), (2, 160), (5, 1), (1, 1)]


@pytest.fixture(scope="module")
def ops():
    from diffulab_amd import ops as o

    return o


def bits(d):
    return {k: v.clone().view(torch.int16 if v.dtype == torch.bfloat16 else torch.int32) for k, v in d.items() if torch.is_tensor(v)}


# ------------------------------------------------------------------------------------------------ LayerNorm + modulate
@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("affine", [False, True])
@pytest.mark.parametrize("gated", [False, True])
def test_ln_modulate_fwd(ops, D, affine, gated):
    run_ln_fwd(ops, D, 2, 100, affine, gated, seed=D)
    run_ln_fwd(ops, D, 1, 1, affine, gated, seed=D + 1)


def test_ln_modulate_fwd_grid_stride(ops):
    """M = 16640 rows > 4 x 4096: the capped grid walks its rows in a loop"""
    run_ln_fwd(ops, 64, 65, 256, True, True, seed=2)
    run_ln_fwd(ops, 64, 65, 256, False, False, seed=3)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("B,N", BWD_ROWS)
def test_ln_modulate_bwd_rows(ops, D, B, N):
    """every launch shape at every width, all fusions on, += on non-zero dscale / dshift / dgate / dwb"""
    run_ln_bwd(ops, D, B, N, True, True, True, seed=D + N, init=True)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("affine,fused,dres_on", FORMS)
def test_ln_modulate_bwd_forms(ops, D, affine, fused, dres_on):
    """the affine / fused-gate / dres combinations on a split launch (2 x 256) and on an undivided one (2 x 100)"""
    run_ln_bwd(ops, D, 2, 256, affine, fused, dres_on, seed=D + 7)
    run_ln_bwd(ops, D, 2, 100, affine, fused, dres_on, seed=D + 8)


@pytest.mark.parametrize("affine,fused,dres_on", FORMS)
def test_ln_modulate_bwd_64_row_shares(ops, affine, fused, dres_on):
    """64 samples of 256 tokens at D = 384: M / 64 = 256 workgroups' worth of rows, so rows_wg 64 and split 4"""
    run_ln_bwd(ops, 384, 64, 256, affine, fused, dres_on, seed=17, init=affine)


@pytest.mark.parametrize("D", [64, 384, 576, 1024])
@pytest.mark.parametrize("M", [1, 63, 64, 200])
@pytest.mark.parametrize("n_part", [1, 3])
def test_ln_modulate_bwd_tok(ops, D, M, n_part):
    for affine, fused in ((False, False), (True, True), (True, False)):
        run_ln_bwd_tok(ops, D, M, affine, fused, seed=D + M, n_part=n_part)


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("B,N", [(3, 100), (2, 256), (1, 1)])
def test_gate_bwd(ops, D, B, N):
    run_gate_bwd(ops, D, B, N, seed=D + N)


# ------------------------------------------------------------------------------------------------ QK RMSNorm + RoPE
@pytest.mark.parametrize("H,dh", HEADS)
@pytest.mark.parametrize("B,N", [(2, 100), (1, 1)])
def test_qk_norm_rope(ops, H, dh, B, N):
    run_qk(ops, B, N, H, dh, dh, False, seed=H * dh + N)


@pytest.mark.parametrize("H,dh,rot", [(1, 64, 40), (6, 64, 40), (8, 64, 16), (5, 104, 64), (9, 64, 40), (16, 64, 32), (4, 32, 16)])
@pytest.mark.parametrize("window", [False, True])
def test_qk_norm_rope_partial_rotation(ops, H, dh, rot, window):
    """rot < dh; window: rows [n_off, n_off + N) of longer q / k / v, a position table, no v output"""
    run_qk(ops, 2, 100, H, dh, rot, window, seed=H * dh + rot, v_on=not window)


@pytest.mark.parametrize("H,dh,B,N", [(6, 64, 65, 256), (16, 64, 65, 256), (1, 64, 65, 256), (1, 64, 100, 656)])
def test_qk_norm_rope_capped_grids(ops, H, dh, B, N):
    """M = 16640: the backward's grid is capped at 1024 with 4 rows per wave; M = 65600 at D = 64: 16 rows per wave, capped, looping"""
    run_qk(ops, B, N, H, dh, dh, False, seed=B + N)


@pytest.mark.parametrize("H,dh,rot", [(1, 64, 64), (6, 64, 64), (8, 64, 64), (6, 64, 40), (4, 32, 16)])
@pytest.mark.parametrize("B,N", [(2, 100), (1, 1), (65, 256)])
def test_qk_norm_rope_bwd_inplace(ops, H, dh, rot, B, N):
    assert run_qk_inplace(ops, B, N, H, dh, rot, with_pos=False, seed=H * dh + N)["ok"]


def test_qk_norm_rope_bwd_inplace_65600_rows_and_positions(ops):
    assert run_qk_inplace(ops, 100, 656, 1, 64, 64, with_pos=False, seed=5)["ok"]  # 16 rows per wave, 768 workgroups, the loop
    assert run_qk_inplace(ops, 2, 100, 6, 64, 64, with_pos=True, seed=6)["ok"]


def test_qk_norm_rope_bwd_inplace_refuses_576(ops):
    res = run_qk_inplace(ops, 2, 100, 9, 64, 64, with_pos=False, seed=7)
    assert res["ok"] is False
    assert torch.equal(res["dqkv"].view(torch.int16), res["g_in"].view(torch.int16)), "a refused call changed dqkv"
    assert torch.equal(res["dscale"], res["i_sc"]), "a refused call changed dscale"


# ------------------------------------------------------------------------------------------------ determinism
@pytest.mark.parametrize("D", [384, 520, 1024])
def test_deterministic_forward_and_dx(ops, D):
    """row statistics are summed in a fixed order: two identical calls give the same bits (forward outputs, mean, rstd, rrms, dx)"""
    for f, kw in ((run_ln_fwd, dict(affine=True, gated=True)), (run_ln_bwd, dict(affine=True, fused=True, dres_on=True))):
        a, b = (bits(f(ops, D, 4, 256, seed=31, check=False, **kw)) for _ in range(2))
        assert a and all(torch.equal(a[k], b[k]) for k in a), f.__name__
    H, dh = (5, 104) if D == 520 else (D // 64, 64)
    a, b = (run_qk(ops, 4, 100, H, dh, dh, False, seed=33, check=False) for _ in range(2))
    for k in ("q", "k", "v", "rrms", "dqkv"):
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("H,dh", [(1, 64), (6, 64), (8, 64)])
def test_inplace_backward_is_deterministic(ops, H, dh):
    """the scale gradients are folded in a fixed order: dqkv AND dscale come back with the same bits"""
    a, b = (bits(run_qk_inplace(ops, 65, 256, H, dh, dh, with_pos=False, seed=35, check=False)) for _ in range(2))
    for k in ("dqkv", "dscale"):
        assert torch.equal(a[k], b[k]), k
