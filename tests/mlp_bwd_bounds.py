"""fp64 reference, element-wise bounds and the tile-ownership mirror of dl_mlp_dswiglu_recompute (csrc/mlp_bwd.hip); imported by
tests/test_mlp_bwd_bounds_host.py and tests/test_mlp_bwd_gpu.py, not a conftest.  Builds on tests/elementwise_bounds.py (GEMM
reference, store terms) and on the V arithmetic of tests/f32_bounds.py / tests/bf16_aux_bounds.py.

The kernel, per 256-row x 128-unit tile:
    u  = X Wp^T       f32 accumulation over K1, then ROUNDED TO bf16 (a = x1, b = x3 of every hidden unit) and kept in registers
    g  = dT W2t^T     f32 accumulation over K2, never rounded
    du[:, :F] = bf16((g * b) * dsilu_f(a))       du[:, F:] = bf16(g * silu_f(a))

Two bounds:
  sound  (du_sound)  a and b carry the accumulation error of their product AND the half bf16 ulp of their rounding, so the bound
                     holds for every accumulation order -- at the price of ~2^-9 relative per rounded factor.
  tight  (du_tight)  a and b are bf16 values the device already stored (the U of dl_gemm_nt_swiglu on the same X, Wp) and enter
                     exactly; only g is inexact.  What is left is half a bf16 ulp of du plus a few 2^-24 terms.  It holds only while
                     the recomputed u has the bits of the stored one.
"""

from __future__ import annotations

import torch

import elementwise_bounds as eb
from bf16_aux_bounds import b16, dsilu_dev, silu_dev
from f32_bounds import V, exact, mul

TBM, TU = 256, 128  # RC_TBM, RC_TU_DEFAULT
MIN_TILES = 64

# (M, F, K1, K2) of the GPU table (tests/test_mlp_bwd_gpu.py), what each reaches, and the workgroup caps it also runs under
CASES = [
    ((2048, 1024, 64, 64), "8 x 8 tiles, one per workgroup, one k-step per phase", (0, 8)),
    ((1280, 1792, 128, 64), "5 x 14 tiles, grid 64, csplit 2, two XCDs empty, K1 != K2", (0, 8, 20)),
    ((1280, 1664, 64, 192), "5 x 13 tiles, csplit 1, XCDs 5..7 empty", (0,)),
    ((256, 8192, 64, 64), "1 x 64 tiles: XCDs 0 and 1 only, four tiles per workgroup", (0, 8)),
    ((16384, 128, 384, 384), "64 x 1 tiles, production K, np_max 8", (0,)),
    ((2304, 1152, 64, 128), "9 x 9 tiles, grid 80, short last panel group", (0,)),
    ((8192, 768, 128, 128), "the tight case: u as dl_gemm_nt_swiglu stored it", (0,)),
]


# ------------------------------------------------------------------------------------------------------------------ reference + bounds
def unit_columns(F: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """columns of X Wp^T that hold x1 / x3 of hidden unit 0..F-1: the weight shadow is row-permuted, 32-row tile t holds x1 of
    units 16t .. 16t+15, then x3 of the same units (the library needs F % 16 == 0; for the host tests a ragged last group of
    n < 16 units holds its n x1 rows, then its n x3 rows)"""
    u = torch.arange(F, device=device)
    i1 = 32 * (u // 16) + u % 16
    return i1, i1 + (F - 16 * (u // 16)).clamp_max(16)


def du_from(a: V, b: V, g: V) -> tuple[torch.Tensor, torch.Tensor]:
    """(ref, bound) of du [M, 2F] from a = x1, b = x3 (as the kernel uses them) and g = dh, in the kernel's order v * b * dsilu_f(a)"""
    r1, e1 = b16(mul(mul(g, b), dsilu_dev(a)))
    r3, e3 = b16(mul(g, silu_dev(a)))
    return torch.cat([r1, r3], 1), torch.cat([e1, e3], 1)


def dh_ref(dT, W2t) -> V:
    return V(*eb.gemm_ref(dT, W2t))


def du_sound(X, Wp, dT, W2t) -> tuple[torch.Tensor, torch.Tensor]:
    """holds whatever the accumulation order of the two products is"""
    P, E = eb.gemm_ref(X, Wp)
    i1, i3 = unit_columns(Wp.shape[0] // 2, P.device)
    x1, e1, x3, e3 = P[:, i1], E[:, i1], P[:, i3], E[:, i3]
    a, b = V(x1, eb.store_bf16(x1, e1)), V(x3, eb.store_bf16(x3, e3))  # the kernel rounds u to bf16 before it uses it
    return du_from(a, b, dh_ref(dT, W2t))


def du_tight(Ustored, dT, W2t) -> tuple[torch.Tensor, torch.Tensor]:
    """u [M, 2F] = [x1 | x3] as bf16 values the device stored: exact inputs"""
    F = Ustored.shape[1] // 2
    return du_from(exact(Ustored[:, :F]), exact(Ustored[:, F:]), dh_ref(dT, W2t))


# ------------------------------------------------------------------------------------------------------------------ ownership mirror
def supported(M, F, K1, K2) -> bool:
    return not (M % TBM or F % TU or K1 % 64 or K2 % 64 or (M // TBM) * (F // TU) < MIN_TILES)


def wg_budget(n_cu: int, cap: int) -> int:
    """dl_wg_budget (csrc/elementwise.hip)"""
    n = cap if 0 < cap < n_cu else n_cu
    return max(n, 8)


def ownership(M: int, F: int, n_cu: int = 256, cap: int = 0) -> dict:
    """the launcher's grid and csplit and, per workgroup, the (tm, tn) tiles the kernel walks, in order"""
    panels, tiles_n = M // TBM, F // TU
    ntiles = panels * tiles_n
    grid = min(wg_budget(n_cu, cap), ntiles) & ~7
    csplit = 2 if tiles_n % 2 == 0 else 1
    GL = grid >> 3
    pgroups = 8 // csplit
    nc, np_max = tiles_n // csplit, (panels + pgroups - 1) // pgroups
    walks, np_of_xcd = [], [0] * 8
    for blk in range(grid):
        xcd, local = blk & 7, blk >> 3
        tm0, tn0 = (xcd // csplit) * np_max, (xcd % csplit) * nc
        np_ = min(max(panels - tm0, 0), np_max)
        np_of_xcd[xcd] = np_
        cnt = (np_ * nc - local + GL - 1) // GL if np_ * nc > local else 0
        walks.append([(tm0 + (local + t * GL) // nc, tn0 + (local + t * GL) % nc) for t in range(cnt)])
    return dict(grid=grid, csplit=csplit, ntiles=ntiles, panels=panels, tiles_n=tiles_n, np_max=np_max, nc=nc, walks=walks,
                np_of_xcd=np_of_xcd)


def assert_owned_once(own: dict) -> None:
    seen: dict = {}
    for w, walk in enumerate(own["walks"]):
        for t in walk:
            assert t not in seen, f"tile {t} owned by workgroups {seen[t]} and {w}"
            assert 0 <= t[0] < own["panels"] and 0 <= t[1] < own["tiles_n"], f"workgroup {w} walks tile {t} outside the grid"
            seen[t] = w
    assert len(seen) == own["ntiles"], f"{own['ntiles'] - len(seen)} tiles have no owner"


def situations(own: dict) -> set[str]:
    """which entries of the ownership checklist a launch reaches"""
    s = {f"csplit {own['csplit']}"}
    per_wg = [len(w) for w in own["walks"]]
    if any(n == 0 for n in own["np_of_xcd"]):
        s.add("empty XCD")
    if any(0 < n < own["np_max"] for n in own["np_of_xcd"]):
        s.add("short last panel group")
    if max(per_wg) >= 2:
        s.add(">= 2 tiles per workgroup")
    if max(per_wg) >= 4:
        s.add(">= 4 tiles per workgroup")
    if own["grid"] < own["ntiles"]:
        s.add("grid < ntiles")
    if own["ntiles"] >= 6 * own["grid"]:
        s.add("ntiles >= 6 grid")
    return s


CHECKLIST = {"csplit 1", "csplit 2", "empty XCD", "short last panel group", ">= 2 tiles per workgroup", ">= 4 tiles per workgroup",
             "grid < ntiles", "ntiles >= 6 grid"}
