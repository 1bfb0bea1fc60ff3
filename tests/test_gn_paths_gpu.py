"""Every GroupNorm kernel form of csrc/unet.hip, element by element, with write guards.

dl_gn_stats, dl_gn_apply_fwd, dl_gn_fwd and dl_gn_bwd pick among 16 kernel forms by HW, C, C/G, B and the lab switch
dl_lab_set_gn_fused.  One table of cases drives them through the C ABI; every case runs all four entry points and
  * checks that each launched the expected form (dl_lab_last_gn_path, csrc/gn_paths.h),
  * compares every element of every output -- mean, rstd, out (both forward routes), dx, dw, db, dfilm_scale, dfilm_shift -- with the
    fp64 reference within its bound (tests/groupnorm_bounds.py; test_groupnorm_bounds_host.py shows what the bounds admit and reject),
  * writes into poisoned allocations with guards before and after (the statistics and the backward's scratch too), reads x / dout /
    dres from allocations that end in NaN rows, and FiLM operands and gradients as strided views (ld > C), as the engine passes them,
  * runs twice and compares bits: the statistics (fixed-order forms), both forward outputs, and dx / dfilm_* of the fused backward
    forms.  Excluded, because atomics feed them: dw / db everywhere (global f32 atomics over the samples), the statistics of the
    C > 2048 form (LDS atomics), and dx / dfilm_* of the three-launch backward (gn_bwd_reduce_k folds its waves with LDS atomics).
The last tests assert that the table reached every DlGnPath code and that PATHS mirrors the header.
"""

from __future__ import annotations

import ctypes
import os
import re
import zlib
from dataclasses import dataclass

import pytest
import torch

import elementwise_bounds as eb
import groupnorm_bounds as gb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_RANGES = 8  # DL_GN_BWD_MAX_RANGES
GUARD = 4096  # poisoned elements on each side of a dense output

# mirror of enum DlGnPath (diffulab_amd/csrc/gn_paths.h), by name: index = code
PATHS = ["DL_GN_PATH_NONE", "GN_FWD_FUSED_16_4", "GN_FWD_FUSED_12_4", "GN_FWD_FUSED_12_12", "GN_FWD_FUSED_8_4", "GN_FWD_FUSED_8_8",
         "GN_FWD_FUSED_8_32", "GN_STATS", "GN_STATS_ATOMIC", "GN_APPLY_FWD", "GN_BWD_FUSED_16_4", "GN_BWD_FUSED_8_0", "GN_BWD_FUSED_12_4",
         "GN_BWD_FUSED_12_0", "GN_BWD_FUSED_64_0", "GN_BWD_REDUCE_64", "GN_BWD_REDUCE_8"]
# channels per workgroup of a form: the tile of a failure message
SLAB = {"GN_FWD_FUSED_16_4": 128, "GN_FWD_FUSED_12_4": 96, "GN_FWD_FUSED_12_12": 96, "GN_FWD_FUSED_8_4": 64, "GN_FWD_FUSED_8_8": 64,
        "GN_FWD_FUSED_8_32": 64, "GN_APPLY_FWD": 8, "GN_BWD_FUSED_16_4": 128, "GN_BWD_FUSED_8_0": 64, "GN_BWD_FUSED_12_4": 96,
        "GN_BWD_FUSED_12_0": 96, "GN_BWD_FUSED_64_0": 512, "GN_BWD_REDUCE_64": 512, "GN_BWD_REDUCE_8": 64}
DEPTH = {"GN_FWD_FUSED_16_4": "fused16", "GN_FWD_FUSED_12_4": "fused12", "GN_FWD_FUSED_12_12": "fused12", "GN_FWD_FUSED_8_4": "fused8",
         "GN_FWD_FUSED_8_8": "fused8", "GN_FWD_FUSED_8_32": "fused8"}


@dataclass
class Case:
    B: int
    HW: int
    C: int
    G: int
    mode: int  # dl_lab_set_gn_fused
    fwd: str  # the form dl_gn_fwd must take (GN_APPLY_FWD: statistics + apply as two launches)
    bwd: str
    cls: str = ""  # input class; "" = by position in the table
    flags: int = -1  # bit 0 FiLM, bit 1 SiLU, bit 2 dres; -1 = by position

    @property
    def id(self):
        f = "".join(ch for k, ch in enumerate("fsr") if self.flags >> k & 1) or "plain"
        return f"B{self.B}-HW{self.HW}-C{self.C}-G{self.G}-m{self.mode}-{self.cls}-{f}"


def _cases():
    F16, F124, F1212, F84, F88, F832, AP = (PATHS[i] for i in (1, 2, 3, 4, 5, 6, 9))
    B16, B80, B124, B120, B640, R64, R8 = PATHS[10:17]
    # shapes follow the dispatch conditions of dl_gn_fwd / dl_gn_bwd (G = 32 unless C forbids):
    #   forward fused where B HW C >= 2^23 or HW >= 64 or mode 3:  HW <= 64, C % 128, cg | 128 -> <16,4>;  C % 96, cg | 96, cg !| 128,
    #   HW <= 252 -> <12,4> (HW <= 84) / <12,12>;  C % 64, cg | 64, cg >= 2, HW <= 1024 -> <8,4> (<= 128) / <8,8> (<= 256) / <8,32>
    #   backward: HW <= 64, C >= 512, cg | 128 -> <16,4>;  64 < HW <= 1024, cg | 64, B C/64 >= 128 or mode 3 -> <8,0>;  C % 96, cg | 96,
    #   HW <= 1024, B C/96 >= 128 or mode 3 -> <12,4> (HW <= 84) / <12,0>;  HW <= 64, C >= 512, cg | 512, cg >= 16 -> <64,0>;
    #   else reduce<64> (HW <= 64, C >= 512) or reduce<8> with min(1024 / (B slabs), HW / 64, 8) pixel ranges
    cs = [
        Case(4, 16, 32, 32, 1, AP, R8),         # cg 1: below every fused form; 1 range
        Case(8, 1, 64, 32, 1, AP, R8),          # HW 1: two elements per group
        Case(4, 64, 64, 32, 1, F84, R8),        # cg 2; HW 64 is not > 64: three launches
        Case(4, 65, 64, 32, 3, F84, B80),       # HW 65, mode 3 at small B
        Case(128, 128, 64, 32, 1, F84, B80),    # B C/64 = 128: the batch gate without mode 3; HW 128: last of <8,4>
        Case(2, 129, 128, 32, 1, F88, R8),      # cg 4; HW 129: first of <8,8>; 2 pixel ranges
        Case(2, 256, 256, 32, 1, F88, R8),      # cg 8; HW 256: last of <8,8>; 4 ranges
        Case(2, 257, 256, 32, 3, F832, B80),    # HW 257: first of <8,32>
        Case(1, 1024, 128, 32, 1, F832, R8),    # HW 1024: last of <8,32>; 8 ranges
        Case(1, 1025, 128, 32, 1, AP, R8),      # HW 1025: beyond the fused forward; 8 ranges of 129 pixels
        Case(1, 4096, 64, 32, 1, AP, R8),       # 64 x 64 map
        Case(64, 1024, 128, 32, 1, F832, B80),  # <8,0> at its largest map through the batch gate
        Case(4, 77, 256, 32, 3, F84, B80),      # the text-context norm: HW = L = 77
        Case(4, 16, 512, 32, 1, AP, B16),       # cg 16; small launch: forward stays two launches in mode 1
        Case(4, 16, 512, 32, 3, F16, B16),      # ... and fuses in mode 3
        Case(4, 16, 512, 32, 2, AP, B640),      # mode 2: 512-channel slabs
        Case(4, 16, 512, 32, 0, AP, R64),       # mode 0: the separate launches
        Case(4, 64, 1024, 32, 1, F16, B16),     # cg 32; HW 64: last of <16,4>
        Case(4, 64, 1024, 32, 0, AP, R64),      # mode 0 where mode 1 fuses both
        Case(2, 1, 2048, 32, 3, F16, B16),      # cg 64, HW 1
        Case(2, 16, 2048, 32, 2, AP, B640),     # cg 64, four 512-channel slabs
        Case(4, 16, 576, 9, 1, AP, B640),       # cg 64, C % 128 != 0: <64,0> in mode 1, second slab 64 channels wide
        Case(2, 16, 2560, 32, 1, AP, R64),      # C > 2048: the LDS-atomic statistics; cg 80, five slabs
        Case(2, 77, 2560, 32, 1, AP, R8),       # ... on 77 pixels
        Case(4, 16, 384, 32, 3, F124, B124),    # cg 12
        Case(4, 84, 384, 32, 3, F124, B124),    # HW 84 = 21 x 4: last of <12,4>
        Case(4, 85, 384, 32, 3, F1212, B120),   # HW 85: first of <12,12> / <12,0>
        Case(32, 252, 384, 32, 1, F1212, B120),  # HW 252: last of <12,12>; B C/96 = 128 without mode 3
        Case(2, 253, 384, 32, 1, AP, R8),       # HW 253: beyond <12,12>, cg 12 fits no 64-channel slab; 3 ranges
        Case(4, 64, 768, 32, 1, F124, R64),     # cg 24; B C/96 = 32: three launches on 512-channel slabs (768 = 512 + 256)
        Case(16, 64, 768, 32, 1, F124, B124),   # ... and B C/96 = 128
        Case(2, 77, 1536, 32, 3, F124, B124),   # cg 48, HW 77
        Case(4, 64, 320, 32, 1, AP, R8),        # cg 10: no fused form
        Case(4, 16, 640, 32, 1, AP, R64),       # cg 20: 512 + 128 channels
    ]
    for i, c in enumerate(cs):
        c.cls, c.flags = gb.CLASSES[i % 5], (7, 2, 5, 3, 0, 6, 1, 4)[i % 8]
    # the offset classes once more on every fused-forward form and both streaming forms (whatever the rotation above gave them)
    extra = [Case(4, 64, 1024, 32, 1, F16, B16, "offset32", 7), Case(4, 84, 384, 32, 3, F124, B124, "offset32", 3),
             Case(4, 252, 384, 32, 3, F1212, B120, "offset32", 5), Case(4, 128, 64, 32, 3, F84, B80, "offset32", 6),
             Case(2, 256, 256, 32, 3, F88, B80, "offset32", 7), Case(1, 1024, 128, 32, 3, F832, B80, "offset32", 2),
             Case(2, 77, 2560, 32, 1, AP, R8, "offset32", 1), Case(1, 4096, 64, 32, 1, AP, R8, "offset32", 4),
             Case(4, 64, 1024, 32, 1, F16, B16, "const", 2), Case(4, 16, 384, 32, 3, F124, B124, "offset4", 6)]
    ids = [c.id for c in cs]
    return cs + [c for c in extra if c.id not in ids]


CASES = _cases()
REACHED: set[str] = set()
WORST: dict[str, tuple[float, str]] = {}


# ------------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    L = _lib.lib()
    L.cdll.dl_lab_last_gn_path.restype = ctypes.c_int
    return L


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _path(L):
    code = L.cdll.dl_lab_last_gn_path()
    name = PATHS[code] if 0 <= code < len(PATHS) else f"<{code}>"
    REACHED.add(name)
    return name


class Dense:
    """a dense tensor between two runs of GUARD poisoned elements (init None: the tensor starts poisoned too)"""

    def __init__(self, shape, dtype, init=None):
        n = 1
        for s in shape:
            n *= s
        self.buf = eb.poison_(torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV))
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def check(self, what, finite=True):
        assert bool(eb.is_poison(self.buf[:GUARD]).all()) and bool(eb.is_poison(self.buf[-GUARD:]).all()), f"{what}: guard written"
        if finite:
            assert bool(torch.isfinite(self.t.float()).all()), f"{what}: unwritten or non-finite elements"


def _rows(values):
    """[B, HW, C] values as dense rows of an allocation that ends in two NaN rows: a read past the last sample hits NaN"""
    B, HW, C = values.shape
    return eb.operand(values.reshape(B * HW, C), C).view(B, HW, C)


def _within(case, what, got, ref, bound, tile):
    """every element inside its bound; the worst |diff| / bound per output is kept for the report of the last test"""
    ratio = gb.worst_ratio(got, ref, bound)
    print(f"{case.id}: {what} worst |diff| / bound {ratio:.3f}")
    if ratio > WORST.get(what, (-1.0, ""))[0]:
        WORST[what] = (ratio, case.id)
    g2, r2, b2 = (t.reshape(-1, t.shape[-1]) for t in (got, ref, bound))
    eb.assert_within(g2, r2, b2, tile=tile, what=f"{case.id}: {what}")


def run_case(L, c: Case):
    """all four entry points on one shape; -> the outputs two runs must agree on bit for bit"""
    B, HW, C, G = c.B, c.HW, c.C, c.G
    cg = C // G
    film, silu, use_dres = bool(c.flags & 1), bool(c.flags & 2), bool(c.flags & 4)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(zlib.crc32(c.id.encode()))
    n = lambda *s: torch.randn(s, generator=gen, device=DEV)  # noqa: E731
    x = _rows(gb.make_x(c.cls, B, HW, C, G, gen, DEV))
    dout = _rows(n(B, HW, C).to(BF))
    dres = _rows(n(B, HW, C).to(BF)) if use_dres else None
    w, b = 1.0 + 0.2 * n(C), 0.2 * n(C)
    sc = sh = None
    ldf = 2 * C + 16
    if film:  # two column windows of one poisoned [B + 2, 2 C + 16] allocation (the engine passes halves of one projection's rows)
        fbuf = eb.poison_(torch.empty(B + 2, ldf, dtype=BF, device=DEV))
        sc, sh = fbuf[:B, :C], fbuf[:B, C + 8:2 * C + 8]
        sc.copy_(0.3 * n(B, C))
        sh.copy_(0.3 * n(B, C))
    dw0, db0 = n(C), n(C)
    reproducible = []
    L.cdll.dl_lab_set_gn_fused(c.mode)
    try:
        # ---- statistics + apply as two calls
        st = Dense((B, G, 2), torch.float32)
        L.call("dl_gn_stats", _p(x), _p(st.t), B, HW, C, G, gb.EPS, _s())
        p_stats = _path(L)
        assert p_stats == ("GN_STATS" if C <= 2048 else "GN_STATS_ATOMIC"), (c.id, p_stats)
        out = Dense((B, HW, C), BF)
        L.call("dl_gn_apply_fwd", _p(x), _p(st.t), _p(w), _p(b), _p(sc), _p(sh), ldf, int(silu), _p(out.t), B, HW, C, G, _s())
        assert _path(L) == "GN_APPLY_FWD", c.id
        # ---- one call
        st1, out1 = Dense((B, G, 2), torch.float32), Dense((B, HW, C), BF)
        L.call("dl_gn_fwd", _p(x), _p(w), _p(b), _p(sc), _p(sh), ldf, int(silu), _p(out1.t), _p(st1.t), B, HW, C, G, gb.EPS, _s())
        p_fwd = _path(L)
        assert p_fwd == c.fwd, f"{c.id}: dl_gn_fwd took {p_fwd}, expected {c.fwd}"
        # ---- backward, from the statistics of the one-call forward; dw / db start from non-zero values (+= semantics)
        dx, dw, db = Dense((B, HW, C), BF), Dense((C,), torch.float32, init=dw0), Dense((C,), torch.float32, init=db0)
        scr = Dense((MAX_RANGES * B * 4 * C + B * G * 2,), torch.float32)
        dfs = dfh = None
        if film:
            dfs, dfh = (eb.Guarded(B, C, BF, DEV, ld=ldf) for _ in range(2))
        L.call("dl_gn_bwd", _p(dout), _p(x), _p(st1.t), _p(w), _p(b), _p(sc), _p(sh), ldf, int(silu), _p(dres), _p(dx.t), _p(dw.t),
               _p(db.t), _p(dfs.win if film else None), _p(dfh.win if film else None), ldf, _p(scr.t), B, HW, C, G, _s())
        p_bwd = _path(L)
        assert p_bwd == c.bwd, f"{c.id}: dl_gn_bwd took {p_bwd}, expected {c.bwd}"
        torch.cuda.synchronize()
    finally:
        L.cdll.dl_lab_set_gn_fused(1)
    # ---- footprints
    for o, what in ((st, "stats"), (out, "out"), (st1, "stats (dl_gn_fwd)"), (out1, "out (dl_gn_fwd)"), (dx, "dx"), (dw, "dw"), (db, "db")):
        o.check(f"{c.id}: {what}")
    scr.check(f"{c.id}: scratch", finite=False)
    if film:
        dfs.check(f"{c.id}: dfilm_scale")
        dfh.check(f"{c.id}: dfilm_shift")
    # ---- forward, both routes
    gtile = max(1, SLAB.get(p_fwd, 64) // cg)
    for route, s_, o_, form in (("two calls", st, out, "stats" if C <= 2048 else "stats_atomic"), ("one call", st1, out1, DEPTH.get(p_fwd))):
        if form is None:  # dl_gn_fwd went through the same two launches
            form = "stats" if C <= 2048 else "stats_atomic"
        ref = gb.fwd_ref(x, w, b, sc, sh, silu, G, gb.EPS, gb.stats_depth(form, HW, C, G))
        _within(c, f"mean [{form}]", s_.t[..., 0], *ref["mean"], tile=(1, gtile))
        _within(c, f"rstd [{form}]", s_.t[..., 1], *ref["rstd"], tile=(1, gtile))
        _within(c, "out", o_.t, *ref["out"], tile=(HW, SLAB["GN_APPLY_FWD" if route == "two calls" else p_fwd]))
    # dl_gn_fwd returns what dl_gn_stats + dl_gn_apply_fwd return
    assert eb.rel_l2(st1.t, st.t.double()) < 1e-5, f"{c.id}: statistics of the two forward routes differ"
    # ---- backward
    ref = gb.bwd_ref(dout, x, st1.t, w, b, sc, sh, silu, dres, dw0, db0, G)
    _within(c, "dx", dx.t, *ref["dx"], tile=(HW, SLAB[p_bwd]))
    _within(c, "dw", dw.t[None, :], ref["dw"][0][None, :], ref["dw"][1][None, :], tile=(1, SLAB[p_bwd]))
    _within(c, "db", db.t[None, :], ref["db"][0][None, :], ref["db"][1][None, :], tile=(1, SLAB[p_bwd]))
    if film:
        _within(c, "dfilm_scale", dfs.win, *ref["dfilm_scale"], tile=(1, SLAB[p_bwd]))
        _within(c, "dfilm_shift", dfh.win, *ref["dfilm_shift"], tile=(1, SLAB[p_bwd]))
    reproducible = [out.t, out1.t]
    if C <= 2048:
        reproducible += [st.t, st1.t]
    if "FUSED" in p_bwd:
        reproducible += [dx.t] + ([dfs.win.contiguous(), dfh.win.contiguous()] if film else [])
    return reproducible


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gn_path(lib, case):
    first = run_case(lib, case)
    second = run_case(lib, case)  # the same inputs again
    assert len(first) == len(second)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(eb._int_view(a), eb._int_view(b)), f"{case.id}: reproducible output {i} differs between two runs"


def test_table_covers_the_issue():
    """the table holds every C/G, every side of every HW threshold and every lab mode it was written for"""
    assert {c.C // c.G for c in CASES} >= {1, 2, 4, 8, 10, 12, 16, 20, 24, 32, 48, 64}
    assert {c.HW for c in CASES} >= {1, 16, 64, 65, 77, 84, 85, 128, 129, 252, 253, 256, 257, 1024, 1025, 4096}
    assert {c.mode for c in CASES} == {0, 1, 2, 3} and max(c.C for c in CASES) > 2048
    assert {c.cls for c in CASES} == set(gb.CLASSES) and {c.flags for c in CASES} == set(range(8))
    assert len({c.id for c in CASES}) == len(CASES)


def test_path_enum_mirror():
    """PATHS mirrors enum DlGnPath by name and order"""
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "gn_paths.h")).read()
    body = text[text.index("enum DlGnPath"):text.index("DL_GN_PATH_COUNT")]
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", body.split("{", 1)[1], flags=re.M)
    assert names == PATHS


def test_every_gn_path_code_is_reached():
    """runs after the table (module order): every DlGnPath code was taken"""
    print(f"\n{len(CASES)} cases; worst |diff| / bound: " + "; ".join(f"{o} {r:.3f} ({cid})" for o, (r, cid) in sorted(WORST.items())))
    missing = set(PATHS[1:]) - REACHED
    assert not missing, f"GroupNorm path codes no case reached: {sorted(missing)}"
    print(f"reached all {len(PATHS) - 1} GroupNorm path codes")
