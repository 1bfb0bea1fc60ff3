"""Every kernel of the 3x3 convolution weight gradient, element by element, with write guards.

dl_conv3x3_wgrad_tn (the pixel ranges meet in g through f32 atomics) and dl_conv3x3_wgrad_tn_parts (every range stores its own image;
the engine's form) pick among conv3x3_wgrad_halo_k in four geometries and the implicit-GEMM kernels gemm_tn_k<true> /
gemm_tn_big_k<true> by map, channel counts, CU count and workgroup cap.  One table of cases (conv_wgrad_bounds.CASES, shared with
tests/test_conv_wgrad_bounds_host.py, which runs an f32 emulation and its mutants on the same cases) drives both entry points on two
input classes; every run
  * checks the kernel the dispatcher took (dl_lab_last_wgrad_path) and the number of pixel ranges (dl_conv3x3_wgrad_tn_nparts)
    against the table -- both assume the 256 CUs of an MI355X,
  * compares every element with the fp64 reference: within the f32-accumulation bound on `gauss` inputs, EQUAL on `exact` inputs
    (small integers: f32 arithmetic is exact in any order, so a fault worth one pixel shows at any R),
  * reads x as a channel slice of a wider poisoned buffer with poisoned rows above and below, dY with a poisoned row gap and poisoned
    rows below its zero pad rows, the zero line inside a poisoned buffer, and writes into poisoned allocations whose guards must come
    back bit-identical.
The parts form is also run twice (bit-identical) and folded by ops.ConvFoldTable onto a non-zero gradient where the fold takes the
channel counts (Co % 32 == 0).  Refused calls must not write a byte.  The last tests assert that the table reached every path code.
"""

from __future__ import annotations

import ctypes
import os
import re
import zlib

import pytest
import torch

import conv_wgrad_bounds as wb
import elementwise_bounds as eb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL0 = 16  # the channel slice starts at this column of the wider x buffer
REACHED: set[str] = set()
WORST: dict[str, tuple[float, str]] = {}  # path -> largest |diff| / bound on gauss inputs
_CACHE: dict = {}  # the operands and references of the last (case, mode): shared by the two forms, never written


@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    L = _lib.lib()
    L.cdll.dl_lab_last_wgrad_path.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def n_cu(lib):
    cu, lds, hbm = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    arch = ctypes.create_string_buffer(64)
    lib.call("dl_device_info", 0, ctypes.byref(cu), ctypes.byref(lds), ctypes.byref(hbm), arch, 64)
    return cu.value


def _s():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


class Zero:
    """the zero line: 64 zeros inside a poisoned buffer"""

    def __init__(self):
        self.buf = eb.poison_(torch.empty(128, dtype=BF, device=DEV))
        self.line = self.buf[:64]
        self.line.zero_()

    def check(self, what):
        assert bool((_bits(self.line) == 0).all()) and bool(eb.is_poison(self.buf[64:]).all()), f"{what}: the zero line changed"


class Problem:
    """operands and fp64 references of one (case, input class), on the device"""

    def __init__(self, c: wb.Case, mode: str):
        x, dy, self.init = wb.make_inputs(c, mode, zlib.crc32(f"{c.id}-{mode}".encode()), DEV)
        self.xbuf, self.x = wb.x_operand(x, c.W, col0=COL0)
        self.dybuf, self.dy = wb.dy_operand(dy, c.R)
        self.xbits, self.dybits = _bits(self.xbuf).clone(), _bits(self.dybuf).clone()
        self.ref, self.bound = wb.reference(self.x, self.dy, c, self.init)
        self.ref0, self.bound0 = wb.reference(self.x, self.dy, c, None)

    def operands_unchanged(self):
        return torch.equal(_bits(self.xbuf), self.xbits) and torch.equal(_bits(self.dybuf), self.dybits)


def problem(c, mode) -> Problem:
    key = (c.id, mode)
    if key not in _CACHE:
        _CACHE.clear()
        _CACHE[key] = Problem(c, mode)
    return _CACHE[key]


def conv_args(c, P, Ci=None, R=None, Co=None, x_ptr=None):
    return (x_ptr or P.x.data_ptr(), P.x.stride(0), c.B, c.H, c.W, Ci or c.Ci, P.dy.data_ptr(), P.dy.stride(0), R or c.R, Co or c.Co)


def check(got, ref, bound, mode, path, what, Ci=None):
    """gauss: every element inside its bound; exact: every element equal.  Ci given (got is g[(tap, ci), co]): a failure names the taps
    whose rows are wrong and the channel and column ranges they span"""
    got = got.double()
    bad = (got != ref) if mode == "exact" else ~((got - ref).abs() <= bound)
    if not bool(bad.any()):
        return
    if Ci is not None:
        rows, cols = bad.any(1).nonzero().reshape(-1), bad.any(0).nonzero().reshape(-1)
        taps = sorted(set((rows // Ci).tolist()))
        what = (f"{what}: wrong rows in taps {[f'{t} (ky {t // 3}, kx {t % 3})' for t in taps]}, channels {int((rows % Ci).min())}.."
                f"{int((rows % Ci).max())}, columns {int(cols.min())}..{int(cols.max())}")
    if mode == "exact":
        r, col = divmod(int(bad.reshape(-1).nonzero()[0]), ref.shape[-1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements differ from the exact result, first [{r}, {col}] = "
                             f"{float(got[r, col])!r}, exact {float(ref[r, col])!r}")
    eb.assert_within(got, ref, bound, tile=wb.TILE.get(path, (128, 128)), what=what)


def note(path, got, ref, bound, what):
    r = wb.worst_ratio(got, ref, bound)
    if r > WORST.get(path, (-1.0, ""))[0]:
        WORST[path] = (r, what)


def run_atomic(L, c, P, mode):
    g = eb.Guarded(9 * c.Ci, c.Co, torch.float32, DEV, init=P.init)
    z = Zero()
    L.call("dl_conv3x3_wgrad_tn", *conv_args(c, P), g.win.data_ptr(), g.buf.stride(0), z.line.data_ptr(), c.max_wgs, _s())
    path = wb.PATHS[L.cdll.dl_lab_last_wgrad_path()]
    torch.cuda.synchronize()
    what = f"{c.id} {mode} atomic [{path}]"
    z.check(what)
    assert P.operands_unchanged(), f"{what}: an operand changed"
    g.check(what)
    if mode == "gauss":
        note(path, g.win, P.ref, P.bound, what)
    check(g.win, P.ref, P.bound, mode, path, what, Ci=c.Ci)
    return path, None


def run_parts(L, c, P, mode):
    from diffulab_amd import ops

    n = int(L.cdll.dl_conv3x3_wgrad_tn_nparts(c.H, c.W, c.Ci, c.Co, c.R, c.max_wgs))
    assert n >= 1
    M, ldg = 9 * c.Ci, c.Co + 8
    z = Zero()
    bufs = []
    for _ in range(2):
        buf = eb.poison_(torch.empty(n + 1, M, ldg, device=DEV))
        L.call("dl_conv3x3_wgrad_tn_parts", *conv_args(c, P), buf.data_ptr(), ldg, M * ldg, n, z.line.data_ptr(), c.max_wgs, _s())
        bufs.append(buf)
    path = wb.PATHS[L.cdll.dl_lab_last_wgrad_path()]
    torch.cuda.synchronize()
    what = f"{c.id} {mode} parts [{path}, {n} images]"
    z.check(what)
    assert P.operands_unchanged(), f"{what}: an operand changed"
    buf = bufs[0]
    imgs = buf[:n, :, :c.Co]
    fin = torch.isfinite(imgs)
    assert bool(fin.all()), f"{what}: {int((~fin).sum())} image elements not written (or NaN), images {sorted(set((~fin).nonzero()[:, 0].tolist()))}"
    assert bool(eb.is_poison(buf[:n, :, c.Co:]).all()), f"{what}: the ldg gap was written"
    assert bool(eb.is_poison(buf[n]).all()), f"{what}: image {n}, one past the last, was written"
    assert torch.equal(_bits(bufs[0]), _bits(bufs[1])), f"{what}: two runs differ"
    total = imgs.double().sum(0)
    if mode == "gauss":
        note(path, total, P.ref0, P.bound0, what)
    check(total, P.ref0, P.bound0, mode, path, what, Ci=c.Ci)
    if ops.ConvFoldTable.accepts(c.Co, c.Ci):  # the batched fold: dw[co, ci, ky, kx] += the images, added in image order
        dw0 = wb.to_dw(P.init, c.Ci)  # a non-zero gradient (integer-valued on exact inputs)
        dw = eb.Guarded(c.Co, 9 * c.Ci, torch.float32, DEV, left=0, right=0, ld=9 * c.Ci, init=dw0.reshape(c.Co, 9 * c.Ci))
        ops.ConvFoldTable([(imgs, dw.win.view(c.Co, c.Ci, 3, 3))]).run(clear=False)
        torch.cuda.synchronize()
        dw.check(what + " fold")
        assert torch.equal(_bits(buf), _bits(bufs[1])), f"{what}: the fold changed the images"
        fref, fbound = wb.fold_bound(P.ref0, P.bound0, dw0, c.Ci)
        check(dw.win, fref.reshape(c.Co, 9 * c.Ci), fbound.reshape(c.Co, 9 * c.Ci), mode, "fold", what + " fold")
    return path, n


RUN = {"atomic": run_atomic, "parts": run_parts}


@pytest.mark.parametrize("form", wb.FORMS)
@pytest.mark.parametrize("mode", wb.MODES)
@pytest.mark.parametrize("case", wb.CASES, ids=lambda c: c.id)
def test_conv_wgrad_path(lib, n_cu, case, mode, form):
    P = problem(case, mode)
    try:
        lib.cdll.dl_lab_set_wgrad_halo(case.halo)
        path, n = RUN[form](lib, case, P, mode)
    finally:
        lib.cdll.dl_lab_set_wgrad_halo(1)
    REACHED.add(path)
    if n_cu == 256:
        assert path == case.path, f"{case.id}: dispatched to {path}, the table expects {case.path}"
        assert n is None or n == case.nparts, f"{case.id}: {n} pixel ranges, the table expects {case.nparts}"


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refused_calls_write_nothing(lib):
    """every refusal of the two entry points, on live operands: the accumulating g and the image buffer keep every bit"""
    from diffulab_amd import ops

    tn, parts, nparts = (lib._fns[k][0] for k in ("dl_conv3x3_wgrad_tn", "dl_conv3x3_wgrad_tn_parts", "dl_conv3x3_wgrad_tn_nparts"))
    c = wb.Case(25, 8, 8, 128, 128, "WG_HALO_W8", 3)
    P = Problem(c, "gauss")
    z = Zero()
    M, ldg = 9 * c.Ci, c.Co + 8
    g = eb.Guarded(M, c.Co, torch.float32, DEV, init=P.init)
    before = _bits(g.buf).clone()
    room = 0  # images the buffer really holds: the largest count either dispatch asks for (a call that is wrongly taken stays inside)
    for halo in (1, 0):
        lib.cdll.dl_lab_set_wgrad_halo(halo)
        room = max(room, int(nparts(c.H, c.W, c.Ci, c.Co, c.R, 0)))
    lib.cdll.dl_lab_set_wgrad_halo(1)
    imgs = eb.poison_(torch.empty(room, M, ldg, device=DEV))
    gp, gl, zp = g.win.data_ptr(), g.buf.stride(0), z.line.data_ptr()

    def untouched(what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(g.buf), before), f"{what}: g was written"
        assert bool(eb.is_poison(imgs).all()), f"{what}: the images were written"
        z.check(what)

    try:
        for halo in (1, 0):
            lib.cdll.dl_lab_set_wgrad_halo(halo)
            n = int(nparts(c.H, c.W, c.Ci, c.Co, c.R, 0))
            assert n >= 2
            # Ci % 128 != 0: unsupported, not an error
            assert tn(*conv_args(c, P, Ci=64), gp, gl, zp, 0, _s()) == -3
            assert not ops.conv3x3_wgrad_tn(P.x[:, :64], c.B, c.H, c.W, 64, P.dy, c.Co, g.win, z.line)
            assert parts(*conv_args(c, P, Ci=64), imgs.data_ptr(), ldg, M * ldg, room, zp, 0, _s()) == -3
            assert int(nparts(c.H, c.W, 64, c.Co, c.R, 0)) == 0
            untouched(f"halo={halo} Ci=64")
            bad = {"R % 64 != 0": dict(R=c.R + 8), "R < B*H*W": dict(R=c.R - 64), "Co % 8 != 0": dict(Co=c.Co - 4),
                   "x not 16-byte aligned": dict(x_ptr=P.x.data_ptr() + 2)}
            for what, kw in bad.items():
                assert tn(*conv_args(c, P, **kw), gp, gl, zp, 0, _s()) == -1, what
                assert parts(*conv_args(c, P, **kw), imgs.data_ptr(), ldg, M * ldg, room, zp, 0, _s()) == -1, what
                untouched(f"halo={halo} {what}")
            assert tn(*conv_args(c, P), gp, c.Co - 8, zp, 0, _s()) == -1
            assert parts(*conv_args(c, P), imgs.data_ptr(), c.Co - 8, M * ldg, room, zp, 0, _s()) == -1
            untouched(f"halo={halo} ldg < Co")
            assert parts(*conv_args(c, P), imgs.data_ptr(), ldg, M * ldg, n - 1, zp, 0, _s()) == -1
            untouched(f"halo={halo} max_parts = nparts - 1")
            assert parts(*conv_args(c, P), imgs.data_ptr(), ldg, M * ldg - 1, room, zp, 0, _s()) == -1
            assert parts(*conv_args(c, P), imgs.data_ptr(), ldg, 0, room, zp, 0, _s()) == -1
            untouched(f"halo={halo} part_stride < 9*Ci*ldg")
    finally:
        lib.cdll.dl_lab_set_wgrad_halo(1)
    assert P.operands_unchanged()


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_path_enum_mirror():
    """conv_wgrad_bounds.PATHS mirrors enum DlConvWgradPath by name and order, and the table names every code"""
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "conv_wgrad_paths.h")).read()
    body = text[text.index("enum DlConvWgradPath"):text.index("WG_PATH_COUNT")]
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", body.split("{", 1)[1], flags=re.M)
    assert names == wb.PATHS
    assert {c.path for c in wb.CASES} == set(wb.PATHS[1:])


def test_every_path_code_is_reached(n_cu):
    """runs after the table (module order): every path code was taken by at least one case"""
    if n_cu != 256:
        pytest.skip(f"the expected codes assume 256 CUs, this device has {n_cu}")
    missing = set(wb.PATHS[1:]) - REACHED
    assert not missing, f"path codes no case reached: {sorted(missing)}"
    print(f"\nreached all {len(wb.PATHS) - 1} path codes; largest |diff| / bound on gauss inputs: "
          + "; ".join(f"{k} {r:.4f} ({w})" for k, (r, w) in sorted(WORST.items())))
