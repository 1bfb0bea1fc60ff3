"""Every dispatch branch of the GEMM family, element by element, with write guards.

dl_gemm_nt (+ _f32_det, _pair, the fused-SwiGLU tilings), dl_gemm_tn_ex / _det / _group and dl_conv3x3_nt each pick among many
kernels by shape, CU count and epilogue.  One table of cases drives them; every case
  * checks that the dispatcher took the expected kernel (dl_lab_last_path; the codes assume the 256 CUs of an MI355X),
  * compares every output element with an fp64 reference within an error bound derived from what the kernel computes
    (tests/elementwise_bounds.py),
  * runs on operands whose leading-dimension gaps and trailing rows hold NaN (a read past K poisons the output) and writes into
    windows of poisoned allocations, whose guard rows and columns must come back bit-identical.
The last test asserts that the table reached every path code.
"""

from __future__ import annotations

import ctypes
import os
import re
import zlib
from dataclasses import dataclass, field

import pytest
import torch

import elementwise_bounds as eb

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mirror of enum DlGemmPath (diffulab_amd/csrc/gemm_paths.h), by name: index = code
PATHS = ["DL_PATH_NONE",
         "NT_BIG_384", "NT_BIG_256", "NT_BIG_192", "NT_BIG_128", "NT_SMALL_RING2", "NT_SMALL_RING4", "NT_SPLITK_RING2", "NT_SPLITK_RING4",
         "NT_DET", "NT_DET_SPLITK", "NT_PAIR_RING2", "NT_PAIR_RING4", "NT_PAIR_FALLBACK",
         "TN_W4", "TN_BIG", "TN_SMALL", "TN_SMALL_SPLITK", "TN_DET", "TN_GROUP_384", "TN_GROUP_256", "TN_GROUP_256_EDGE",
         "CONV_HALO_256_2", "CONV_HALO_128_4", "CONV_HALO_128_3", "CONV_HALO_128_2", "CONV_BIG_256", "CONV_BIG_128",
         "CONV_BIG_256_SPLITK", "CONV_BIG_128_SPLITK", "CONV_SMALL_RING2", "CONV_SMALL_RING4", "CONV_SPLITK_RING2", "CONV_SPLITK_RING4"]

# the library's lab switches (not in the header) and their defaults
LAB_DEFAULTS = {"nt_deep": 1, "conv_big": 1, "conv_halo": 1, "conv_halo_nst": 4, "conv_split128": 1, "wg_cap": 0}

# output tile of each path, for the failure messages
TILE = {"NT_BIG_384": (256, 384), "NT_BIG_256": (256, 256), "NT_BIG_192": (256, 192), "NT_BIG_128": (256, 128),
        "TN_W4": (384, 192), "TN_BIG": (384, 128), "TN_GROUP_384": (384, 192), "TN_GROUP_256": (256, 256), "TN_GROUP_256_EDGE": (256, 256),
        "CONV_HALO_256_2": (256, 256), "CONV_HALO_128_4": (256, 128), "CONV_HALO_128_3": (256, 128), "CONV_HALO_128_2": (256, 128),
        "CONV_BIG_256": (256, 256), "CONV_BIG_128": (256, 128), "CONV_BIG_256_SPLITK": (256, 256), "CONV_BIG_128_SPLITK": (256, 128)}


@dataclass
class Case:
    kind: str  # nt | nt_det | swiglu | pair | tn | tn_det | tn_group | conv
    path: str  # expected path code (256 CUs)
    dims: tuple
    epi: str = "plain"  # nt: plain | f32 | bias | silu_pre | resid | gate | f32_resid;  conv: plain | bias_resid
    lab: dict = field(default_factory=dict)
    pad: int = 8  # extra leading-dimension columns of the operands (poisoned)
    ldc: int | None = None  # nt: output row stride with no left guard (the UNet's output convolution: N = 1 | 3, ldc = 8)
    extra: dict = field(default_factory=dict)

    @property
    def id(self):
        lab = "".join(f"-{k}{v}" for k, v in self.lab.items())
        ex = "".join(f"-{k}{v}" for k, v in self.extra.items())
        dims = re.sub(r"[^0-9x,]", "", "x".join(map(str, self.dims)).replace(", ", "x"))
        return f"{self.kind}-{dims}-{self.epi}{lab}{ex}{'' if self.ldc is None else f'-ldc{self.ldc}'}"


NT_EPIS = ("plain", "f32", "bias", "silu_pre", "resid", "gate", "f32_resid")


def _cases():
    cs = []
    # ---- dl_gemm_nt, persistent big tiles (M % 256 == 0); 256 x 384 takes the plain epilogue only
    cs.append(Case("nt", "NT_BIG_384", (16384, 1152, 384)))
    for M, N, K, path in ((10240, 1280, 128, "NT_BIG_256"), (3072, 3072, 192, "NT_BIG_192"), (10240, 640, 320, "NT_BIG_128")):
        for epi in NT_EPIS:
            cs.append(Case("nt", path, (M, N, K), epi=epi))
    # ---- the 128 x 128 kernel: every epilogue on both rings (ring 2: more than one workgroup per CU, or fewer than four k-steps)
    for epi in NT_EPIS:
        cs.append(Case("nt", "NT_SMALL_RING2", (4200, 1152, 384), epi=epi))
        cs.append(Case("nt", "NT_SMALL_RING4", (300, 1000, 448), epi=epi))
    cs.append(Case("nt", "NT_SMALL_RING2", (300, 1000, 448), epi="gate", lab={"nt_deep": 0}))
    # edges: M, N around one tile and below a fragment, the prologue / tail of both rings (K / 64 = 1..5)
    for M in (1, 2, 127, 129):
        for N in (1, 3, 8, 72, 130):
            for kk in (1, 2, 3, 4, 5):
                cs.append(Case("nt", "NT_SMALL_RING2" if kk < 4 else "NT_SMALL_RING4", (M, N, 64 * kk)))
    for M in (1, 129):  # the UNet's output convolution as a GEMM: 1 or 3 output channels, row stride padded to 8
        for N in (1, 3):
            cs.append(Case("nt", "NT_SMALL_RING4", (M, N, 320), ldc=8))
            cs.append(Case("nt", "NT_SMALL_RING4", (M, N, 320), epi="bias", ldc=8))
    for M, N in ((127, 72), (129, 130)):
        cs.append(Case("nt", "NT_SMALL_RING4", (M, N, 256), epi="gate"))
        cs.append(Case("nt", "NT_SMALL_RING2", (M, N, 192), epi="silu_pre"))
    # split contraction (f32 plain output, < 64 tiles, K >= 2048): hipMemsetAsync (ldc == N) or hipMemset2DAsync (ldc > N) + atomics
    cs.append(Case("nt", "NT_SPLITK_RING4", (64, 136, 4096), epi="f32"))
    cs.append(Case("nt", "NT_SPLITK_RING4", (64, 136, 4096), epi="f32", extra={"dense": 1}))
    cs.append(Case("nt", "NT_SPLITK_RING4", (256, 384, 28416), epi="f32"))
    cs.append(Case("nt", "NT_SPLITK_RING2", (200, 72, 2048), epi="f32", lab={"nt_deep": 0}))
    # ---- dl_gemm_nt_f32_det
    cs.append(Case("nt_det", "NT_DET", (300, 200, 384)))
    cs.append(Case("nt_det", "NT_DET_SPLITK", (64, 136, 4096)))
    cs.append(Case("nt_det", "NT_DET_SPLITK", (256, 384, 28416)))
    # ---- fused SwiGLU (EPI 2): a persistent tiling by score, and the fallbacks for launches with few tiles (M, F, K)
    cs.append(Case("swiglu", "NT_BIG_384", (16384, 576, 384)))
    cs.append(Case("swiglu", "NT_BIG_192", (2048, 768, 384)))
    cs.append(Case("swiglu", "NT_BIG_192", (2048, 768, 384), extra={"noU": 1}))
    cs.append(Case("swiglu", "NT_BIG_128", (512, 2048, 256)))
    # ---- under a data-parallel host's workgroup cap (8 workgroups): every workgroup walks many tiles, launch_big staggers their starts
    cs.append(Case("nt", "NT_BIG_192", (3072, 3072, 192), lab={"wg_cap": 8}))
    cs.append(Case("swiglu", "NT_BIG_192", (2048, 768, 384), lab={"wg_cap": 8}))
    # ---- dl_gemm_nt_pair (M, N0, N1, K0, K1) on column windows, with bias / residual
    cs.append(Case("pair", "NT_PAIR_RING2", (1000, 136, 264, 64, 192), epi="bias_resid"))
    cs.append(Case("pair", "NT_PAIR_RING2", (129, 72, 130, 192, 320), epi="plain"))
    cs.append(Case("pair", "NT_PAIR_RING4", (1024, 1024, 2048, 1024, 1024), epi="bias_resid"))
    cs.append(Case("pair", "NT_PAIR_RING4", (640, 384, 1000, 448, 256), epi="plain"))
    cs.append(Case("pair", "NT_PAIR_FALLBACK", (4096, 1024, 1024, 512, 512), epi="bias_resid"))
    # ---- dl_gemm_tn_ex (R, M, N): += on a non-zero window; column windows a[:, off:]
    cs.append(Case("tn", "TN_W4", (2048, 384, 192)))
    cs.append(Case("tn", "TN_W4", (2048 + 7 * 64, 768, 384), extra={"cap": 64, "off": 64}))
    cs.append(Case("tn", "TN_W4", (8192, 1152, 384), extra={"off": 8}))
    cs.append(Case("tn", "TN_BIG", (4096, 640, 256), extra={"off": 64}))  # ragged last 384-row m-tile
    cs.append(Case("tn", "TN_BIG", (4096 + 64, 768, 128)))
    cs.append(Case("tn", "TN_SMALL", (64, 136, 264)))
    cs.append(Case("tn", "TN_SMALL", (64, 16, 384), extra={"off": 8}))
    cs.append(Case("tn", "TN_SMALL_SPLITK", (4096 + 64, 200, 136)))
    cs.append(Case("tn", "TN_SMALL_SPLITK", (16384, 64, 128), extra={"off": 16}))
    # ---- dl_gemm_tn_det: partial images + fold, or (ring-kernel shapes with ldc == N) the grouped form
    cs.append(Case("tn_det", "TN_DET", (4096 + 64, 200, 136)))
    cs.append(Case("tn_det", "TN_DET", (2048, 384, 192), extra={"wide": 1}))  # ldc > N: not forwarded to the grouped form
    cs.append(Case("tn_det", "TN_GROUP_384", (2048 + 64, 384, 192)))
    cs.append(Case("tn_det", "TN_GROUP_256", (2048, 512, 256)))
    # ---- dl_gemm_tn_group (R, [(M, N), ...]): ragged last token range, the shifted edge tiles overlap their neighbours
    cs.append(Case("tn_group", "TN_GROUP_384", (2048 + 32 * 5, ((1152, 384), (384, 384), (3072, 384), (384, 1536))), extra={"cap": 0}))
    cs.append(Case("tn_group", "TN_GROUP_384", (4096, ((384, 192),)), extra={"cap": 64}))
    cs.append(Case("tn_group", "TN_GROUP_256", (2048 + 32 * 3, ((512, 512), (1024, 256))), extra={"cap": 96}))
    cs.append(Case("tn_group", "TN_GROUP_256_EDGE", (2048 + 32 * 3, ((264, 320), (640, 640))), extra={"cap": 0}))
    cs.append(Case("tn_group", "TN_GROUP_256_EDGE", (2048, ((960, 320),)), extra={"cap": 0}))
    # ---- dl_conv3x3_nt (B, H, W, Ci, Co)
    cs.append(Case("conv", "CONV_HALO_256_2", (32, 32, 32, 64, 512), epi="bias_resid"))
    cs.append(Case("conv", "CONV_HALO_128_4", (96, 16, 16, 64, 256), epi="bias_resid"))
    cs.append(Case("conv", "CONV_HALO_128_4", (8, 16, 16, 128, 128), lab={"conv_halo": 2}))
    cs.append(Case("conv", "CONV_HALO_128_3", (32, 8, 8, 64, 128), epi="bias_resid", lab={"conv_halo": 2}))  # 8 x 8: 50 halo chunks
    cs.append(Case("conv", "CONV_HALO_128_3", (8, 16, 16, 128, 128), lab={"conv_halo": 2, "conv_halo_nst": 3}))
    cs.append(Case("conv", "CONV_HALO_128_2", (2, 32, 32, 64, 128), epi="bias_resid", lab={"conv_halo": 2, "conv_halo_nst": 2}))
    cs.append(Case("conv", "CONV_BIG_256", (128, 4, 4, 128, 256), epi="bias_resid", lab={"conv_big": 2}))
    cs.append(Case("conv", "CONV_BIG_256", (32, 16, 16, 128, 256), lab={"conv_big": 2, "conv_halo": 0}))
    cs.append(Case("conv", "CONV_BIG_128", (128, 4, 4, 128, 384), epi="bias_resid", lab={"conv_big": 2}))
    cs.append(Case("conv", "CONV_BIG_128_SPLITK", (64, 4, 4, 512, 256), epi="bias_resid", lab={"conv_big": 2}, extra={"scratch": 8}))
    cs.append(Case("conv", "CONV_BIG_128_SPLITK", (64, 4, 4, 512, 384), lab={"conv_big": 2}, extra={"scratch": 8}))
    cs.append(Case("conv", "CONV_BIG_256_SPLITK", (64, 4, 4, 512, 256), epi="bias_resid", lab={"conv_big": 2, "conv_split128": 0},
                   extra={"scratch": 8}))
    cs.append(Case("conv", "CONV_SMALL_RING4", (2, 16, 16, 64, 3), epi="bias_resid"))
    cs.append(Case("conv", "CONV_SMALL_RING4", (3, 4, 4, 128, 128), epi="bias_resid"))  # M % 256 != 0
    cs.append(Case("conv", "CONV_SMALL_RING4", (2, 16, 16, 128, 128), lab={"conv_big": 0}))
    cs.append(Case("conv", "CONV_SMALL_RING2", (240, 12, 12, 64, 3), epi="bias_resid"))  # 270 tiles; W = 12: no shift / mask pixels
    cs.append(Case("conv", "CONV_SMALL_RING2", (2, 16, 16, 64, 3), lab={"nt_deep": 0}))
    cs.append(Case("conv", "CONV_SPLITK_RING4", (8, 4, 4, 512, 200), epi="bias_resid", extra={"scratch": 8}))
    cs.append(Case("conv", "CONV_SPLITK_RING4", (8, 4, 4, 512, 200), extra={"scratch": 2}))  # scratch for two images only
    cs.append(Case("conv", "CONV_SPLITK_RING2", (400, 4, 4, 512, 200), epi="bias_resid", extra={"scratch": 8}))
    return cs


CASES = _cases()
REACHED: set[str] = set()


# ------------------------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module")
def lib():
    from diffulab_amd import _lib

    L = _lib.lib()
    L.cdll.dl_lab_last_path.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def n_cu(lib):
    cu, lds, hbm = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    arch = ctypes.create_string_buffer(64)
    lib.call("dl_device_info", 0, ctypes.byref(cu), ctypes.byref(lds), ctypes.byref(hbm), arch, 64)
    return cu.value


def _set_lab(L, settings):
    for k, v in settings.items():
        getattr(L.cdll, f"dl_lab_set_{k}")(int(v))


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


class Rand:
    def __init__(self, seed):
        self.g = torch.Generator(device=DEV)
        self.g.manual_seed(seed)

    def bf(self, shape, std=1.0):
        return (torch.randn(shape, generator=self.g, device=DEV) * std).to(BF)

    def f32(self, shape, std=1.0):
        return torch.randn(shape, generator=self.g, device=DEV) * std


def _seed(case):
    return zlib.crc32(case.id.encode())


def Guarded(rows, cols, dtype, **kw):
    return eb.Guarded(rows, cols, dtype, DEV, **kw)


def _bias(r, n):
    """f32 bias [n] inside a poisoned allocation (16-byte aligned, NaN after the end)"""
    buf = eb.poison_(torch.empty(n + 12, device=DEV))
    v = buf[4:4 + n]
    v.copy_(r.f32((n,), 0.5))
    return v


def _bf_window(r, rows, cols, std=1.0, pad=8):
    return eb.operand(r.bf((rows, cols), std), (cols + pad + 7) // 8 * 8)


# ------------------------------------------------------------------------------------------------------------------ runners
def run_nt(L, c: Case, r: Rand):
    M, N, K = c.dims
    a = eb.operand(r.bf((M, K)), K + c.pad)
    b = eb.operand(r.bf((N, K), K**-0.5), K + c.pad)
    f32 = c.epi.startswith("f32")
    dt = torch.float32 if f32 else BF
    kw = dict(left=0, ld=c.ldc) if c.ldc is not None else dict(left=0, right=0, ld=N) if c.extra.get("dense") else {}
    out = Guarded(M, N, dt, **kw)
    pre = Guarded(M, N, BF, **{**kw, "ld": out.buf.shape[1]}) if c.epi == "silu_pre" else None  # pre_out shares C's row stride
    bias = _bias(r, N) if c.epi in ("bias", "silu_pre") else None
    resid = _bf_window(r, M, N) if c.epi in ("resid", "gate", "f32_resid") else None
    rows = 128 if c.path.startswith("NT_BIG") else 4  # rows per gate row
    gate = _bf_window(r, (M + rows - 1) // rows, N, 0.5, pad=N + 8) if c.epi == "gate" else None
    L.call("dl_gemm_nt", _p(a), a.stride(0), _p(b), b.stride(0), _p(out.win), out.buf.stride(0), M, N, K, _p(bias),
           1 if c.epi == "silu_pre" else 0, 1 if f32 else 0, _p(pre.win) if pre is not None else None, _p(resid),
           resid.stride(0) if resid is not None else 0, _p(gate), gate.stride(0) if gate is not None else 0, rows, _s())
    path = L.cdll.dl_lab_last_path()
    ref, err = eb.gemm_ref(a, b)
    if bias is not None:
        ref, err = eb.add_bias(ref, err, bias)
    checks = []
    if pre is not None:
        checks.append((pre, ref, eb.store_bf16(ref, err), "pre_out"))
        ref, err = eb.silu(ref, err)
    if resid is not None:
        g = gate.repeat_interleave(rows, 0)[:M] if gate is not None else None
        ref, err = eb.gate_resid(ref, err, resid, g)
    checks.append((out, ref, (eb.store_f32 if f32 else eb.store_bf16)(ref, err), "out"))
    return path, checks


def run_nt_det(L, c: Case, r: Rand):
    M, N, K = c.dims
    a = eb.operand(r.bf((M, K)), K + c.pad)
    b = eb.operand(r.bf((N, K), K**-0.5), K + c.pad)
    out = Guarded(M, N, torch.float32)
    scratch = eb.poison_(torch.empty(8 * M * N, device=DEV))  # contents on entry are irrelevant
    L.call("dl_gemm_nt_f32_det", _p(a), a.stride(0), _p(b), b.stride(0), _p(out.win), out.buf.stride(0), M, N, K, _p(scratch),
           scratch.numel(), _s())
    path = L.cdll.dl_lab_last_path()
    ref, err = eb.gemm_ref(a, b)
    return path, [(out, ref, eb.store_f32(ref, err), "out")]


def run_swiglu(L, c: Case, r: Rand):
    M, F, K = c.dims
    x = eb.operand(r.bf((M, K)), K + c.pad)
    wp = eb.operand(r.bf((2 * F, K), K**-0.5), K + c.pad)
    U = None if c.extra.get("noU") else Guarded(M, 2 * F, BF)
    H = Guarded(M, F, BF)
    L.call("dl_gemm_nt_swiglu", _p(x), x.stride(0), _p(wp), wp.stride(0), _p(U.win) if U else None, U.buf.stride(0) if U else 0,
           _p(H.win), H.buf.stride(0), M, F, K, _s())
    path = L.cdll.dl_lab_last_path()
    P, E = eb.gemm_ref(x, wp)
    # the weight shadow is row-permuted: 32-column tile t holds x1 of hidden units 16t .. 16t+15, then x3 of the same units
    u = torch.arange(F, device=DEV)
    i1 = 32 * (u // 16) + u % 16
    r1, e1, r3, e3 = P[:, i1], E[:, i1], P[:, i1 + 16], E[:, i1 + 16]
    h, eh = eb.swiglu(r1, e1, r3, e3)
    checks = [(H, h, eb.store_bf16(h, eh), "h")]
    if U is not None:
        ru, euu = torch.cat([r1, r3], 1), torch.cat([e1, e3], 1)
        checks.append((U, ru, eb.store_bf16(ru, euu), "u"))
    return path, checks


class _NtProblem(ctypes.Structure):
    _fields_ = [("A", ctypes.c_void_p), ("lda", ctypes.c_int64), ("B", ctypes.c_void_p), ("ldb", ctypes.c_int64), ("C", ctypes.c_void_p),
                ("ldc", ctypes.c_int64), ("M", ctypes.c_int64), ("N", ctypes.c_int64), ("K", ctypes.c_int64), ("bias", ctypes.c_void_p),
                ("resid", ctypes.c_void_p), ("ldr", ctypes.c_int64)]


def run_pair(L, c: Case, r: Rand):
    M, N0, N1, K0, K1 = c.dims
    arr = (_NtProblem * 2)()
    checks, keep = [], []  # (keep: the operands must outlive the launch below)
    for q, N, K in zip(arr, (N0, N1), (K0, K1)):
        a = eb.operand(r.bf((M, K)), K + c.pad)
        b = eb.operand(r.bf((N, K), K**-0.5), K + c.pad)
        out = Guarded(M, N, BF)
        bias = _bias(r, N) if c.epi == "bias_resid" else None
        resid = _bf_window(r, M, N) if c.epi == "bias_resid" else None
        q.A, q.lda, q.B, q.ldb, q.C, q.ldc = _p(a), a.stride(0), _p(b), b.stride(0), _p(out.win), out.buf.stride(0)
        q.M, q.N, q.K, q.bias, q.resid, q.ldr = M, N, K, _p(bias), _p(resid), resid.stride(0) if resid is not None else 0
        keep += [a, b, bias, resid]
        ref, err = eb.gemm_ref(a, b)
        ref, err = eb.add_bias_resid(ref, err, bias, resid)
        checks.append((out, ref, eb.store_bf16(ref, err), f"C{len(checks)}"))
    L.call("dl_gemm_nt_pair", ctypes.addressof(arr), 2, _s())
    return L.cdll.dl_lab_last_path(), checks


def run_tn(L, c: Case, r: Rand):
    R, M, N = c.dims
    off = c.extra.get("off", 0)
    a = eb.operand(r.bf((R, M)), off + M + c.pad, col0=off)
    b = eb.operand(r.bf((R, N)), N + c.pad)
    init = r.f32((M, N))
    if c.kind == "tn_det":
        wide = c.extra.get("wide", 0)
        C = Guarded(M, N, torch.float32, left=0, right=8 if wide else 0, init=init)
        scratch = eb.poison_(torch.empty(8 * M * N, device=DEV))
        L.call("dl_gemm_tn_det", _p(a), a.stride(0), _p(b), b.stride(0), _p(C.win), C.buf.stride(0), M, N, R, _p(scratch), scratch.numel(), _s())
    else:
        C = Guarded(M, N, torch.float32, init=init)
        L.call("dl_gemm_tn_ex", _p(a), a.stride(0), _p(b), b.stride(0), _p(C.win), C.buf.stride(0), M, N, R, c.extra.get("cap", 0), _s())
    path = L.cdll.dl_lab_last_path()
    ref, err = eb.tn_ref(a, b, init)
    return path, [(C, ref, eb.store_f32(ref, err), "C")]


class _WGrad(ctypes.Structure):
    _fields_ = [("dy", ctypes.c_void_p), ("ld_dy", ctypes.c_int64), ("x", ctypes.c_void_p), ("ld_x", ctypes.c_int64),
                ("g", ctypes.c_void_p), ("m_out", ctypes.c_int64), ("n_in", ctypes.c_int64)]


def run_tn_group(L, c: Case, r: Rand):
    R, shapes = c.dims
    arr = (_WGrad * len(shapes))()
    checks, keep = [], []  # (keep: the operands must outlive the launch below)
    for i, (q, (M, N)) in enumerate(zip(arr, shapes)):
        a = eb.operand(r.bf((R, M)), 64 + M + c.pad, col0=64)
        b = eb.operand(r.bf((R, N)), N + 128)
        init = r.f32((M, N))
        g = Guarded(M, N, torch.float32, left=0, right=0, ld=N, init=init)  # contiguous [M, N]: guard rows only
        q.dy, q.ld_dy, q.x, q.ld_x, q.g, q.m_out, q.n_in = _p(a), a.stride(0), _p(b), b.stride(0), _p(g.win), M, N
        keep += [a, b]
        ref, err = eb.tn_ref(a, b, init)
        checks.append((g, ref, eb.store_f32(ref, err), f"g{i}"))
    total = sum(M * N for M, N in shapes)
    slab = eb.poison_(torch.empty(8 * total, device=DEV))
    L.call("dl_gemm_tn_group", ctypes.addressof(arr), len(shapes), R, _p(slab), slab.numel(), c.extra.get("cap", 0), _s())
    return L.cdll.dl_lab_last_path(), checks


def run_conv(L, c: Case, r: Rand):
    Bn, H, W, Ci, Co = c.dims
    M, K = Bn * H * W, 9 * Ci
    x = eb.operand(r.bf((M, Ci)), Ci + c.pad)  # the ldx > Ci gap and the rows below the last pixel hold NaN
    wf = eb.operand(r.bf((Co, K), K**-0.5), (K + 63) // 64 * 64 + 8)
    zbuf = eb.poison_(torch.empty(128, dtype=BF, device=DEV))
    zero = zbuf[:64]
    zero.zero_()
    out = Guarded(M, Co, BF, left=0, ld=8) if Co < 8 else Guarded(M, Co, BF)
    bias = _bias(r, Co) if c.epi == "bias_resid" else None
    resid = _bf_window(r, M, Co) if c.epi == "bias_resid" else None
    ns = c.extra.get("scratch", 0)
    scratch = eb.poison_(torch.empty(ns * M * Co, device=DEV)) if ns else None
    L.call("dl_conv3x3_nt", _p(x), x.stride(0), Bn, H, W, Ci, _p(wf), wf.stride(0), _p(out.win), out.buf.stride(0), Co, _p(bias), _p(resid),
           resid.stride(0) if resid is not None else 0, _p(zero), _p(scratch), scratch.numel() if scratch is not None else 0, _s())
    path = L.cdll.dl_lab_last_path()
    torch.cuda.synchronize()
    assert bool((zero == 0).all()) and bool(eb.is_poison(zbuf[64:]).all()), "the zero line changed"
    ref, err = eb.conv_ref(x, Bn, H, W, wf)
    ref, err = eb.add_bias_resid(ref, err, bias, resid)
    return path, [(out, ref, eb.store_bf16(ref, err), "out")]


RUN = {"nt": run_nt, "nt_det": run_nt_det, "swiglu": run_swiglu, "pair": run_pair, "tn": run_tn, "tn_det": run_tn, "tn_group": run_tn_group,
       "conv": run_conv}


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gemm_path(lib, n_cu, case):
    try:
        _set_lab(lib, case.lab)
        path, checks = RUN[case.kind](lib, case, Rand(_seed(case)))
        torch.cuda.synchronize()
    finally:
        _set_lab(lib, LAB_DEFAULTS)
    name = PATHS[path] if 0 <= path < len(PATHS) else f"<{path}>"
    REACHED.add(name)
    if n_cu == 256:
        assert name == case.path, f"{case.id}: dispatched to {name}, the table expects {case.path}"
    tile = TILE.get(name, (128, 128))
    for g, ref, bound, what in checks:
        g.check(f"{case.id} [{name}] {what}")
        eb.assert_within(g.win, ref, bound, tile=tile, what=f"{case.id} [{name}] {what}")


def test_path_enum_mirror():
    """PATHS mirrors enum DlGemmPath by name and order"""
    text = open(os.path.join(ROOT, "diffulab_amd", "csrc", "gemm_paths.h")).read()
    body = text[text.index("enum DlGemmPath"):text.index("DL_PATH_COUNT")]
    names = re.findall(r"^\s*([A-Z][A-Z0-9_]+)\b", body.split("{", 1)[1], flags=re.M)
    assert names == PATHS
    assert {c.path for c in CASES} == set(PATHS[1:]), set(PATHS[1:]) ^ {c.path for c in CASES}


def test_every_path_code_is_reached(n_cu):
    """runs after the table (module order): every path code was taken by at least one case"""
    if n_cu != 256:
        pytest.skip(f"the expected codes assume 256 CUs, this device has {n_cu}")
    missing = set(PATHS[1:]) - REACHED
    assert not missing, f"path codes no case reached: {sorted(missing)}"
    print(f"reached all {len(PATHS) - 1} path codes")
