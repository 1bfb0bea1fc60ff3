"""Reference, bound, case table and f32 emulation of the 3x3 convolution weight gradient (imported by the test modules; not a conftest).

    g[(tap, ci), co] = init + sum_p x[p + shift(tap), ci] * dY[p, co],   tap = 3 ky + kx, zero outside the image

over NHWC rows, by dl_conv3x3_wgrad_tn (the pixel ranges meet in g through f32 atomics) and dl_conv3x3_wgrad_tn_parts (every range
stores its own image; init = 0, the quantity checked is the fp64 sum of the images).  Six kernels compute it: conv3x3_wgrad_halo_k
in four geometries and the implicit-GEMM kernels gemm_tn_k<true> / gemm_tn_big_k<true> (csrc/conv_wgrad_paths.h).

Reference and bound are those of every other TN product of the suite (tests/elementwise_bounds.py): the operand is
eb.conv_cols(x), the reference eb.tn_ref in fp64, the bound the f32-accumulation bound ACC_C * (R + 1) * 2^-24 * (|init| + |cols|^T |dY|)
with R = the number of REAL pixels, plus the f32 store.  No constant of its own.

Two input classes.  `gauss`: bf16 normal operands, judged by the bound.  `exact`: operands from {-2 .. 2} and a small integer init:
every partial sum stays below 2^24, f32 arithmetic is exact in any order, and the result must EQUAL the reference.  The bound grows
with R^2 while one pixel's contribution does not: at R = 8192 a fault worth one pixel, or a result rounded to bf16, sits inside the
bound; the exact class sees it.

The emulation below walks the pixels as the kernels do (64-pixel steps of four 16-pixel blocks, `nparts` ranges of `sps` steps,
ranges combined in an arbitrary order, through an accumulating g or through stored images) in torch f32 on the CPU.  MUTANTS lists
the faults planted into it by tests/test_conv_wgrad_bounds_host.py.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

import elementwise_bounds as eb

BF = torch.bfloat16
PATHS = ["WG_NONE", "WG_HALO_W32", "WG_HALO_W16", "WG_HALO_W8", "WG_HALO_W4", "WG_IGEMM_BIG", "WG_IGEMM_SMALL"]  # enum DlConvWgradPath
MODES = ("gauss", "exact")
FORMS = ("atomic", "parts")
TILE = {"WG_IGEMM_BIG": (384, 128)}  # output tile per path for the failure messages (halo: all nine taps of 64 channels, see tile_rows)


# ------------------------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    B: int
    H: int
    W: int
    Ci: int
    Co: int
    path: str  # expected path code (256 CUs)
    nparts: int  # expected pixel ranges = partial images (256 CUs)
    max_wgs: int = 0
    halo: int = 1  # lab switch dl_lab_set_wgrad_halo

    @property
    def npix(self):
        return self.B * self.H * self.W

    @property
    def R(self):
        return (self.npix + 63) // 64 * 64

    @property
    def id(self):
        return (f"{self.B}x{self.H}x{self.W}-{self.Ci}-{self.Co}" + (f"-wgs{self.max_wgs}" if self.max_wgs else "")
                + ("" if self.halo == 1 else f"-halo{self.halo}"))


CASES = [
    # ---- conv3x3_wgrad_halo_k.  One step (ring prologue and tail only) in each geometry; H = 2: every row is a border row
    Case(1, 2, 32, 128, 128, "WG_HALO_W32", 1),
    Case(1, 4, 16, 128, 128, "WG_HALO_W16", 1),
    Case(1, 8, 8, 128, 128, "WG_HALO_W8", 1),
    Case(1, 4, 4, 128, 128, "WG_HALO_W4", 1),
    # 2, 3, 4 and 5 steps in one range: the four-slot ring fills, then wraps
    Case(2, 8, 8, 128, 128, "WG_HALO_W8", 1),
    Case(3, 2, 32, 128, 256, "WG_HALO_W32", 1),
    Case(1, 8, 32, 128, 128, "WG_HALO_W32", 1),  # steps that start in mid-image: py0 = 0, 2, 4, 6
    Case(5, 8, 8, 128, 128, "WG_HALO_W8", 1),
    Case(5, 4, 4, 128, 128, "WG_HALO_W4", 1),  # 80 pixels: the last step holds one image, its other three segments lie outside x
    Case(2, 16, 16, 256, 128, "WG_HALO_W16", 1),  # 8 steps, py0 = 0, 4, 8, 12; four channel chunks
    # several ranges: tile-minor with a ragged last range (9, 9, 7 steps), XCD-major with 8 and 16 ranges, a workgroup cap
    Case(25, 8, 8, 128, 128, "WG_HALO_W8", 3),
    Case(64, 8, 8, 128, 128, "WG_HALO_W8", 8),
    Case(8, 32, 32, 128, 128, "WG_HALO_W32", 16),
    Case(64, 8, 8, 256, 256, "WG_HALO_W8", 2, max_wgs=16),  # 4 x 2 tiles, 2 ranges of 32 steps
    # ---- gemm_tn_k<true>.  1 x 1, W = 1 and H = 1 maps; Co = 8 and 72: one clamped column tile
    Case(3, 1, 1, 128, 8, "WG_IGEMM_SMALL", 1),
    Case(2, 3, 1, 128, 72, "WG_IGEMM_SMALL", 1),
    Case(2, 1, 5, 128, 72, "WG_IGEMM_SMALL", 1),
    Case(3, 7, 7, 128, 8, "WG_IGEMM_SMALL", 3),  # division, not shift and mask; 147 pixels in 3 steps
    Case(2, 14, 14, 128, 136, "WG_IGEMM_SMALL", 7),  # second column tile clamped to its last 8 columns
    Case(1, 28, 28, 128, 128, "WG_IGEMM_SMALL", 13),  # 13 steps: below the big kernel's threshold
    Case(2, 12, 20, 256, 200, "WG_IGEMM_SMALL", 8),  # not square, not a power of two
    Case(1, 16, 8, 128, 128, "WG_IGEMM_SMALL", 2),  # a power-of-two map the halo kernel does not take
    Case(2, 8, 8, 128, 128, "WG_IGEMM_SMALL", 2, halo=0),  # shift / mask pixels
    Case(20, 16, 8, 384, 200, "WG_IGEMM_SMALL", 14),  # ranges of 3 steps, the last of 1
    # ---- gemm_tn_big_k<true> (R >= 4096, Co % 128 == 0); its 384-row tiles hold three taps (Ci = 128) or one and a half (Ci = 256)
    Case(6, 28, 28, 128, 128, "WG_IGEMM_BIG", 9),  # 74 steps: 8 ranges of 9, the last of 2
    Case(4, 32, 32, 256, 128, "WG_IGEMM_BIG", 8, halo=0),
    Case(6, 28, 28, 128, 256, "WG_IGEMM_BIG", 2, max_wgs=16),  # 6 units padded to 8: two idle ones return without writing
]


# ------------------------------------------------------------------------------------------------------------------ dispatch mirror
@dataclass(frozen=True)
class Plan:
    path: str
    nparts: int
    sps: int  # steps per range
    nsteps: int


def plan(c: Case, n_cu: int = 256) -> Plan:
    """what conv_wgrad_halo_splits (csrc/conv_wgrad.hip) and conv_wgrad_plan (csrc/gemm.hip) decide for a case on n_cu CUs"""
    nsteps = c.R // 64
    budget = c.max_wgs if 0 < c.max_wgs < n_cu else n_cu
    pow2 = c.H & (c.H - 1) == 0
    geom = (c.W == 32 and c.H % 2 == 0) or (c.W == 16 and c.H % 4 == 0) or (c.W == 8 and c.H == 8) or (c.W == 4 and c.H == 4)
    if c.halo and c.Ci % 64 == 0 and c.Co % 128 == 0 and pow2 and geom:
        ntile = (c.Ci // 64) * (c.Co // 128)
        splits = max(1, min(budget // ntile, nsteps // 8))
        if splits >= 8:
            splits &= ~7
        sps = -(-nsteps // splits)
        return Plan(f"WG_HALO_W{c.W}", -(-nsteps // sps), sps, nsteps)
    M, N = 9 * c.Ci, c.Co
    if M % 384 == 0 and N % 128 == 0 and nsteps >= 64:
        tiles_m, tiles_n = M // 384, N // 128
        padded = max(8, (budget // tiles_n) & ~7)
        splits = min(max(1, padded // tiles_m), nsteps // 8)
        sps = -(-nsteps // splits)
        return Plan("WG_IGEMM_BIG", -(-nsteps // sps), sps, nsteps)
    ntile = -(-M // 128) * -(-N // 128)
    splits = max(1, min(-(-1024 // ntile), nsteps))
    sps = -(-nsteps // splits)
    return Plan("WG_IGEMM_SMALL", -(-nsteps // sps), sps, nsteps)


def tile_rows(path: str, Ci: int, tm: int) -> torch.Tensor:
    """rows of g that output tile tm of a kernel owns: all nine taps of a 64-channel chunk (halo), 128 or 384 consecutive rows"""
    if path.startswith("WG_HALO"):
        return (torch.arange(9)[:, None] * Ci + tm * 64 + torch.arange(64)[None, :]).reshape(-1)
    n = 384 if path == "WG_IGEMM_BIG" else 128
    return torch.arange(tm * n, (tm + 1) * n)


# ------------------------------------------------------------------------------------------------------------------ inputs + operands
def make_inputs(c: Case, mode: str, seed: int, device) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """x bf16 [npix, Ci], dY bf16 [npix, Co], init f32 [9 Ci, Co]"""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    if mode == "gauss":
        n = lambda *s: torch.randn(s, generator=g, device=device)  # noqa: E731
        return n(c.npix, c.Ci).to(BF), n(c.npix, c.Co).to(BF), n(9 * c.Ci, c.Co)
    assert mode == "exact" and 4 * c.npix + 3 < 2**24
    k = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g, device=device).float()  # noqa: E731
    return k(-2, 2, c.npix, c.Ci).to(BF), k(-2, 2, c.npix, c.Co).to(BF), k(-3, 3, 9 * c.Ci, c.Co)


def x_guard_rows(W: int) -> int:
    """guard rows above and below x: a tap displacement (W + 1 rows) from any row of a padded 64-pixel step stays inside the buffer"""
    return W + 1 + 64


def x_operand(values: torch.Tensor, W: int, col0: int = 8, right: int = 8) -> tuple[torch.Tensor, torch.Tensor]:
    """(buffer, window): values [npix, Ci] as a channel slice at the 8-aligned column col0 of a poisoned, wider bf16 buffer with
    x_guard_rows(W) poisoned rows above and below: a tap that reads a row or a channel it must not reads NaN"""
    npix, Ci = values.shape
    assert col0 % 8 == 0
    top = x_guard_rows(W)
    buf = eb.poison_(torch.empty(top + npix + top, (col0 + Ci + right + 7) // 8 * 8, dtype=values.dtype, device=values.device))
    win = buf[top:top + npix, col0:col0 + Ci]
    win.copy_(values)
    return buf, win


def dy_operand(values: torch.Tensor, R: int, pad: int = 8) -> tuple[torch.Tensor, torch.Tensor]:
    """(buffer, window [R, Co]): rows >= npix of the window zero (the contract), the ldy gap and two rows below R poisoned"""
    npix, Co = values.shape
    buf = eb.poison_(torch.empty(R + 2, Co + pad, dtype=values.dtype, device=values.device))
    win = buf[:R, :Co]
    win.zero_()
    win[:npix].copy_(values)
    return buf, win


# ------------------------------------------------------------------------------------------------------------------ reference + bound
def reference(x: torch.Tensor, dy: torch.Tensor, c: Case, init: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor]:
    """(ref, bound) fp64 [9 Ci, Co] of the stored f32 result; init None: the parts form (init = 0)"""
    if init is None:
        init = torch.zeros(9 * c.Ci, c.Co, device=x.device)
    ref, err = eb.tn_ref(eb.conv_cols(x[:c.npix], c.B, c.H, c.W), dy[:c.npix], init)
    return ref, eb.store_f32(ref, err)


def to_dw(g: torch.Tensor, Ci: int) -> torch.Tensor:
    """g[(tap, ci), co] -> dw[co, ci, ky, kx]"""
    Co = g.shape[1]
    return g.reshape(3, 3, Ci, Co).permute(3, 2, 0, 1).contiguous()


def fold_bound(ref: torch.Tensor, bound: torch.Tensor, dw0: torch.Tensor, Ci: int) -> tuple[torch.Tensor, torch.Tensor]:
    """dw0 + (the images added in f32): one more f32 addition on top of the bound of their sum"""
    r, b, d0 = to_dw(ref, Ci), to_dw(bound, Ci), dw0.double()
    out = d0 + r
    return out, eb.store_f32(out, b + eb.U32 * (r.abs() + b + d0.abs()))


def rejected(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, mode: str) -> bool:
    """the verdict of the GPU test on a result: outside the bound (gauss; NaN is outside) or not equal (exact)"""
    if mode == "exact":
        return not torch.equal(got.double(), ref)
    return bool((~((got.double() - ref).abs() <= bound)).any())


def worst_ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    r = (got.double().to(ref.device) - ref).abs() / bound
    return float(torch.nan_to_num(r, nan=float("inf")).max())


# ------------------------------------------------------------------------------------------------------------------ emulation
MUTANTS = {
    "a": "a left/right border tap reads p + shift instead of the zero line (one tile, tap, step)",
    "b": "a top/bottom border tap reads the neighbouring image's row (one tile, tap, step)",
    "c": "rows at or beyond npix of the last step read x instead of the zero line (one tile, tap)",
    "d": "the last step of one range is dropped (one tile)",
    "e": "one step is counted by two ranges (one tile)",
    "f": "one 16-pixel block of one tap is dropped (one tile, step)",
    "g": "ky and kx are swapped (one tile)",
    "h": "the second 64-channel chunk's ci0 is used for the first (one tile)",
    "i": "a 384-row tile that holds several taps uses its first tap's shift throughout",
    "j": "init is overwritten, not added to (atomic form, one tile)",
    "k": "one partial image keeps what its buffer held (parts form, one tile)",
    "l": "the result is rounded to bf16 (one tile)",
}


def mutant_exists(m: str, c: Case, p: Plan) -> bool:
    return {"a": c.npix > c.W, "b": c.B > 1, "c": c.R > c.npix, "e": p.nparts >= 2, "g": c.H * c.W > 1,
            "i": p.path == "WG_IGEMM_BIG"}.get(m, True)


def _gather(xg: torch.Tensor, top: int, c: Case, taps, rows: slice | None = None, lr=True, tb=True, inside=True, chan=None):
    """f32 [R, len(taps) * Ci]: row p of tap (ky, kx) is x[p + (ky - 1) W + kx - 1] or the zero line.  xg f32 [top + npix + top, Ci]
    is the whole guarded buffer (NaN outside the window).  lr / tb / inside = False drop the left-right, top-bottom or p < npix
    test (where the row read instead is a pixel of x: the verdict on (a), (b) then comes from data, not from the poison)"""
    p = torch.arange(c.R)
    px, py = p % c.W, (p // c.W) % c.H
    out = []
    for ky, kx in taps:
        dy, dx = ky - 1, kx - 1
        src = p + dy * c.W + dx
        ok_lr = (px + dx >= 0) & (px + dx < c.W)
        ok_tb = (py + dy >= 0) & (py + dy < c.H)
        ok_in = p < c.npix
        real = (src >= 0) & (src < c.npix)
        ok = (ok_lr if lr else real) & (ok_tb if tb else real) & (ok_in if inside else torch.ones_like(ok_in))
        v = xg[(top + src).clamp(0, xg.shape[0] - 1)]
        out.append(torch.where(ok[:, None], v, torch.zeros_like(v)))
    return torch.cat(out, 1)


TAPS = [(ky, kx) for ky in range(3) for kx in range(3)]


def _accumulate(cols, dy, p: Plan, row_tap=None, drop_last_of=None, twice=None, drop_block=None):
    """parts f32 [nparts, m, n]: range r adds its steps' four 16-pixel blocks one after the other.  drop_last_of = r; twice = r: range
    r + 1 also runs the last step of range r; drop_block = (step, kk, tap) with row_tap[m] = the tap of row m"""
    m, n = cols.shape[1], dy.shape[1]
    parts = torch.zeros(p.nparts, m, n)
    for r in range(p.nparts):
        steps = list(range(r * p.sps, min((r + 1) * p.sps, p.nsteps)))
        if drop_last_of == r:
            steps = steps[:-1]
        if twice is not None and r == twice + 1:
            steps = [steps[0] - 1] + steps
        acc = torch.zeros(m, n)
        for s in steps:
            a = cols[s * 64:(s + 1) * 64].reshape(4, 16, m)
            b = dy[s * 64:(s + 1) * 64].reshape(4, 16, n)
            pb = torch.bmm(a.transpose(1, 2), b)
            for kk in range(4):
                if drop_block is not None and drop_block[:2] == (s, kk):
                    pb[kk][row_tap == drop_block[2]] = 0.0
                acc = acc + pb[kk]
        parts[r] = acc
    return parts


def _combine(parts, init, order, overwrite=False):
    g = torch.zeros_like(init) if overwrite else init.clone()
    for r in order:
        g = g + parts[r]
    return g


def emulate(xbuf: torch.Tensor, col0: int, dy: torch.Tensor, init: torch.Tensor, c: Case, p: Plan, form: str, seed: int = 0,
            mut: str = "") -> torch.Tensor:
    """the (mutated) f32 computation on the CPU.  xbuf: the poisoned buffer of x_operand, dy the [R, Co] window, init f32.
    -> atomic: g f32 [9 Ci, Co];  parts: the stored images f32 [nparts, 9 Ci, Co] (init is not used)"""
    top = x_guard_rows(c.W)
    xg = xbuf[:, col0:col0 + c.Ci].float()
    D = dy.float()
    order = torch.randperm(p.nparts, generator=torch.Generator().manual_seed(seed)).tolist()
    parts = _accumulate(_gather(xg, top, c, TAPS), D, p)
    out = parts if form == "parts" else _combine(parts, init, order)
    if not mut:
        return out
    assert mutant_exists(mut, c, p), (mut, c.id)
    # ---- the mutated tile, its result spliced into the clean one: the last column tile; the row tile that holds the last channels of
    # the tap the fault shows in ((1, 2): right neighbour; (2, 1): the row below; else the centre tap, which is never all zero)
    tap = {"a": 5, "b": 7, "g": 5}.get(mut, 4)
    tn = (c.Co - 1) // 128
    if p.path.startswith("WG_HALO"):
        tm = 0 if mut == "h" else c.Ci // 64 - 1
    else:
        tm = (tap * c.Ci + c.Ci - 1) // (384 if p.path == "WG_IGEMM_BIG" else 128)
    rows = tile_rows(p.path, c.Ci, tm)
    n0, n1 = tn * 128, min(c.Co, tn * 128 + 128)
    row_tap, row_ci = rows // c.Ci, rows % c.Ci
    # (a), (b): the step of the last pixel of the first row / of the first image, whose right / lower neighbour in memory is a pixel of x
    step = {"a": 0, "b": (c.H * c.W - 1) // 64}.get(mut, p.nsteps // 2)
    full = _gather(xg, top, c, TAPS)
    colsm = full[:, rows].clone()
    kw = {}
    if mut in ("a", "b", "c"):
        if mut == "c":
            step = p.nsteps - 1
        alt = _gather(xg, top, c, [TAPS[tap]], lr=mut != "a", tb=mut != "b", inside=mut != "c")
        sel = row_tap == tap
        colsm[step * 64:(step + 1) * 64, sel] = alt[step * 64:(step + 1) * 64][:, row_ci[sel]]
    elif mut == "g":
        sw = _gather(xg, top, c, [(kx, ky) for ky, kx in TAPS])
        colsm = sw[:, rows]
    elif mut == "h":
        first = row_ci < 64
        colsm[:, first] = full[:, rows[first] + 64]
    elif mut == "i":
        one = _gather(xg, top, c, [TAPS[int(row_tap[0])]])
        colsm = one[:, row_ci]
    elif mut == "d":
        kw = dict(drop_last_of=p.nparts // 2)
    elif mut == "e":
        kw = dict(twice=(p.nparts - 1) // 2)
    elif mut == "f":
        kw = dict(drop_block=(step if step * 64 < c.npix else 0, 0, tap), row_tap=row_tap)
    pm = _accumulate(colsm, D[:, n0:n1], p, **kw)
    if mut == "l":
        pm = pm.to(BF).float() if form == "parts" else pm
    if form == "parts":
        if mut == "k":
            pm[p.nparts // 2] = eb.poison_(torch.empty_like(pm[0]))  # the test's images start out poisoned
        assert mut != "j"
        out[:, rows[:, None], torch.arange(n0, n1)[None, :]] = pm
        return out
    assert mut != "k"
    gm = _combine(pm, init[rows][:, n0:n1], order, overwrite=mut == "j")
    out[rows[:, None], torch.arange(n0, n1)[None, :]] = gm.to(BF).float() if mut == "l" else gm
    return out
