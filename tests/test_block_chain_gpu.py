"""dl_dit_block_fwd_chain (csrc/block_fused.hip): the forward of one DiT block as ONE launch in which every workgroup carries whole
samples through the five phases (qkv GEMM + statistics, QK-norm + RoPE + attention, projection + LN2, MLP-up + SwiGLU, MLP-down +
next LayerNorm).  The phases are the device bodies of the separate launches, so every output must carry the SAME BITS as
dl_dit_block_fwd's five launches on the same inputs: every output buffer is compared byte for byte, together with the guard elements
in front of and behind each of them.

Shapes: D = 384, 6 heads, F = 1536, N = 256; the chain runs at B = 2 and 3 (M = 512 and 768).  The separate launches do not exist
for so few samples (the row-complete GEMMs want 8 tiles, the stationary GEMMs panels for 0.7 of a workgroup budget that never goes
below 8, the tiled qkv GEMM 64 tiles), so the reference is dl_dit_block_fwd with bit 3 clear at B = 8 on the same buffers, computed
once per mode: every operation of the block is local to a sample, so its first B samples ARE the unfused result of the B-sample
block.  The chain then runs on the same dl_dit_block_t with B lowered to 2 or 3: the rows of samples B .. 7 of every output must
keep their poison, which guards every output a whole sample deep.  At B = 8 bit 3 is also toggled on one and the same block."""

from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF = torch.bfloat16
D, HEADS, F, DH = 384, 6, 1536, 64
GUARD = 64  # guard elements in front of and behind every output
CHAIN = 8   # bit 3 of dl_dit_block_t::row_gemms

OUT_BF = ("qkv", "q", "k", "a", "t1", "x1", "xm2", "h", "u", "t2", "next_x", "next_xm", "xm1", "v")
OUT_F32 = ("ssq", "rrms", "lse", "mean2", "rstd2", "next_mean", "next_rstd", "mean1", "rstd1")


def _randn(gen, *shape, std=1.0, dtype=BF):
    return (torch.randn(*shape, generator=gen) * std).to(DEV, dtype)


class Block:
    """operands of one block on seeded values; every output is a window of a poisoned allocation"""

    def __init__(self, B: int, N: int, seed: int, ssq: bool = True, row: bool = True, store_u: bool = False):
        from diffulab_amd._block import DitBlock

        g = torch.Generator().manual_seed(seed)
        self.B, self.N, self.M = B, N, B * N
        M = self.M
        self.row = row
        v_in_place = N <= 256
        self.inp = dict(
            x_in=_randn(g, M, D), xm1=_randn(g, M, D), mod=_randn(g, B, 8 * D, std=0.3),
            ln1_w=1 + _randn(g, D, std=0.1, dtype=torch.float32), ln1_b=_randn(g, D, std=0.1, dtype=torch.float32),
            ln2_w=1 + _randn(g, D, std=0.1, dtype=torch.float32), ln2_b=_randn(g, D, std=0.1, dtype=torch.float32),
            nln_w=1 + _randn(g, D, std=0.1, dtype=torch.float32), nln_b=_randn(g, D, std=0.1, dtype=torch.float32),
            qn=1 + _randn(g, D, std=0.1, dtype=torch.float32), kn=1 + _randn(g, D, std=0.1, dtype=torch.float32),
            w_qkv=_randn(g, 3 * D, D, std=D**-0.5), w_proj=_randn(g, D, D, std=D**-0.5), w_up=_randn(g, 2 * F, D, std=D**-0.5),
            w_down=_randn(g, D, F, std=F**-0.5))
        ang = torch.rand(N, DH // 2, generator=g) * 6.28
        self.inp["cos"], self.inp["sin"] = torch.cos(ang).to(DEV), torch.sin(ang).to(DEV)
        shapes = dict(qkv=(M, 3 * D), q=(B, HEADS, N, DH), k=(B, HEADS, N, DH), a=(M, D), t1=(M, D), x1=(M, D), xm2=(M, D), h=(M, F),
                      u=(M, 2 * F), t2=(M, D), next_x=(M, D), next_xm=(M, D), ssq=(M, 2), rrms=(M, 2), lse=(B, HEADS, N), mean2=(M,),
                      rstd2=(M,), next_mean=(M,), next_rstd=(M,))
        if not row:  # the sequence without row-complete GEMMs runs LN1 itself
            shapes.update(xm1=(M, D), mean1=(M,), rstd1=(M,))
        if not v_in_place:
            shapes.update(v=(B, HEADS, N, DH))
        self.flat, self.out = {}, {}
        for name, shp in shapes.items():
            n = 1
            for s in shp:
                n *= s
            dt = BF if name in OUT_BF else torch.float32
            self.flat[name] = torch.empty(n + 2 * GUARD, device=DEV, dtype=dt)
            self.out[name] = self.flat[name][GUARD : GUARD + n].view(shp)
        i, o = self.inp, self.out
        mod = i["mod"]
        mrow = lambda c: mod.data_ptr() + 2 * c * D  # noqa: E731
        blk = DitBlock()
        blk.B, blk.N, blk.D, blk.H, blk.F = B, N, D, HEADS, F
        blk.ld_mod, blk.ldw_d, blk.ldw_f, blk.rot, blk.eps, blk.next_eps = mod.stride(0), D, F, DH, 1e-5, 1e-5
        blk.set(x_in=i["x_in"], scale1=mrow(0), shift1=mrow(1), gate1=mrow(2), scale2=mrow(3), shift2=mrow(4), gate2=mrow(5),
                ln1_w=i["ln1_w"], ln1_b=i["ln1_b"], ln2_w=i["ln2_w"], ln2_b=i["ln2_b"], qn_scale=i["qn"], kn_scale=i["kn"],
                w_qkv=i["w_qkv"], w_proj=i["w_proj"], w_up=i["w_up"], w_up_perm=i["w_up"], w_down=i["w_down"], rope_cos=i["cos"],
                rope_sin=i["sin"], xm1=o["xm1"] if not row else i["xm1"], mean1=o.get("mean1"), rstd1=o.get("rstd1"), qkv=o["qkv"],
                q=o["q"], k=o["k"], v=o.get("v"), rrms=o["rrms"], a=o["a"], lse=o["lse"], t1=o["t1"], x1=o["x1"], xm2=o["xm2"],
                mean2=o["mean2"], rstd2=o["rstd2"], u=o["u"] if store_u else None, h=o["h"], t2=o["t2"],
                ssq=o["ssq"] if ssq else None)
        if row:
            blk.set(next_ln_w=i["nln_w"], next_ln_b=i["nln_b"], next_scale=mrow(6), next_shift=mrow(7), next_x=o["next_x"],
                    next_xm=o["next_xm"], next_mean=o["next_mean"], next_rstd=o["next_rstd"])
        self.blk = blk

    def feed(self, prev: "Block") -> None:
        """this block reads what `prev` wrote for the block that follows it"""
        self.blk.set(x_in=prev.out["next_x"], xm1=prev.out["next_xm"])

    def poison(self, B: int) -> None:
        for name, f in self.flat.items():
            f.fill_(-7.0 if f.dtype == BF else -7.5)
        self.out["ssq"][: B * self.N].zero_()  # (the caller zeroes SSQ: the tiled qkv GEMM adds two addends per word)

    def run(self, row_gemms: int, train: bool, max_wgs: int, entry: str = "dl_dit_block_fwd", B: int | None = None):
        """poison every output, run the block over its first B samples (default: all) and return copies of the allocations"""
        from diffulab_amd import ops

        B = self.B if B is None else B
        self.poison(B)
        self.blk.row_gemms, self.blk.max_workgroups, self.blk.B = row_gemms, max_wgs, B
        if entry == "dl_dit_block_fwd":
            ops.dit_block_fwd(self.blk, train)
        else:
            assert ops.dit_block_fwd_chain(self.blk, train), "dl_dit_block_fwd_chain declined a block it should serve"
        torch.cuda.synchronize()
        self.blk.B = self.B
        return {name: f.clone() for name, f in self.flat.items()}


def _poison(t):
    return -7.0 if t.dtype == BF else -7.5


def assert_same(got: dict, ref: dict, written: tuple = (), frac: tuple = (1, 1)) -> None:
    """got equals ref bit for bit over the leading frac[0] / frac[1] of every output (its first samples: every output is
    sample-major), keeps its poison behind that, and its guards; the outputs named in `written` hold finite values there"""
    for name, r in ref.items():
        g = got[name]
        n = (r.numel() - 2 * GUARD) * frac[0] // frac[1]
        assert bool((g[:GUARD] == _poison(g)).all()) and bool((g[GUARD + n :] == _poison(g)).all()), \
            f"{name}: elements in front of or behind the output were overwritten"
        it = torch.int16 if g.dtype == BF else torch.int32
        gi, ri = g[GUARD : GUARD + n].view(it), r[GUARD : GUARD + n].view(it)
        assert torch.equal(gi, ri), f"{name}: {int((gi != ri).sum())} of {n} elements differ"
        if name in written:
            body = g[GUARD : GUARD + n].float()
            assert bool(torch.isfinite(body).all()) and bool((body != _poison(g)).any()), f"{name} not written"


ROW_OUTPUTS = ("qkv", "ssq", "a", "lse", "t1", "x1", "xm2", "mean2", "rstd2", "h", "t2", "next_x", "next_xm", "next_mean", "next_rstd")
TRAIN_OUTPUTS = ("q", "k", "rrms")
MODES = [pytest.param(True, False, id="train"), pytest.param(True, True, id="train-storeU"), pytest.param(False, False, id="inference")]
B_REF = 8
_REF: dict = {}


def reference(train: bool, store_u: bool = False):
    """the block of B_REF samples and what dl_dit_block_fwd's separate launches (bit 3 clear) write for it; computed once per mode"""
    key = (train, store_u)
    if key not in _REF:
        blk = Block(B_REF, 256, seed=100, store_u=store_u)
        ref = blk.run(1, train, B_REF)
        for name in ROW_OUTPUTS + (TRAIN_OUTPUTS if train else ()) + (("u",) if train and store_u else ()):
            body = ref[name][GUARD:-GUARD].float()
            assert bool(torch.isfinite(body).all()) and bool((body != _poison(ref[name])).any()), f"{name} not written by the reference"
        _REF[key] = (blk, ref)
    return _REF[key]


def written(train: bool, store_u: bool = False) -> tuple:
    return ROW_OUTPUTS + (TRAIN_OUTPUTS if train else ()) + (("u",) if train and store_u else ())


@pytest.mark.parametrize("train,store_u", MODES)
@pytest.mark.parametrize("B", [2, 3])
def test_chain_equals_the_five_launches_bit_for_bit(B, train, store_u):
    """one block at B = 2 and 3: QKV, SSQ, Q, K, RRMS, A, LSE, T1, X1, XM2, MEAN2 / RSTD2, H, U where stored, T2, NEXT_X, NEXT_XM,
    NEXT_MEAN / NEXT_RSTD and the guards around each.  In inference Q, K, RRMS (and U) stay untouched in both runs."""
    blk, ref = reference(train, store_u)
    assert_same(blk.run(1 | CHAIN, train, 0, B=B), ref, written(train, store_u), frac=(B, B_REF))
    # the entry point itself does not look at bit 3
    assert_same(blk.run(1, train, 0, entry="dl_dit_block_fwd_chain", B=B), ref, written(train, store_u), frac=(B, B_REF))
    if not train:
        for name in TRAIN_OUTPUTS + ("u",):
            assert bool((ref[name] == _poison(ref[name])).all()), f"{name} written in inference"


@pytest.mark.parametrize("train,store_u", MODES)
def test_bit_3_toggles_the_chain_on_one_block(train, store_u):
    """B = 8 (the fewest samples the separate launches serve): dl_dit_block_fwd with bit 3 set and clear on the same block"""
    blk, ref = reference(train, store_u)
    assert_same(blk.run(1 | CHAIN, train, B_REF), ref, written(train, store_u))
    assert_same(blk.run(1 | CHAIN, train, 0), ref, written(train, store_u))


@pytest.mark.parametrize("train", [True, False], ids=["train", "inference"])
@pytest.mark.parametrize("max_wgs", [1, 2])
def test_a_workgroup_carries_several_samples_in_turn(max_wgs, train):
    """B = 3 on one and on two workgroups: the operand rings, the LDS and the fences are reused across samples"""
    blk, ref = reference(train)
    assert_same(blk.run(1 | CHAIN, train, max_wgs, B=3), ref, written(train), frac=(3, B_REF))


def test_two_blocks_in_a_row():
    """block 0's NEXT_X / NEXT_XM are block 1's X_IN / XM1: both blocks equal the unfused sequence (B = 8 for it; the chain also
    at B = 3 on two workgroups)"""
    b0, b1 = Block(B_REF, 256, seed=11), Block(B_REF, 256, seed=12)
    b1.feed(b0)
    ref = (b0.run(1, True, B_REF), b1.run(1, True, B_REF))
    for kw, frac in ((dict(max_wgs=B_REF), (1, 1)), (dict(max_wgs=2, B=3), (3, B_REF))):
        g0 = b0.run(1 | CHAIN, True, **kw)
        g1 = b1.run(1 | CHAIN, True, **kw)
        assert_same(g0, ref[0], written(True), frac)
        assert_same(g1, ref[1], written(True), frac)


@pytest.mark.parametrize("N", [128, 512])
def test_other_token_counts_are_refused_and_the_driver_runs_its_launch_sequence(N):
    """N != 256: a panel is not a sample.  dl_dit_block_fwd_chain declines; dl_dit_block_fwd with bit 3 set gives what it gives
    with the bit clear (these token counts have no row-complete GEMMs either: bit 0 is clear)"""
    from diffulab_amd import ops

    blk = Block(4 if N == 128 else 2, N, seed=N, row=False, store_u=True)
    for flags in (CHAIN, 1 | CHAIN):
        blk.blk.row_gemms, blk.blk.max_workgroups = flags, 0
        assert not ops.dit_block_fwd_chain(blk.blk, True)
    ref = blk.run(0, True, 0)
    assert_same(blk.run(CHAIN, True, 0), ref, ("qkv", "a", "t1", "x1", "xm2", "h", "u", "t2"))


def test_a_block_without_ssq_is_refused_and_the_driver_runs_its_launch_sequence():
    """no SSQ buffer (QK-norm + RoPE as their own pass): the chain has no such phase"""
    from diffulab_amd import ops

    blk = Block(B_REF, 256, seed=5, ssq=False)
    blk.blk.row_gemms, blk.blk.max_workgroups = 1 | CHAIN, B_REF
    assert not ops.dit_block_fwd_chain(blk.blk, True)
    ref = blk.run(1, True, B_REF)
    assert_same(blk.run(1 | CHAIN, True, B_REF), ref, ("qkv", "q", "k", "rrms", "a", "t1", "x1", "xm2", "h", "t2", "next_x", "next_xm"))
