"""fp64 references and element-wise error bounds for the bf16-regime token, embedding and layout kernels: every entry point of
csrc/tokens.hip, the stem / head / conditioning / reduction kernels of csrc/embed.hip, the kernels of csrc/unet.hip outside GroupNorm
and attention, and the SwiGLU of csrc/norm.hip (imported by the test modules; not a conftest).  Builds on
tests/elementwise_bounds.py (constants, store terms, poisoned buffers) and on the V arithmetic of tests/f32_bounds.py: a V carries
the fp64 value of an intermediate and a bound on the distance of the kernel's f32 intermediate from it; one named term per rounding.

Operands are bf16 or f32, so fp64 holds them, their sums and their products exactly.  What differs from the fp32 regime:

  stores     a bf16 output adds half a bf16 ulp of |ref| + err (b16, = eb.store_bf16 with an exact zero kept exact); an f32 output is
             the last f32 rounding of the V arithmetic itself.
  sigmoid    sigmoid_f / silu_f / dsilu_f (csrc/common.h: v_rcp_f32 of 1 + __expf(-x)) carry the relative error eb.silu_dev_rel
             documents, (1.5 |x| + 6) 2^-24; dsilu_f = s (1 + x (1 - s)) is then assembled from it with the V arithmetic.
  __expf     see the table below: its relative error grows with |x| and passes the 8-ulp cap on every range swept, so no relative
             allowance is taken.  For arguments <= 0 (dgelu_f: exp(-x^2 / 2); ddt_cond_bwd_k: exp(-u), exp(-z) at u, z >= 0) the
             ABSOLUTE error measured over [-88, 0] bounds it: FAST_EXP_ABS units of 2^-24 on a result in (0, 1].  For arguments in
             (0, 16] (ddt_cond_bwd_k at u < 0; z = silu(u) >= -0.28) the allowance is twice the maximum measured over the range that
             holds |x| ([-4, 4], [-8, 8], [-16, 16]); it never reaches an output as a relative term: E = exp(|u|) enters through
             s = 1 / (1 + E) only, where the V arithmetic multiplies it by s (1 - s) <= exp(-|u|) -- the product stays under
             2.1 ulp of 1.  The cases keep |u| <= 16 (fast_exp_ asserts it).
  reductions ACC_C depth 2^-24 sum |term| (fb.fsum).  Where the kernel fixes the order, depth is its chain length (stated at each
             reference); where partial sums meet in f32 atomics, depth is the number of terms; the previous value of a += output is
             one more term.
  movement   gather, restore, copies, layout changes, im2col, the weight casts, pick / stuff, expand at scale 1, head split / merge
             without rotary tables: compared bit for bit (bound None), every zero the kernel writes included.  Where f32 becomes
             bf16 the expected bits are tensor.to(torch.bfloat16): round to nearest even.

Library-function allowances: expf, erff, sinf, cosf, sqrtf and the divisions as recorded in tests/f32_bounds.py.  The fast exponential
was measured the same way (scripts/f32_libm_ulp.hip, built with the flags of csrc/Makefile, every third f32 bit pattern, against fp64):

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics scripts/f32_libm_ulp.hip -o f32_libm_ulp && ./f32_libm_ulp

    function    range swept     measured max                           constant
    __expf      [-88, 0]        8.4e6 ulp at x = -87.34 (results below the normal range are flushed to zero); NOT USED
    __expf      [-88, 0]        0.8992 x 2^-24 absolute (x = -0.434)   FAST_EXP_ABS = 2      (units of 2^-24)
    __expf      [-4, 4]         4.0258 ulp (x = 3.46)                  FAST_EXP_ULP[4]  = 9  > ULP_CAP: only under s (1 - s), see above
    __expf      [-8, 8]         7.6843 ulp (x = 7.62)                  FAST_EXP_ULP[8]  = 16 > ULP_CAP: likewise
    __expf      [-16, 16]       15.0879 ulp (x = 15.94)                FAST_EXP_ULP[16] = 31 > ULP_CAP: likewise
"""

from __future__ import annotations

import math

import torch

import elementwise_bounds as eb
import f32_bounds as fb
from f32_bounds import V, add, bits, const, exact, fsum, mul, neg, sub

U = eb.U32
ACC_C = eb.ACC_C
BF = torch.bfloat16
FAST_EXP_ABS = 2  # units of 2^-24, arguments in [-88, 0]
FAST_EXP_ULP = {4: 9, 8: 16, 16: 31}  # ulps of the result, arguments in (0, R]
COS_EPS = 1e-8

ENTRY_POINTS = [
    # tokens.hip
    "dl_gather_tokens", "dl_scatter_tokens_add", "dl_restore_tokens", "dl_masked_colsum", "dl_gated_residual_fwd", "dl_copy_rows3d",
    "dl_ddt_cond_fwd", "dl_ddt_cond_bwd",
    # embed.hip
    "dl_patchify", "dl_unpatchify", "dl_timestep_embedding", "dl_cond_combine_fwd", "dl_cond_combine_bwd", "dl_cond_combine_dense_fwd",
    "dl_cond_combine_dense_bwd", "dl_silu_bwd", "dl_gelu_bwd", "dl_heads_split_rope", "dl_heads_merge_rope_bwd", "dl_colsum",
    "dl_colsum_det", "dl_colsum_batched", "dl_reduce_rows_f32", "dl_reduce_rows_batched_f32", "dl_cosine_rows_fwd", "dl_cosine_rows_bwd",
    # unet.hip
    "dl_nchw_to_nhwc", "dl_nhwc_to_nchw", "dl_im2col3x3", "dl_cast_conv3x3_weight", "dl_cast_conv3x3_weights_batched",
    "dl_conv3x3_wgrad_fold", "dl_conv3x3_wgrad_fold_batched", "dl_reduce2x2", "dl_expand2x2", "dl_resample2x2_pair", "dl_pick2x2",
    "dl_stuff2x2", "dl_rowbias_add", "dl_rowbias_bwd", "dl_geglu_fwd", "dl_geglu_bwd", "dl_add_bf16", "dl_copy2d_bf16",
    # norm.hip
    "dl_swiglu_fwd", "dl_swiglu_bwd",
]
assert len(ENTRY_POINTS) == 46 and len(set(ENTRY_POINTS)) == 46


# ------------------------------------------------------------------------------------------------------------------ stores, device functions
def b16(v: V):
    """a bf16 store: half a bf16 ulp of |ref| + err; an exact zero stays exact"""
    m = v.mag
    return v.ref, v.err + torch.where(m == 0, torch.zeros_like(m), eb.half_ulp(m, 8))


def o32(v: V):
    """an f32 output: the V arithmetic's last rounding is the store"""
    return v.ref, v.err


def sigmoid_dev(x: V) -> V:
    """sigmoid_f: the argument's error through s' <= 1/4, the device's relative error eb.silu_dev_rel on the result"""
    s = torch.sigmoid(x.ref)
    return V(s, 0.25 * x.err + eb.silu_dev_rel(x.mag) * s + fb.FLUSH)


def silu_dev(x: V) -> V:
    """silu_f = x * sigmoid_f(x)"""
    return mul(x, sigmoid_dev(x))


def dsilu_dev(x: V) -> V:
    """dsilu_f = s * (1 + x * (1 - s))"""
    s = sigmoid_dev(x)
    one = const(1.0, x)
    return mul(s, add(one, mul(x, sub(one, s))))


def fast_exp_(a: V) -> V:
    """__expf(a): the argument's error through the derivative, then the measured allowance of the docstring table"""
    assert float(a.mag.max()) <= 16.0 or float((a.ref + a.err).max()) <= 0.0, "positive arguments beyond the measured range"
    assert float(a.mag.max()) <= 88.0
    r = a.ref.exp()
    e = r * torch.expm1(a.err)
    hu = 2 * fb.half_ulp(r + e)  # one ulp of the result
    m = a.mag
    pos = torch.where(m <= 4, FAST_EXP_ULP[4] * hu, torch.where(m <= 8, FAST_EXP_ULP[8] * hu, FAST_EXP_ULP[16] * hu))
    allow = torch.where(a.ref + a.err <= 0, torch.full_like(r, FAST_EXP_ABS * U), pos)
    return V(r, e + allow + fb.FLUSH)


def sigmoid_fast_div(x: V) -> V:
    """1.f / (1.f + __expf(-x)) with the IEEE division (ddt_cond_bwd_k)"""
    return fb.rcp(add(const(1.0, x), fast_exp_(neg(x))))


def dgelu_dev(x: V) -> V:
    """dgelu_f (csrc/common.h): 0.5f * (1 + erff(x c1)) + x * c2 * __expf(-0.5f * x * x)"""
    cdf = fb.scale2(add(const(1.0, x), fb.erf_(mul(x, fb._cst(fb.INV_SQRT2, x)))), 0.5)
    pdf = fast_exp_(mul(fb.scale2(neg(x), 0.5), x))
    return add(cdf, mul(mul(x, fb._cst(0.3989422804014327, x)), pdf))


def _rows(t, rows_per_mod, M):
    return t.repeat_interleave(rows_per_mod, 0)[:M]


def sum_ref(terms, out0, depth):
    """out0 [C] (f32, += semantics) + sum over dim 0 of terms [R, C] (exact operands) through at most `depth` f32 additions"""
    t = torch.cat([out0.double()[None], terms.double()], 0)
    return o32(fsum(V(t), 0, depth))


# ------------------------------------------------------------------------------------------------------------------ tokens.hip
def gather_ref(src, idx, keep, B, N, k):
    D = src.shape[1]
    g = src.reshape(B, N, D).gather(1, idx.reshape(B, k).long()[:, :, None].expand(B, k, D))
    if keep is not None:
        g = torch.where((keep != 0)[:, None, None], g, torch.zeros_like(g))
    return {"dst": bits(g.reshape(B * k, D))}


def scatter_add_ref(src, idx, dst0, B, N, k):
    """dst[b, idx[b, j]] += src[b, j]: one f32 addition, one bf16 store; rows no index names keep their bits (bound 0)"""
    D = src.shape[1]
    ii = idx.reshape(B, k).long()[:, :, None].expand(B, k, D)
    upd = torch.zeros(B, N, D, dtype=torch.float64, device=src.device).scatter(1, ii, src.double().reshape(B, k, D))
    hit = torch.zeros(B, N, D, dtype=torch.bool, device=src.device).scatter(1, ii, torch.ones(B, k, D, dtype=torch.bool, device=src.device))
    r, e = b16(add(exact(dst0).map(lambda u: u.reshape(B, N, D)), V(upd)))
    return {"dst": (r.reshape(B * N, D), torch.where(hit, e, torch.zeros_like(e)).reshape(B * N, D))}


def restore_ref(xd, inv, mask, B, N, k):
    D = xd.shape[1]
    j = inv.reshape(B, N).long()
    g = xd.reshape(B, k, D).gather(1, j.clamp_min(0)[:, :, None].expand(B, N, D))
    return {"out": bits(torch.where((j >= 0)[:, :, None], g, mask.to(BF)[None, None, :]).reshape(B * N, D))}


def masked_colsum_ref(x, sel, out0):
    """slab partials meet in f32 atomics: depth = the selected rows + the previous value"""
    xm = torch.where((sel < 0)[:, None], x.double(), torch.zeros(1, dtype=torch.float64, device=x.device))
    return {"out": sum_ref(xm, out0, int((sel < 0).sum()) + 1)}


def gated_residual_ref(x, t, gate, rows_per_mod):
    M = x.shape[0]
    return {"out": b16(add(exact(x), mul(exact(_rows(gate, rows_per_mod, M)), exact(t))))}


def ddt_fwd_ref(enc, temb, N):
    u = add(exact(enc), exact(temb.repeat_interleave(N, 0)))
    return {"out": b16(silu_dev(silu_dev(u)))}


def ddt_bwd_ref(dsz, enc, temb, dtemb0, N):
    """ddt_cond_bwd_k line by line; dtemb: a slab's rows in order, the slabs and the previous value through atomics: depth N + 1"""
    M, D = enc.shape
    B = M // N
    u = add(exact(enc), exact(temb.repeat_interleave(N, 0)))
    one = const(1.0, u)
    su = sigmoid_fast_div(u)
    z = mul(u, su)
    dz = mul(su, add(one, mul(u, sub(one, su))))
    sz = sigmoid_fast_div(z)
    d = mul(mul(exact(dsz), mul(sz, add(one, mul(z, sub(one, sz))))), dz)
    t = V(torch.cat([dtemb0.double()[:, None], d.ref.reshape(B, N, D)], 1), torch.cat([torch.zeros_like(dtemb0.double())[:, None], d.err.reshape(B, N, D)], 1))
    return {"denc": b16(d), "dtemb": o32(fsum(t, 1, N + 1))}


# ------------------------------------------------------------------------------------------------------------------ embed.hip
def patchify_ref(x, p, ld, order_cpp: bool):
    return {"tok": bits(fb.patchify_ref(x, p, ld, order_cpp)["tok"][0].to(BF))}


def unpatchify_ref(tok, B, C, H, W, p):
    """tok f32 [B gh gw, ld] with features (p1 p2 c) -> img f32 [B, C, H, W]"""
    gh, gw = H // p, W // p
    t = tok[:, :C * p * p].reshape(B, gh, gw, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)
    return {"img": bits(t.contiguous())}


def timestep_ref(t, dim, max_period):
    """[cos(t f_j) | sin(t f_j)], f_j = expf((float)j * c), c = (float)(-ln(P) / half) rounded once on the host"""
    B, half = t.shape[0], dim // 2
    j = torch.arange(half, dtype=torch.float64, device=t.device)[None].expand(B, half)
    c = -math.log(max_period) / half
    f = fb.exp_(mul(V(j), V(torch.full_like(j, c), torch.full_like(j, abs(fb.f32c(c) - c)))))
    f = V(f.ref, torch.where(j == 0, torch.zeros_like(f.err), f.err))  # expf(0) = 1
    a = mul(exact(t).map(lambda u: u[:, None].expand(B, half)), f)
    cs, sn = b16(fb.cos_(a)), b16(fb.sin_(a))
    return {"emb": (torch.cat([cs[0], sn[0]], 1), torch.cat([cs[1], sn[1]], 1))}


def cond_fwd_ref(e, addend):
    """addend: table[idx] or the dense pe, or None (emb = e bit for bit)"""
    v = exact(e) if addend is None else add(exact(e), exact(addend))
    return {"emb": o32(v), "act": b16(silu_dev(v))}


def cond_bwd_ref(dact, emb, idx, dtable0):
    """demb = dact * dsilu_f(emb) (f32 and its bf16 copy); dtable[label] += the demb of its samples in batch order by the first
    sample that carries the label: a chain of cnt additions (cnt - 1 in the accumulator, one into the table)"""
    g = mul(exact(dact), dsilu_dev(exact(emb)))
    res = {"demb": o32(g), "demb16": b16(g)}
    if dtable0 is not None:
        n_cls = dtable0.shape[0]
        onehot = torch.nn.functional.one_hot(idx, n_cls).double()
        cnt = onehot.sum(0)[:, None]
        d0 = dtable0.double()
        mag = d0.abs() + onehot.t() @ g.mag
        res["dtable"] = (d0 + onehot.t() @ g.ref, onehot.t() @ g.err + ACC_C * cnt * U * mag + fb.TINY * (cnt > 0))
    return res


def silu_bwd_ref(dy, pre):
    return {"dx": b16(mul(exact(dy), dsilu_dev(exact(pre))))}


def gelu_bwd_ref(dy, pre):
    return {"dx": b16(mul(exact(dy), dgelu_dev(exact(pre))))}


def _rot_rows(v: V, cs, sn, n_src, H, rot, inverse):
    """v [B n_src, H 64]: the rotary pairs of the first `rot` channels of every head, row n of a sample with table row n"""
    M = v.ref.shape[0]
    tok = torch.arange(M, device=v.ref.device) % n_src
    c, s, on = fb._rope_cs(cs, sn, tok, H, 64, rot)
    return fb._rotate(v, c, s, on, inverse)


def heads_split_ref(src, cs, sn, B, H, n_src, rot):
    """-> the [B, H, n_src, 64] rows the kernel writes at n_off"""
    v = exact(src)
    if cs is None:
        return {"dst": bits(src.reshape(B, n_src, H, 64).permute(0, 2, 1, 3).contiguous())}
    r = _rot_rows(v, cs, sn, n_src, H, rot, False)
    # channels at or above rot are moved only: exact (their bound is 0)
    keep = lambda u: u.reshape(B, n_src, H, 64).permute(0, 2, 1, 3)  # noqa: E731
    ref, err = b16(V(keep(r.ref), keep(r.err)))
    moved = (torch.arange(64, device=src.device) >= rot).expand_as(ref)
    return {"dst": (ref, torch.where(moved, torch.zeros_like(err), err))}


def heads_merge_ref(dst_grad, src0, cs, sn, B, H, n_src, rot):
    """dst_grad: the [B, H, n_src, 64] rows at n_off; src0: the previous src_grad (accumulate) or None"""
    g = dst_grad.permute(0, 2, 1, 3).reshape(B * n_src, H * 64)
    if cs is None and src0 is None:
        return {"src": bits(g.contiguous())}
    v = exact(g)
    if cs is not None:
        v = _rot_rows(v, cs, sn, n_src, H, rot, True)
    if src0 is not None:
        v = add(v, exact(src0))
    return {"src": b16(v)}


def colsum_ref(x, out0, depth):
    return {"out": sum_ref(x, out0, depth)}


def colsum_det_depth(R, C, scratch_floats, vec: bool) -> int:
    """dl_colsum_det: a lane's rows of a slab in order (the vector form adds two rows first), the thread rows of the block in order (or
    the (r0 + r1) + (r2 + r3) tree of the scalar forms), then the slabs and the previous value in the fold"""
    slabs = min(-(-R // 256), 512)
    if slabs * C > scratch_floats:
        slabs = scratch_floats // C
    rps = -(-R // slabs)
    slabs = -(-R // rps)
    if vec:
        vl = 1
        while vl * 8 < C and vl < 64:
            vl <<= 1
        nr = 256 // vl
        return -(-rps // nr) + 1 + nr + slabs + 1
    return -(-rps // 4) + 2 + slabs + 1


def reduce_rows_batched_depth(G: int) -> int:
    """a row lane's ceil(G / 16) rows in order, (a + b) + (c + d) per four lanes, the four groups in order, the previous value"""
    return -(-G // 16) + 2 + 4 + 1


def cosine_depth(E: int) -> int:
    """a lane's 8 ceil(E / 512) products in order, four DPP levels and the (r0 + r1) + (r2 + r3) of the row sums"""
    return 8 * -(-E // 512) + 6


def cosine_fwd_ref(p, d, eps=COS_EPS):
    pv, dv = exact(p), exact(d)
    dep = cosine_depth(p.shape[1])
    s, a, b = fsum(mul(pv, dv), 1, dep), fsum(mul(pv, pv), 1, dep), fsum(mul(dv, dv), 1, dep)
    ab = mul(a, b)
    e2 = fb.f32c(fb.f32c(eps) * fb.f32c(eps))
    assert bool((((ab.ref - ab.err) > e2) | ((ab.ref + ab.err) < e2)).all()), "a row too close to the clamp"
    den = fb.sqrt_(V(ab.ref.clamp_min(e2), torch.where(ab.ref > e2, ab.err, torch.zeros_like(ab.err))))
    return {"cos": o32(fb.div(s, den)), "pn2": o32(a), "dn2": o32(b)}


def cosine_bwd_ref(p, d, cosv, pn2, dn2, gscale, gscale_dev, eps=COS_EPS):
    """from the f32 cos, |p|^2, |d|^2 as given: dp = g (d / den - k p), k = 0 where the clamp is active (the kernel's comment)"""
    M, E = p.shape
    a, b, cs = exact(pn2), exact(dn2), exact(cosv)
    ab = mul(a, b)
    e2 = fb.f32c(fb.f32c(eps) * fb.f32c(eps))
    clamped = ab.ref < e2
    assert bool((((ab.ref - ab.err) > e2) | ((ab.ref + ab.err) < e2)).all()), "a row too close to the clamp"
    inv = fb.rcp(fb.sqrt_(V(ab.ref.clamp_min(e2), torch.where(clamped, torch.zeros_like(ab.err), ab.err))))
    kk = fb.div(cs, V(a.ref.clamp_min(fb.f32c(1e-30))))
    kk = V(torch.where(clamped, torch.zeros_like(kk.ref), kk.ref), torch.where(clamped, torch.zeros_like(kk.err), kk.err))
    g = const(fb.f32c(gscale), a) if gscale_dev is None else mul(const(fb.f32c(gscale), a), exact(gscale_dev.reshape(1).expand(M)))
    col = lambda v: v.map(lambda u: u[:, None].expand(M, E))  # noqa: E731
    return {"dp": b16(mul(col(g), sub(mul(exact(d), col(inv)), mul(col(kk), exact(p)))))}


# ------------------------------------------------------------------------------------------------------------------ unet.hip
def im2col_ref(x, B, H, W, C, rows, ld):
    """cols [rows, ld]: column tap C + c of pixel row r = x at the tap's neighbour (zero outside the image); rows past B H W and
    columns past 9 C are zeros"""
    xp = torch.nn.functional.pad(x.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    taps = torch.cat([xp[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)], 3).reshape(B * H * W, 9 * C)
    out = torch.zeros(rows, ld, dtype=x.dtype, device=x.device)
    out[:B * H * W, :9 * C] = taps
    return {"cols": bits(out)}


def cast_conv_ref(w, ldf, ldd):
    """wf[co, tap Ci + ci] = bf16(w[co, ci, tap]); wd[ci, tap' Co + co] = bf16(w[co, ci, 8 - tap']) (the 180-degree rotation)"""
    Co, Ci = w.shape[:2]
    w9 = w.reshape(Co, Ci, 9).to(BF)
    wf = torch.zeros(Co, ldf, dtype=BF, device=w.device)
    wd = torch.zeros(Ci, ldd, dtype=BF, device=w.device)
    wf[:, :9 * Ci] = w9.permute(0, 2, 1).reshape(Co, 9 * Ci)
    wd[:, :9 * Co] = w9.flip(2).permute(1, 2, 0).reshape(Ci, 9 * Co)
    return {"wf": bits(wf), "wd": bits(wd)}


def fold_ref(g, dw0, Co, Ci):
    """g [n_img, 9 Ci, Co] (logical): dw[co, ci, tap] += sum_img g[img, tap Ci + ci, co], the images in order then the previous value:
    a chain of n_img additions"""
    n = g.shape[0]
    t = g.double().reshape(n, 9, Ci, Co).permute(0, 3, 2, 1)  # [n, Co, Ci, 9]
    return {"dw": o32(fsum(V(torch.cat([t, dw0.double().reshape(1, Co, Ci, 9)], 0)), 0, n))}


def reduce2x2_ref(x, B, Hs, Ws, C, scale):
    """scale * (((a + b) + c) + d): the kernels add left to right"""
    t = exact(x).map(lambda u: u.reshape(B, Hs, 2, Ws, 2, C))
    g = lambda i, j: t.map(lambda u: u[:, :, i, :, j, :])  # noqa: E731
    v = mul(const(fb.f32c(scale), g(0, 0)), add(add(add(g(0, 0), g(0, 1)), g(1, 0)), g(1, 1)))
    return {"out": b16(v.map(lambda u: u.reshape(B * Hs * Ws, C)))}


def expand2x2_ref(x, B, Hs, Ws, C, scale):
    up = lambda u: u.reshape(B, Hs, 1, Ws, 1, C).expand(B, Hs, 2, Ws, 2, C).reshape(B * 4 * Hs * Ws, C)  # noqa: E731
    if scale == 1.0:
        return {"out": bits(up(x).contiguous())}
    t = exact(x).map(up)
    return {"out": b16(mul(const(fb.f32c(scale), t), t))}


def pick_ref(x, B, Hs, Ws, C):
    return {"out": bits(x.reshape(B, Hs, 2, Ws, 2, C)[:, :, 0, :, 0, :].reshape(B * Hs * Ws, C).contiguous())}


def stuff_ref(x, B, Hs, Ws, C):
    o = torch.zeros(B, Hs, 2, Ws, 2, C, dtype=x.dtype, device=x.device)
    o[:, :, 0, :, 0, :] = x.reshape(B, Hs, Ws, C)
    return {"out": bits(o.reshape(B * 4 * Hs * Ws, C))}


def rowbias_add_ref(x, e, B, HW, C):
    v = add(exact(x).map(lambda u: u.reshape(B, HW, C)), exact(e).map(lambda u: u[:, None, :].expand(B, HW, C)))
    return {"out": b16(v.map(lambda u: u.reshape(B * HW, C)))}


def rowbias_bwd_ref(dy, B, HW, C):
    """a pixel lane's ceil(HW / 32) pixels in order, then the 32 lanes in order; one bf16 store"""
    return {"de": b16(fsum(exact(dy).map(lambda u: u.reshape(B, HW, C)), 1, -(-HW // 32) + 32))}


def _gelu_erf(g: V) -> V:
    """gelu_erf_f: (0.5f * g) * (1 + erff(g c))"""
    return mul(fb.scale2(g, 0.5), add(const(1.0, g), fb.erf_(mul(g, fb._cst(fb.INV_SQRT2, g)))))


def geglu_fwd_ref(u, F):
    return {"h": b16(mul(exact(u[:, :F]), _gelu_erf(exact(u[:, F:2 * F]))))}


def geglu_bwd_ref(dh, u, F):
    a, g, d = exact(u[:, :F]), exact(u[:, F:2 * F]), exact(dh)
    da = mul(d, _gelu_erf(g))
    cdf = fb.scale2(add(const(1.0, g), fb.erf_(mul(g, fb._cst(fb.INV_SQRT2, g)))), 0.5)
    pdf = fb.exp_(mul(fb.scale2(neg(g), 0.5), g))
    dg = mul(mul(d, a), add(cdf, mul(mul(g, fb._cst(fb.INV_SQRT2PI, g)), pdf)))
    ra, rg = b16(da), b16(dg)
    return {"du": (torch.cat([ra[0], rg[0]], 1), torch.cat([ra[1], rg[1]], 1))}


def swiglu_fwd_ref(u, F):
    return {"h": b16(mul(silu_dev(exact(u[:, :F])), exact(u[:, F:2 * F])))}


def swiglu_bwd_ref(dh, u, F):
    a, b, g = exact(u[:, :F]), exact(u[:, F:2 * F]), exact(dh)
    ra, rb = b16(mul(mul(g, b), dsilu_dev(a))), b16(mul(g, silu_dev(a)))
    return {"du": (torch.cat([ra[0], rb[0]], 1), torch.cat([ra[1], rb[1]], 1))}


def add_ref(a, b):
    return {"out": b16(add(exact(a), exact(b)))}


# ------------------------------------------------------------------------------------------------------------------ judging
def same_bits(a, b) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    iv = torch.int16 if a.element_size() == 2 else torch.int32
    return bool(torch.equal(a.contiguous().view(iv), b.to(a.device).contiguous().view(iv)))


def judge(got: dict, ref: dict) -> dict:
    """-> {output: worst |diff| / bound, or 0.0 / inf for a bit-compare}; every reference and bound must be finite"""
    res = {}
    for name, (r, bound) in ref.items():
        g = got[name]
        assert tuple(g.shape) == tuple(r.shape), (name, tuple(g.shape), tuple(r.shape))
        assert bool(torch.isfinite(r.double()).all()), f"{name}: the reference is not finite"
        if bound is None:
            res[name] = 0.0 if same_bits(g, r) else float("inf")
        else:
            assert bool(torch.isfinite(bound).all()), f"{name}: a bound is not finite"
            res[name] = fb.worst_ratio(g, r, bound)
    return res


def spread(shape, gen, device, lim=12.0, dtype=BF):
    """pre-activations spread over [-lim, lim] with the ends and an exact zero among them"""
    t = (2.0 * torch.rand(shape, generator=gen, device=device) - 1.0) * lim
    f = t.reshape(-1)
    f[0], f[1 % f.numel()], f[2 % f.numel()] = lim, -lim, 0.0
    return t.to(dtype)


# ------------------------------------------------------------------------------------------------------------------ coverage
# every name of ENTRY_POINTS -> the tests of tests/test_bf16_aux_paths_gpu.py that call it
COVERAGE = {
    "dl_gather_tokens": ["test_token_routing", "test_row_grid_second_trip"],
    "dl_scatter_tokens_add": ["test_token_routing", "test_row_grid_second_trip"],
    "dl_restore_tokens": ["test_token_routing", "test_row_grid_second_trip"],
    "dl_masked_colsum": ["test_masked_colsum"],
    "dl_gated_residual_fwd": ["test_gated_residual_and_copy_rows", "test_row_grid_second_trip"],
    "dl_copy_rows3d": ["test_gated_residual_and_copy_rows", "test_row_grid_second_trip"],
    "dl_ddt_cond_fwd": ["test_ddt_cond", "test_row_grid_second_trip"],
    "dl_ddt_cond_bwd": ["test_ddt_cond", "test_rejections"],
    "dl_patchify": ["test_patchify_unpatchify"],
    "dl_unpatchify": ["test_patchify_unpatchify"],
    "dl_timestep_embedding": ["test_timestep_embedding"],
    "dl_cond_combine_fwd": ["test_cond_combine"],
    "dl_cond_combine_bwd": ["test_cond_combine"],
    "dl_cond_combine_dense_fwd": ["test_cond_combine"],
    "dl_cond_combine_dense_bwd": ["test_cond_combine"],
    "dl_silu_bwd": ["test_act_bwd"],
    "dl_gelu_bwd": ["test_act_bwd"],
    "dl_heads_split_rope": ["test_heads", "test_rejections"],
    "dl_heads_merge_rope_bwd": ["test_heads", "test_rejections"],
    "dl_colsum": ["test_colsum"],
    "dl_colsum_det": ["test_colsum"],
    "dl_colsum_batched": ["test_colsum_batched"],
    "dl_reduce_rows_f32": ["test_reduce_rows", "test_rejections"],
    "dl_reduce_rows_batched_f32": ["test_reduce_rows_batched", "test_rejections"],
    "dl_cosine_rows_fwd": ["test_cosine_rows", "test_rejections"],
    "dl_cosine_rows_bwd": ["test_cosine_rows", "test_rejections"],
    "dl_nchw_to_nhwc": ["test_layout_and_glue"],
    "dl_nhwc_to_nchw": ["test_layout_and_glue"],
    "dl_im2col3x3": ["test_im2col"],
    "dl_cast_conv3x3_weight": ["test_conv_weight_cast_and_fold"],
    "dl_cast_conv3x3_weights_batched": ["test_conv_tables"],
    "dl_conv3x3_wgrad_fold": ["test_conv_weight_cast_and_fold"],
    "dl_conv3x3_wgrad_fold_batched": ["test_conv_tables"],
    "dl_reduce2x2": ["test_resamplers"],
    "dl_expand2x2": ["test_resamplers"],
    "dl_resample2x2_pair": ["test_resamplers"],
    "dl_pick2x2": ["test_resamplers", "test_rejections"],
    "dl_stuff2x2": ["test_resamplers", "test_rejections"],
    "dl_rowbias_add": ["test_rowbias", "test_rejections"],
    "dl_rowbias_bwd": ["test_rowbias", "test_rejections"],
    "dl_geglu_fwd": ["test_glu", "test_rejections"],
    "dl_geglu_bwd": ["test_glu", "test_rejections"],
    "dl_add_bf16": ["test_layout_and_glue"],
    "dl_copy2d_bf16": ["test_layout_and_glue"],
    "dl_swiglu_fwd": ["test_glu"],
    "dl_swiglu_bwd": ["test_glu"],
}
