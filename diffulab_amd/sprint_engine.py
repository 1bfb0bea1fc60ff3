"""Host-side runtime of SprintDiT (simple_dit): the DiT engine's arena / shadows / conditioning path with the block stack cut
into three stages and the SPRINT token routing between them (reference networks/denoisers/sprint.py:505-573):

    encoder blocks (all N tokens) -> gather the kept tokens -> deep blocks (k tokens, RoPE rows picked by position index)
    -> restore into a mask-token canvas -> fuse Linear(2D -> D) on [restored ; encoder output] -> decoder blocks -> last layer

Inside a stage the launch sequence is the DiT engine's (gated residuals absorbed by the next LayerNorm-modulate kernel, weight
gradients on the side stream); at a stage boundary the pending residual is materialised by dl_gated_residual_fwd and its backward
is dl_gate_bwd.  The concatenation [restored ; encoder output] is one [B*N, 2D] buffer written in place by the restore kernel
(left half) and the encoder's last residual (right half), so `fuse` is a single GEMM with K = 2D.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import Tensor

from . import ops, tuning
from .engine import DiTDims, DiTEngine, Modulation, ParamLayout, SideWork, _rup, rope_grid_tables


@dataclass
class SprintDims(DiTDims):
    encoder_depth: int = 2
    deep_layers_depth: int = 8
    decoder_depth: int = 2
    drop_rate: float = 0.75

    def __post_init__(self) -> None:
        super().__post_init__()
        self.depth = self.encoder_depth + self.deep_layers_depth + self.decoder_depth

    def n_kept(self, S: int) -> int:
        """sprint.py:342"""
        return max(1, int(S * (1.0 - float(self.drop_rate))))


@dataclass
class Route:
    """token routing of one forward: idx int32 [B, k] kept positions (ascending per sample), inv int32 [B, N] their inverse
    (-1 = the canvas keeps the mask token there; every entry of a sample whose deep path is dropped), keep int32 [B] (0 = deep
    path dropped) or None, skip_deep: the p >= 1 branch (no deep layers at all)"""
    idx: Tensor | None
    inv: Tensor
    keep: Tensor | None
    k: int
    skip_deep: bool = False
    pos_lat: Tensor | None = None  # joint form: RoPE table row of every [text ; kept image] token, int32 [B * (Lc + k)]


class SprintEngine(DiTEngine):
    def _make_layout(self, d: SprintDims) -> ParamLayout:
        D = d.inner_dim
        pre = ([f"layers.{i}." for i in range(d.encoder_depth)] + [f"deep_layers.{i}." for i in range(d.deep_layers_depth)]
               + [f"decoder_layers.{i}." for i in range(d.decoder_depth)])
        return ParamLayout(d, pre, extra=(("mask_token", (1, 1, D)), ("fuse.weight", (D, 2 * D))))

    def _extra_shadows(self, reg) -> None:
        reg("fuse.weight", self.d.inner_dim, 2 * self.d.inner_dim)

    # ------------------------------------------------------------------ workspace
    def _alloc(self, B: int, H: int, W: int, train: bool, k: int | None = None) -> None:  # type: ignore[override]
        d, z = self.d, self._z
        p = d.patch_size
        gh, gw = H // p, W // p
        N = gh * gw
        k = N if k is None else k
        key = (B, H, W, train, k)
        if self._cached(key):
            return
        D = d.inner_dim
        for n in (N, k):
            if n % 64 or (n > 256 and (n % 256 or n > ops.ATTN_MAX_TOKENS)):
                raise NotImplementedError(f"SprintDiT HIP path: token counts must be multiples of 64 up to 256, or of 256 up to "
                                          f"{ops.ATTN_MAX_TOKENS} (grid {gh}x{gw} = {N} tokens, {k} kept)")
        M = B * N
        F = d.mlp_ratio * D
        ops.check_row_extent(M, max(2 * F, 6 * D), "SprintDiT HIP path")
        w: dict[str, object] = {}
        self._cond_buffers(w, B, H, W, train, train and self._grouped_widths())
        ne, nd = d.encoder_depth, d.deep_layers_depth
        tokens = [N] * ne + [k] * nd + [N] * d.decoder_depth
        blk = []
        for nt in tokens:
            a = self._dit_block_buffers(B, nt, train)
            if train:
                a["dwb"] = z(2, B, 2, D, dtype=torch.float32)
            blk.append(a)
        w["blk"] = blk
        w["x_stem"] = z(M, D)
        w["x"] = [w["x_stem"]]               # (_stem_fwd writes the patch embedding into ws["x"][0])
        w["cat"] = z(M, 2 * D)               # [restored canvas | encoder output]
        w["xd0"], w["xd_out"] = z(B * k, D), z(B * k, D)
        w["xfuse"], w["xdec"] = z(M, D), z(M, D)
        if train:
            for nt in {N, k}:  # chain scratch per token count
                w[f"s{nt}"] = self._dit_chain_buffers(B, nt)
            w["dleft"], w["dright"], w["dxd"] = z(M, D), z(M, D), z(B * k, D)
            if D <= 512 and tuning.on("DL_QK_INPLACE"):  # scale-gradient partials of the in-place QK-norm backward (ops.qk_inplace_ok)
                w["qk_part"] = torch.empty(1024 * 2 * D, device=self.dev, dtype=torch.float32)
        self._publish(w, key, (B, H, W, gh, gw, N, M, _rup(B, 64), p * p * d.output_channels), (gh, gw),
                      lambda: rope_grid_tables(gh, gw, d.rope_axes_dim, d.rope_base))

    def _dit_chain_buffers(self, B: int, nt: int) -> dict:
        """scratch of the backward chain over B * nt tokens (shared by every block with that token count)"""
        d, z = self.d, self._z
        D, Hh, mt = d.inner_dim, d.num_heads, B * nt
        return {"dxa": z(mt, D), "dxb": z(mt, D), "dxm": z(mt, D), "da": z(mt, D), "dh": z(mt, d.mlp_ratio * D),
                "dq": z(B, Hh, nt, 64), "dk": z(B, Hh, nt, 64), "dv": z(B, Hh, nt, 64)}

    # ------------------------------------------------------------------ stages
    def _stage_fwd(self, blocks: range, xin: Tensor, nt: int, pos: Tensor | None, out: Tensor) -> None:
        """DiT blocks `blocks` (indices into the block list) over xin [B*nt, D]; the stage output (last gated residual
        materialised) is written to `out` (rows may be strided)"""
        w, D = self.ws, self.d.inner_dim
        cos, sin = self._rope[(self.geo[3], self.geo[4])]
        pend = None
        for bi in blocks:
            a = w["blk"][bi]
            a["xin"] = xin if pend is None else a["x0"]
            pend = self._dit_block_fwd(a, self.prefixes[bi], a["xin"], pend, Modulation(w["mod"], None, bi * 6 * D, D, nt), nt, cos, sin,
                                       pos)
        ops.gated_residual_fwd(*pend, nt, out)

    def _stage_bwd(self, blocks: range, dx: Tensor, nt: int, pos: Tensor | None, dfe: dict[int, Tensor], sw: SideWork) -> Tensor:
        """backward of _stage_fwd: dx = gradient at the stage output, contiguous bf16 [B*nt, D] (overwritten); returns the
        gradient at the stage input.  dfe: {block index: auxiliary-loss gradient at that block's output}"""
        w, B, D = self.ws, self.geo[0], self.d.inner_dim
        cos, sin = self._rope[(self.geo[3], self.geo[4])]
        mod, dmod = w["mod"], w["dmod32"]
        blocks = list(blocks)
        last = blocks[-1]
        if last in dfe:
            ops.add_bf16(dx, dfe[last], dx)
        ml = last * 6 * D
        ops.gate_bwd(dx, w["blk"][last]["t2"], mod[:, ml + 5 * D : ml + 6 * D], nt, w["blk"][last]["wg"]["dt2"],
                     dmod[:, ml + 5 * D : ml + 6 * D])
        for j in reversed(range(len(blocks))):
            bi = blocks[j]
            a = w["blk"][bi]
            prev = dres = None
            if j > 0:
                bp = blocks[j - 1]
                prev, dres = (w["blk"][bp]["t2"], bp * 6 * D + 5 * D, w["blk"][bp]["wg"]["dt2"]), dfe.get(bp)
            m = Modulation(mod, dmod, bi * 6 * D, D, nt, part=a["dwb"], groups=B)
            dx = self._dit_block_bwd(a, a["wg"], self.prefixes[bi], a["xin"], dx, prev, dres, w[f"s{nt}"], m, nt, cos, sin, sw, pos)
            self._end_block(sw, bi)
        return dx

    # ------------------------------------------------------------------ forward
    def forward(self, x: Tensor, t: Tensor, y_eff: Tensor | None, train: bool = True, refresh: bool = True,
                route: Route | None = None) -> Tensor:
        d = self.d
        B, C, H, W = x.shape
        assert C == d.input_channels and x.dtype == torch.float32 and x.is_cuda
        route = route if route is not None else self.route
        assert route is not None, "SprintEngine.forward needs the token routing of this step"
        self._alloc(B, H, W, train, route.k)
        if refresh:
            self.refresh_shadows(force=train)
        w, sh = self.ws, self.sh
        _, _, _, gh, gw, N, M, Bp, Fo = self.geo
        D, L, k = d.inner_dim, d.depth, route.k
        ne, nd = d.encoder_depth, d.deep_layers_depth
        self._train, self._yeff, self._route = train, y_eff, route
        mod = self._stem_fwd(x, t, y_eff)
        cat = w["cat"]
        self._stage_fwd(range(0, ne), w["x_stem"], N, None, cat[:, D:])
        mask = self.P("mask_token").view(D)
        if route.skip_deep:
            ops.restore_tokens(w["xd_out"], route.inv, mask, cat[:, :D], B, N, k, D)  # inv == -1 everywhere: mask-token canvas
        else:
            ops.gather_tokens(cat[:, D:], route.idx, w["xd0"], B, N, k, D)
            self._stage_fwd(range(ne, ne + nd), w["xd0"], k, route.idx.view(-1), w["xd_out"])
            ops.restore_tokens(w["xd_out"], route.inv, mask, cat[:, :D], B, N, k, D)
        ops.gemm_nt(cat, sh["fuse.weight|f"], w["xfuse"], M=M, N=D, K=2 * D)
        self._stage_fwd(range(ne + nd, L), w["xfuse"], N, None, w["xdec"])
        return self._head_fwd(Modulation(mod, None, L * 6 * D, D, N), w["xdec"])

    route: Route | None = None

    def feature(self, kblk: int) -> Tensor:
        """output of encoder block k (``layers[k]``, the blocks a REPA hook can attach to) of the last train-mode forward"""
        assert self._train and 0 <= kblk < self.d.encoder_depth
        B, N, D = self.geo[0], self.geo[5], self.d.inner_dim
        if kblk + 1 < self.d.encoder_depth:
            return self.ws["blk"][kblk + 1]["x0"].view(B, N, D)
        return self.ws["cat"].view(B, N, 2 * D)[:, :, D:]

    # ------------------------------------------------------------------ backward
    def backward(self, dpred: Tensor, dfeats: dict[int, Tensor] | None = None) -> None:
        assert self._train and self.grads is not None
        d, w, sh = self.d, self.ws, self.sh
        B, H, W, gh, gw, N, M, Bp, Fo = self.geo
        D, L = d.inner_dim, d.depth
        ne, nd = d.encoder_depth, d.deep_layers_depth
        route = self._route
        k = route.k
        dfe = self._dfeat_rows(dfeats)
        mod, dmod = w["mod"], w["dmod32"]
        dmod[:B].zero_()
        sN = w[f"s{N}"]

        # head
        self._head_bwd(dpred, sN["dxm"])
        Modulation(mod, dmod, L * 6 * D, D, N).ln_bwd(sN["dxm"], w["xdec"], None, None, 0, w["meanf"], w["rstdf"], None, sN["dxa"], None)
        sw = SideWork(self)
        dxf = self._stage_bwd(range(ne + nd, L), sN["dxa"], N, None, {}, sw)
        # fuse: xfuse = [restored | enc] Wf^T
        ops.gemm_tn(dxf, w["cat"], self.G("fuse.weight"))  # (main stream: dxf is chain scratch that the next stage reuses)
        wt = sh["fuse.weight|t"]
        ops.gemm_nt(dxf, wt[:D], w["dleft"], M=M, N=D, K=D)
        ops.gemm_nt(dxf, wt[D:], w["dright"], M=M, N=D, K=D)
        ops.masked_colsum(w["dleft"], route.inv.view(-1), self.G("mask_token").view(D), M, D)
        if not route.skip_deep:
            ops.gather_tokens(w["dleft"], route.idx, w["dxd"], B, N, k, D, keep=route.keep)
            dxd0 = self._stage_bwd(range(ne, ne + nd), w["dxd"], k, route.idx.view(-1), {}, sw)
            ops.scatter_tokens_add(dxd0, route.idx, w["dright"], B, N, k, D)
        elif self.reducer is not None:
            for bi in reversed(range(ne, ne + nd)):
                self.reducer.ready(*self.layer_ranges[bi])
        dx0 = self._stage_bwd(range(0, ne), w["dright"], N, None, dfe, sw)
        sw.join()
        self._cond_bwd(dx0)
