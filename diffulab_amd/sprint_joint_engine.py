"""Host-side runtime of SprintDiT in its joint text-image form (simple_dit=False; reference networks/denoisers/sprint.py:389-503,
the model of configs/train_imagenet_repa_txt_to_img_sprint.yaml):

    joint encoder blocks (N image + Lc text tokens) -> keep k of the N image tokens -> deep stage on [text ; kept image tokens]:
    joint blocks, then MMDiTSingleStreamBlocks (mmdit.py:442-532: attention and MLP in parallel on the modulated concatenation,
    one 3D-row modulation) -> restore the image canvas, fuse = Linear(2D -> D) on [restored ; encoder image output],
    fuse_context = Linear(2D -> D) on [deep context ; encoder context] -> joint decoder blocks -> last layer

Every joint stage is DiTEngine._jstage_fwd / _jstage_bwd (engine.py) over ONE flat arena: per-stream gated residuals are absorbed by
the next LayerNorm-modulate kernel inside a stage and materialised at stage boundaries; the single-stream stage keeps the
concatenated latents [B, Lc + k, D] resident across its blocks (the reference's split / re-concatenate between consecutive blocks
is the identity); RoPE rows of the kept tokens come from a position index, the key-padding mask from an additive key bias.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import Tensor

from . import ops
from .engine import ArenaLayout, DiTEngine, Modulation, SideWork, _other, _rup
from .mmdit_engine import STREAMS, JointDims, joint_rope_tables
from .sprint_engine import Route


@dataclass
class SprintJointDims(JointDims):
    encoder_depth: int = 2
    deep_layers_depth: int = 8
    n_single_stream_blocks: int = 0
    decoder_depth: int = 2
    drop_rate: float = 0.75

    def __post_init__(self) -> None:
        super().__post_init__()
        self.depth = self.encoder_depth + self.deep_layers_depth + self.decoder_depth

    def n_kept(self, S: int) -> int:
        return max(1, int(S * (1.0 - float(self.drop_rate))))

    def kinds(self) -> list[tuple[str, str]]:
        """(state_dict prefix, 'J' joint block | 'S' single-stream block) of every block in execution order"""
        nj = self.deep_layers_depth - self.n_single_stream_blocks
        return ([(f"layers.{i}.", "J") for i in range(self.encoder_depth)]
                + [(f"deep_layers.{i}.", "J" if i < nj else "S") for i in range(self.deep_layers_depth)]
                + [(f"decoder_layers.{i}.", "J") for i in range(self.decoder_depth)])


class SprintJointLayout(ArenaLayout):
    def _place(self, d: "SprintJointDims | JointStackDims", sprint: bool = True) -> None:
        D, E, p, add = d.inner_dim, d.embedding_dim, d.patch_size, self.add
        F = d.mlp_ratio * D
        kinds = d.kinds()
        self.prefixes = [pre for pre, _ in kinds]

        # stacked adaLN matrix: [input 6D | context 6D] per joint block, 3D per single-stream block, then the last layer's 2D
        self.add_stacked_adaln(kinds, D, E, last_layer=True)
        add("time_embed.0.weight", (E, d.frequency_embedding))
        add("time_embed.0.bias", (E,))
        add("time_embed.2.weight", (E, E))
        add("time_embed.2.bias", (E,))
        self.add_pooled_mlp(d.pooled_dim, E)
        add("conv_proj.weight", (D, d.input_channels, p, p))
        add("context_embed.weight", (D, d.context_dim))
        add("last_layer.linear.weight", (p * p * d.output_channels, D))
        add("last_layer.linear.bias", (p * p * d.output_channels,))
        if sprint:
            add("mask_token", (1, 1, D))
            add("fuse.weight", (D, 2 * D))
            add("fuse_context.weight", (D, 2 * D))
        self.block_first = []
        for pre, kind in kinds:
            if kind == "J":
                self.block_first.append(pre + "input_norm_1.weight")
                self.add_joint_block(pre, D, F)
            else:
                self.block_first.append(pre + "norm.weight")
                self.add_single_block(pre, D, F)


class SprintJointEngine(DiTEngine):
    context: tuple[Tensor, Tensor | None] | None = None
    route: Route | None = None

    def _make_layout(self, d: SprintJointDims) -> SprintJointLayout:  # type: ignore[override]
        self.kinds = d.kinds()
        return SprintJointLayout(d)

    def _extra_shadows(self, reg) -> None:
        D = self.d.inner_dim
        reg("context_embed.weight", D, self.d.context_dim, dgrad=False)
        reg("fuse.weight", D, 2 * D)
        reg("fuse_context.weight", D, 2 * D)

    def _block_shadows(self, reg, pre: str) -> None:
        d, dev = self.d, self.dev
        D, F = d.inner_dim, d.mlp_ratio * d.inner_dim
        kind = dict(self.kinds)[pre]
        names = ([(f"attention.qkv_{st}.weight", f"attention.{st}_proj_out.weight", f"mlp_{st}.0.weight", f"mlp_{st}.2.weight")
                  for st in STREAMS] if kind == "J" else [("attention.qkv.weight", "attention.proj_out.weight", "mlp.0.weight", "mlp.2.weight")])
        for qkv, proj, m0, m2 in names:
            reg(pre + qkv, 3 * D, D)
            reg(pre + proj, D, D)
            reg(pre + m0, 2 * F, D)
            self.sh[pre + m0 + "|g"] = torch.zeros(2 * F, D, device=dev, dtype=torch.bfloat16)
            reg(pre + m2, D, F)

    # ------------------------------------------------------------------ workspace
    def _alloc(self, B: int, H: int, W: int, train: bool, Lc: int = 0, k: int = 0) -> None:  # type: ignore[override]
        d, z, zr = self.d, self._z, self._zr
        key = (B, H, W, train, Lc, k)
        if self._cached(key):
            return
        D, p = d.inner_dim, d.patch_size
        gh, gw = H // p, W // p
        N = gh * gw
        Tf, Td = Lc + N, Lc + k
        Tpf, Tpd = _rup(Tf, 256), _rup(Td, 256)
        if Tpf > ops.ATTN_MAX_TOKENS or (B * N) % 64 or Lc < 1:
            raise NotImplementedError(f"joint SprintDiT HIP path: context + image tokens <= {ops.ATTN_MAX_TOKENS} (got {Lc} + {N}), batch * tokens of "
                                      f"each stream a multiple of 64 (kept {k})")
        M, F = B * N, d.mlp_ratio * D
        ops.check_row_extent(B * Tpf, max(2 * F, 6 * D), "joint SprintDiT HIP path")
        f32 = torch.float32
        Hh = d.num_heads
        w: dict[str, object] = {}
        self._cond_buffers(w, B, H, W, train, train and self._grouped_widths())
        w["ctxP"] = zr(B * Lc, _rup(d.context_dim, 64))
        w["x"] = [z(M, D)]
        w["c0"] = zr(B * Lc, D)
        w["kb_f"], w["kb_d"] = z(B, Tpf, dtype=f32), z(B, Tpd, dtype=f32)
        w["kb_f"][:, Tf:] = float("-inf")
        w["kb_d"][:, Td:] = float("-inf")
        ne, nd = d.encoder_depth, d.deep_layers_depth
        blk = []
        for bi, (_, kind) in enumerate(self.kinds):
            deep = ne <= bi < ne + nd
            nx, Tp = (k, Tpd) if deep else (N, Tpf)
            per = self._joint_attn_buffers(B, Tp)
            if kind == "J":
                for st, nt in (("input", nx), ("context", Lc)):
                    per[st] = self._joint_stream_buffers(B, nt, train)
            else:
                per.update(self._single_stream_buffers(B, Td, train))
            blk.append(per)
        w["blk"] = blk
        w["cat"], w["ccat"] = z(M, 2 * D), zr(B * Lc, 2 * D)   # [restored | encoder image], [deep context | encoder context]
        w["c_enc"] = zr(B * Lc, D)
        w["xd0"], w["xd_out"] = z(B * k, D), z(B * k, D)
        w["xj"], w["cj"] = z(B * k, D), zr(B * Lc, D)           # outputs of the deep joint sub-stage
        w["lat0"], w["lat_out"] = zr(B * Td, D), zr(B * Td, D)
        w["xfuse"], w["cfuse"], w["xdec"] = z(M, D), zr(B * Lc, D), z(M, D)
        if train:
            for name, mt in ((f"x{N}", M), (f"x{k}", B * k), ("c", B * Lc), ("l", B * Td)):
                w["s_" + name] = {"dxa": zr(mt, D), "dxb": zr(mt, D), "dxm": zr(mt, D), "dxm2": zr(mt, D), "da": zr(mt, D), "dh": zr(mt, F)}
            for tag, Tp in (("f", Tpf), ("d", Tpd)):
                w["dao_" + tag] = z(B * Tp, D)
                w["dq_" + tag], w["dk_" + tag], w["dv_" + tag] = (z(B, Hh, Tp, 64) for _ in range(3))
            w["dleft"], w["dright"], w["dcl"], w["dcr"] = z(M, D), z(M, D), zr(B * Lc, D), zr(B * Lc, D)
            w["dxd"], w["dlat"], w["dxj"], w["dcj"] = z(B * k, D), zr(B * Td, D), z(B * k, D), zr(B * Lc, D)
            w["dxdec"] = z(M, D)
        self._publish(w, key, (B, H, W, gh, gw, N, M, _rup(B, 64), p * p * d.output_channels), (Lc, gh, gw),
                      lambda: joint_rope_tables(Lc, gh, gw, d.rope_axes_dim, d.rope_base))

    def _jscratch(self, nx: int, tag: str) -> tuple[dict, tuple]:
        """scratch of _jstage_bwd over nx image tokens per sample: the chain scratch of each stream and the attention scratch of the
        full ("f") or the deep ("d") joint sequence"""
        w = self.ws
        return {"input": w[f"s_x{nx}"], "context": w["s_c"]}, (w["dao_" + tag], w["dq_" + tag], w["dk_" + tag], w["dv_" + tag])

    # ------------------------------------------------------------------ single-stream stage
    def _sstage_fwd(self, blocks, lat_in: Tensor, T: int, pos: Tensor, kb: Tensor, out: Tensor) -> None:
        """MMDiTSingleStreamBlocks on the concatenated latents lat_in [B*T, D] (context rows first); materialised output -> out"""
        d, w, sh = self.d, self.ws, self.sh
        B = self.geo[0]
        D, Hh = d.inner_dim, d.num_heads
        cos, sin = self._tabs
        rot = sum(d.rope_axes_dim)
        mod = w["mod"]
        Tp = kb.shape[1]
        pend = None
        for bi in blocks:
            a, pre, mo = w["blk"][bi], self.prefixes[bi], self.layout.mod_off[bi]
            nw, nb = self.P(pre + "norm.weight"), self.P(pre + "norm.bias")
            if pend is None:
                xcur = lat_in
                ops.ln_modulate_fwd(xcur, nw, nb, mod[:, mo : mo + D], mod[:, mo + D : mo + 2 * D], T, 1e-5, a["m"], a["mean"], a["rstd"])
            else:
                xcur = a["x0"]
                ops.ln_modulate_fwd(pend[0], nw, nb, mod[:, mo : mo + D], mod[:, mo + D : mo + 2 * D], T, 1e-5, a["m"], a["mean"],
                                    a["rstd"], t=pend[1], gate=pend[2], x_out=xcur)
            a["xin"] = xcur
            ops.gemm_nt(a["m"], sh[pre + "attention.qkv.weight|f"], a["qkv"])
            ops.qk_norm_rope_fwd(a["qkv"], self.P(pre + "attention.qk_norm.query_norm.scale"),
                                 self.P(pre + "attention.qk_norm.key_norm.scale"), cos, sin, a["q"], a["k"], a["v"], a["rrms"], B, T, Hh,
                                 64, rot, pos=pos, n_off=0)
            ops.attn_fwd_ex(a["q"], a["k"], a["v"], a["ao"], a["lse"], B, Hh, Tp, Tp, 64, 64**-0.5, kb)
            ops.copy_rows3d(a["ao"], Tp * D, D, a["a"], T * D, D, B, T, D)
            ops.gemm_nt(a["a"], sh[pre + "attention.proj_out.weight|f"], a["ta"])
            if not ops.gemm_nt_swiglu(a["m"], sh[pre + "mlp.0.weight|g"], a["u"] if self._train else None, a["h"]):
                ops.gemm_nt(a["m"], sh[pre + "mlp.0.weight|f"], a["u"])
                ops.swiglu_fwd(a["u"], a["h"])
            ops.gemm_nt(a["h"], sh[pre + "mlp.2.weight|f"], a["t"], resid=a["ta"])  # attention + MLP (mmdit.py:524-527)
            pend = (xcur, a["t"], mod[:, mo + 2 * D : mo + 3 * D])
        ops.gated_residual_fwd(pend[0], pend[1], pend[2], T, out)

    def _sstage_bwd(self, blocks, dlat: Tensor, T: int, pos: Tensor, kb: Tensor, sw: SideWork, attn: tuple | None = None) -> Tensor:
        """backward of _sstage_fwd; attn: the attention scratch (dao, dq, dk, dv) over kb.shape[1] rows, default the deep stage's"""
        d, w, sh = self.d, self.ws, self.sh
        B = self.geo[0]
        D, Hh = d.inner_dim, d.num_heads
        cos, sin = self._tabs
        rot = sum(d.rope_axes_dim)
        mod, dmod = w["mod"], w["dmod32"]
        Tp = kb.shape[1]
        s = w["s_l"]
        dao, dq, dk, dv = attn if attn is not None else (w["dao_d"], w["dq_d"], w["dk_d"], w["dv_d"])
        blocks = list(blocks)
        last = blocks[-1]
        ml = self.layout.mod_off[last]
        ops.gate_bwd(dlat, w["blk"][last]["t"], mod[:, ml + 2 * D : ml + 3 * D], T, w["blk"][last]["wg"]["dt"],
                     dmod[:, ml + 2 * D : ml + 3 * D])
        dx = dlat
        for j in reversed(range(len(blocks))):
            bi = blocks[j]
            a, pre, mo = w["blk"][bi], self.prefixes[bi], self.layout.mod_off[bi]
            g = a["wg"]
            sw.wgrad(g["dt"], a["h"], pre + "mlp.2.weight")
            sw.wgrad(g["dt"], a["a"], pre + "attention.proj_out.weight")
            ops.mlp_swiglu_bwd(g["dt"], sh[pre + "mlp.2.weight|t"], a["m"], sh[pre + "mlp.0.weight|g"], a["u"], s["dh"], g["du"])
            sw.wgrad(g["du"], a["m"], pre + "mlp.0.weight")
            ops.gemm_nt(g["du"], sh[pre + "mlp.0.weight|t"], s["dxm"])
            ops.gemm_nt(g["dt"], sh[pre + "attention.proj_out.weight|t"], s["da"])
            dao.zero_()
            ops.copy_rows3d(s["da"], T * D, D, dao, Tp * D, D, B, T, D)
            ops.attn_bwd_ex(a["q"], a["k"], a["v"], a["ao"], dao, a["lse"], dq, dk, dv, B, Hh, Tp, Tp, 64, 64**-0.5, kb)
            ops.qk_norm_rope_bwd(dq, dk, dv, a["qkv"], self.P(pre + "attention.qk_norm.query_norm.scale"),
                                 self.P(pre + "attention.qk_norm.key_norm.scale"), cos, sin, a["rrms"], g["dqkv"],
                                 self.G(pre + "attention.qk_norm.query_norm.scale"), B, T, Hh, 64, rot, pos=pos, n_off=0)
            sw.wgrad(g["dqkv"], a["m"], pre + "attention.qkv.weight")
            ops.gemm_nt(g["dqkv"], sh[pre + "attention.qkv.weight|t"], s["dxm2"], resid=s["dxm"])
            nxt = {}
            if j > 0:
                bp = blocks[j - 1]
                mp = self.layout.mod_off[bp]
                nxt = dict(gate_t=w["blk"][bp]["t"], gate=mod[:, mp + 2 * D : mp + 3 * D], dt=w["blk"][bp]["wg"]["dt"],
                           dgate=dmod[:, mp + 2 * D : mp + 3 * D])
            nx_ = _other(s, dx)
            ops.ln_modulate_bwd(s["dxm2"], a["xin"], self.P(pre + "norm.weight"), self.P(pre + "norm.bias"), mod[:, mo : mo + D], T,
                                a["mean"], a["rstd"], dx, nx_, dmod[:, mo : mo + D], dmod[:, mo + D : mo + 2 * D], a["dwb"][0], **nxt)
            sw.fold(a["dwb"][0], pre + "norm.weight", B)
            dx = nx_
            self._end_block(sw, bi)
        return dx

    # ------------------------------------------------------------------ forward
    def forward(self, x: Tensor, t: Tensor, y_eff: Tensor | None = None, train: bool = True, refresh: bool = True) -> Tensor:
        d = self.d
        B, C, H, W = x.shape
        assert C == d.input_channels and x.dtype == torch.float32 and x.is_cuda and self.context is not None and self.route is not None
        ctx, keep = self.context
        route = self.route
        Lc, k = ctx.shape[1], route.k
        self._alloc(B, H, W, train, Lc, k)
        if refresh:
            self.refresh_shadows(force=train)
        w, sh = self.ws, self.sh
        _, _, _, gh, gw, N, M, Bp, Fo = self.geo
        D, L, Cd = d.inner_dim, d.depth, d.context_dim
        ne, nd, ns = d.encoder_depth, d.deep_layers_depth, d.n_single_stream_blocks
        nj = nd - ns
        Td = Lc + k
        self._train, self._yeff, self._Lc, self._route = train, None, Lc, route
        self._tabs = self._rope[(Lc, gh, gw)]
        mod = self._stem_fwd(x, t, None)
        w["ctxP"][:, :Cd].copy_(ctx.reshape(B * Lc, Cd))
        ops.gemm_nt(w["ctxP"], sh["context_embed.weight|f"], w["c0"], M=B * Lc, N=D, K=w["ctxP"].shape[1])
        for kb in (w["kb_f"], w["kb_d"]):
            if keep is None:
                kb[:, :Lc].zero_()
            else:
                kb[:, :Lc].zero_().masked_fill_(~keep.to(device=kb.device, dtype=torch.bool), float("-inf"))
        cat, ccat = w["cat"], w["ccat"]
        # encoder: image output -> right half of cat, context output -> c_enc (and the right half of ccat)
        self._jstage_fwd(range(0, ne), w["x"][0], w["c0"], N, None, w["kb_f"], cat[:, D:], w["c_enc"])
        ops.copy_rows3d(w["c_enc"], 0, D, ccat[:, D:], 0, 2 * D, 1, B * Lc, D)
        mask = self.P("mask_token").view(D)
        if route.skip_deep:
            ops.restore_tokens(w["xd_out"], route.inv, mask, cat[:, :D], B, N, k, D)
            ops.copy_rows3d(w["c_enc"], 0, D, ccat, 0, 2 * D, 1, B * Lc, D)  # the deep layers did not touch the context
        else:
            ops.gather_tokens(cat[:, D:], route.idx, w["xd0"], B, N, k, D)
            pos_img = route.idx.view(-1)
            xs, cs = w["xd0"], w["c_enc"]
            if nj:
                if ns:
                    self._jstage_fwd(range(ne, ne + nj), xs, cs, k, pos_img, w["kb_d"], w["xj"], w["cj"])
                    xs, cs = w["xj"], w["cj"]
                else:
                    self._jstage_fwd(range(ne, ne + nj), xs, cs, k, pos_img, w["kb_d"], w["xd_out"], ccat[:, :D])
            if ns:
                lat0 = w["lat0"]
                ops.copy_rows3d(cs, Lc * D, D, lat0, Td * D, D, B, Lc, D)
                ops.copy_rows3d(xs, k * D, D, lat0[Lc:], Td * D, D, B, k, D)
                self._sstage_fwd(range(ne + nj, ne + nd), lat0, Td, route.pos_lat, w["kb_d"], w["lat_out"])
                ops.copy_rows3d(w["lat_out"][Lc:], Td * D, D, w["xd_out"], k * D, D, B, k, D)
                ops.copy_rows3d(w["lat_out"], Td * D, D, ccat, Lc * 2 * D, 2 * D, B, Lc, D)
            ops.restore_tokens(w["xd_out"], route.inv, mask, cat[:, :D], B, N, k, D)
        ops.gemm_nt(cat, sh["fuse.weight|f"], w["xfuse"], M=M, N=D, K=2 * D)
        ops.gemm_nt(ccat, sh["fuse_context.weight|f"], w["cfuse"], M=B * Lc, N=D, K=2 * D)
        self._jstage_fwd(range(ne + nd, L), w["xfuse"], w["cfuse"], N, None, w["kb_f"], w["xdec"], None)
        return self._head_fwd(Modulation(mod, None, self.layout.mod_rows - 2 * D, D, N), w["xdec"])

    def feature(self, kblk: int) -> Tensor:
        """image-stream output of encoder block k (``layers[k]``) of the last train-mode forward"""
        assert self._train and 0 <= kblk < self.d.encoder_depth
        B, N, D = self.geo[0], self.geo[5], self.d.inner_dim
        if kblk + 1 < self.d.encoder_depth:
            return self.ws["blk"][kblk + 1]["input"]["x0"].view(B, N, D)
        return self.ws["cat"].view(B, N, 2 * D)[:, :, D:]

    # ------------------------------------------------------------------ backward
    def backward(self, dpred: Tensor, dfeats: dict[int, Tensor] | None = None) -> None:
        assert self._train and self.grads is not None
        d, w, sh = self.d, self.ws, self.sh
        B, H, W, gh, gw, N, M, Bp, Fo = self.geo
        D, L, Cd = d.inner_dim, d.depth, d.context_dim
        ne, nd, ns = d.encoder_depth, d.deep_layers_depth, d.n_single_stream_blocks
        nj = nd - ns
        route, Lc = self._route, self._Lc
        k = route.k
        Td = Lc + k
        dfe = self._dfeat_rows(dfeats)
        mod, dmod = w["mod"], w["dmod32"]
        dmod[:B].zero_()
        sN = w[f"s_x{N}"]

        self._head_bwd(dpred, sN["dxm"])
        Modulation(mod, dmod, self.layout.mod_rows - 2 * D, D, N).ln_bwd(sN["dxm"], w["xdec"], None, None, 0, w["meanf"], w["rstdf"], None,
                                                                         w["dxdec"], None)
        sw = SideWork(self)
        dxf, dcf = self._jstage_bwd(range(ne + nd, L), w["dxdec"], None, N, None, w["kb_f"], *self._jscratch(N, "f"), {}, sw)
        # fuse / fuse_context (main stream: dxf / dcf are chain scratch that the next stages reuse)
        ops.gemm_tn(dxf, w["cat"], self.G("fuse.weight"))
        ops.gemm_tn(dcf, w["ccat"], self.G("fuse_context.weight"))
        wt, wc = sh["fuse.weight|t"], sh["fuse_context.weight|t"]
        ops.gemm_nt(dxf, wt[:D], w["dleft"], M=M, N=D, K=D)
        ops.gemm_nt(dxf, wt[D:], w["dright"], M=M, N=D, K=D)
        ops.gemm_nt(dcf, wc[:D], w["dcl"], M=B * Lc, N=D, K=D)
        ops.gemm_nt(dcf, wc[D:], w["dcr"], M=B * Lc, N=D, K=D)
        ops.masked_colsum(w["dleft"], route.inv.view(-1), self.G("mask_token").view(D), M, D)
        if route.skip_deep:
            ops.add_bf16(w["dcr"], w["dcl"], w["dcr"])
            if self.reducer is not None:
                for bi in reversed(range(ne, ne + nd)):
                    self.reducer.ready(*self.layer_ranges[bi])
        else:
            pos_img = route.idx.view(-1)
            ops.gather_tokens(w["dleft"], route.idx, w["dxd"], B, N, k, D, keep=route.keep)
            gx, gc = w["dxd"], w["dcl"]
            if ns:
                dlat = w["dlat"]
                ops.copy_rows3d(gc, Lc * D, D, dlat, Td * D, D, B, Lc, D)
                ops.copy_rows3d(gx, k * D, D, dlat[Lc:], Td * D, D, B, k, D)
                dl = self._sstage_bwd(range(ne + nj, ne + nd), dlat, Td, route.pos_lat, w["kb_d"], sw)
                ops.copy_rows3d(dl[Lc:], Td * D, D, w["dxj"], k * D, D, B, k, D)
                ops.copy_rows3d(dl, Td * D, D, w["dcj"], Lc * D, D, B, Lc, D)
                gx, gc = w["dxj"], w["dcj"]
            if nj:
                gx, gc = self._jstage_bwd(range(ne, ne + nj), gx, gc, k, pos_img, w["kb_d"], *self._jscratch(k, "d"), {}, sw)
            ops.scatter_tokens_add(gx, route.idx, w["dright"], B, N, k, D)
            ops.add_bf16(w["dcr"], gc, w["dcr"])
        dx0, dc0 = self._jstage_bwd(range(0, ne), w["dright"], w["dcr"], N, None, w["kb_f"], *self._jscratch(N, "f"), dfe, sw)
        sw.join()
        ops.gemm_tn(dc0, w["ctxP"], self.G("context_embed.weight"), M=D, N=Cd)
        self._cond_bwd(dx0)


# ================================================================================================ plain MMDiT with single-stream blocks
@dataclass
class JointStackDims(JointDims):
    n_single_stream_blocks: int = 0

    def kinds(self) -> list[tuple[str, str]]:
        nj = self.depth - self.n_single_stream_blocks
        return [(f"layers.{i}.", "J" if i < nj else "S") for i in range(self.depth)]


class JointStackEngine(SprintJointEngine):
    """MMDiT(simple_dit=False, n_single_stream_blocks > 0) (mmdit.py:699-731, 789-851): joint blocks, then single-stream blocks on
    the concatenated [context ; image] latents; the image rows of the result feed the last layer.  Reuses the joint and
    single-stream stages of SprintJointEngine without the token routing."""

    route = None

    def _make_layout(self, d: JointStackDims) -> SprintJointLayout:  # type: ignore[override]
        self.kinds = d.kinds()
        return SprintJointLayout(d, sprint=False)

    def _extra_shadows(self, reg) -> None:
        reg("context_embed.weight", self.d.inner_dim, self.d.context_dim, dgrad=False)

    def _alloc(self, B: int, H: int, W: int, train: bool, Lc: int = 0, k: int = 0) -> None:  # type: ignore[override]
        d, z, zr = self.d, self._z, self._zr
        key = (B, H, W, train, Lc)
        if self._cached(key):
            return
        D, p = d.inner_dim, d.patch_size
        gh, gw = H // p, W // p
        N = gh * gw
        T = Lc + N
        Tp = _rup(T, 256)
        if Tp > ops.ATTN_MAX_TOKENS or (B * N) % 64 or Lc < 1:
            raise NotImplementedError(f"joint MMDiT HIP path: context + image tokens <= {ops.ATTN_MAX_TOKENS} (got {Lc} + {N}), image tokens a "
                                      "multiple of 64")
        M, F = B * N, d.mlp_ratio * D
        ops.check_row_extent(B * Tp, max(2 * F, 6 * D), "joint MMDiT HIP path")
        f32 = torch.float32
        Hh = d.num_heads
        w: dict[str, object] = {}
        self._cond_buffers(w, B, H, W, train, train and self._grouped_widths())
        w["ctxP"] = zr(B * Lc, _rup(d.context_dim, 64))
        w["x"] = [z(M, D)]
        w["c0"] = zr(B * Lc, D)
        w["kb_f"] = z(B, Tp, dtype=f32)
        w["kb_f"][:, T:] = float("-inf")
        blk = []
        for _, kind in self.kinds:
            per = self._joint_attn_buffers(B, Tp)
            if kind == "J":
                for st, nt in (("input", N), ("context", Lc)):
                    per[st] = self._joint_stream_buffers(B, nt, train)
            else:
                per.update(self._single_stream_buffers(B, T, train))
            blk.append(per)
        w["blk"] = blk
        w["xj"], w["cj"] = z(M, D), zr(B * Lc, D)
        w["lat0"], w["lat_out"] = zr(B * T, D), zr(B * T, D)
        w["xl"] = z(M, D)
        if train:
            for name, mt in ((f"x{N}", M), ("c", B * Lc), ("l", B * T)):
                w["s_" + name] = {"dxa": zr(mt, D), "dxb": zr(mt, D), "dxm": zr(mt, D), "dxm2": zr(mt, D), "da": zr(mt, D),
                                  "dh": zr(mt, F)}
            w["dao_f"] = z(B * Tp, D)
            w["dq_f"], w["dk_f"], w["dv_f"] = (z(B, Hh, Tp, 64) for _ in range(3))
            for n_ in ("dao", "dq", "dk", "dv"):  # (the single-stream stage addresses its attention scratch as "_d")
                w[n_ + "_d"] = w[n_ + "_f"]
            w["dxl"], w["dlat"], w["dxj"], w["dcj"] = z(M, D), zr(B * T, D), z(M, D), zr(B * Lc, D)
        self._publish(w, key, (B, H, W, gh, gw, N, M, _rup(B, 64), p * p * d.output_channels), (Lc, gh, gw),
                      lambda: joint_rope_tables(Lc, gh, gw, d.rope_axes_dim, d.rope_base))

    def forward(self, x: Tensor, t: Tensor, y_eff: Tensor | None = None, train: bool = True, refresh: bool = True) -> Tensor:
        d = self.d
        B, C, H, W = x.shape
        assert C == d.input_channels and x.dtype == torch.float32 and x.is_cuda and self.context is not None
        ctx, keep = self.context
        Lc = ctx.shape[1]
        self._alloc(B, H, W, train, Lc)
        if refresh:
            self.refresh_shadows(force=train)
        w, sh = self.ws, self.sh
        _, _, _, gh, gw, N, M, Bp, Fo = self.geo
        D, L, Cd = d.inner_dim, d.depth, d.context_dim
        nj = L - d.n_single_stream_blocks
        T = Lc + N
        self._train, self._yeff, self._Lc = train, None, Lc
        self._tabs = self._rope[(Lc, gh, gw)]
        mod = self._stem_fwd(x, t, None)
        w["ctxP"][:, :Cd].copy_(ctx.reshape(B * Lc, Cd))
        ops.gemm_nt(w["ctxP"], sh["context_embed.weight|f"], w["c0"], M=B * Lc, N=D, K=w["ctxP"].shape[1])
        kb = w["kb_f"]
        if keep is None:
            kb[:, :Lc].zero_()
        else:
            kb[:, :Lc].zero_().masked_fill_(~keep.to(device=kb.device, dtype=torch.bool), float("-inf"))
        xs, cs = w["x"][0], w["c0"]
        if nj:
            self._jstage_fwd(range(0, nj), xs, cs, N, None, kb, w["xj"], w["cj"])
            xs, cs = w["xj"], w["cj"]
        lat0 = w["lat0"]
        ops.copy_rows3d(cs, Lc * D, D, lat0, T * D, D, B, Lc, D)
        ops.copy_rows3d(xs, N * D, D, lat0[Lc:], T * D, D, B, N, D)
        self._sstage_fwd(range(nj, L), lat0, T, None, kb, w["lat_out"])
        ops.copy_rows3d(w["lat_out"][Lc:], T * D, D, w["xl"], N * D, D, B, N, D)
        return self._head_fwd(Modulation(mod, None, self.layout.mod_rows - 2 * D, D, N), w["xl"])

    def feature(self, kblk: int) -> Tensor:
        nj = self.d.depth - self.d.n_single_stream_blocks
        assert self._train
        B, N, D = self.geo[0], self.geo[5], self.d.inner_dim
        if kblk + 1 < nj:
            return self.ws["blk"][kblk + 1]["input"]["x0"].view(B, N, D)
        if kblk + 1 == nj:
            return self.ws["xj"].view(B, N, D)
        raise NotImplementedError("forward hooks on single-stream blocks (the image rows live inside the concatenated latents)")

    def backward(self, dpred: Tensor, dfeats: dict[int, Tensor] | None = None) -> None:
        assert self._train and self.grads is not None
        d, w, sh = self.d, self.ws, self.sh
        B, H, W, gh, gw, N, M, Bp, Fo = self.geo
        D, L, Cd, Lc = d.inner_dim, d.depth, d.context_dim, self._Lc
        nj = L - d.n_single_stream_blocks
        T = Lc + N
        dfe = self._dfeat_rows(dfeats)
        mod, dmod = w["mod"], w["dmod32"]
        dmod[:B].zero_()
        sN = w[f"s_x{N}"]
        self._head_bwd(dpred, sN["dxm"])
        Modulation(mod, dmod, self.layout.mod_rows - 2 * D, D, N).ln_bwd(sN["dxm"], w["xl"], None, None, 0, w["meanf"], w["rstdf"], None,
                                                                         w["dxl"], None)
        sw = SideWork(self)
        dlat = w["dlat"]
        dlat.zero_()  # the context rows of the last block's output feed nothing
        ops.copy_rows3d(w["dxl"], N * D, D, dlat[Lc:], T * D, D, B, N, D)
        dl = self._sstage_bwd(range(nj, L), dlat, T, None, w["kb_f"], sw)
        ops.copy_rows3d(dl[Lc:], T * D, D, w["dxj"], N * D, D, B, N, D)
        ops.copy_rows3d(dl, T * D, D, w["dcj"], Lc * D, D, B, Lc, D)
        gx, gc = w["dxj"], w["dcj"]
        if nj:
            gx, gc = self._jstage_bwd(range(0, nj), gx, gc, N, None, w["kb_f"], *self._jscratch(N, "f"), dfe, sw)
        sw.join()
        ops.gemm_tn(gc, w["ctxP"], self.G("context_embed.weight"), M=D, N=Cd)
        self._cond_bwd(gx)
