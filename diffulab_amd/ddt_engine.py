"""Host-side runtime of DDT with simple_ddt=True (reference networks/denoisers/ddt.py:346-464; configs/model/ddt.yaml).

Encoder = a stage of DiT blocks with per-sample adaLN conditioning (SprintEngine._stage_fwd over DiTEngine._dit_block_fwd).  Decoder = DiT blocks on a second
patch embedding of the input whose conditioning is PER TOKEN, z = silu(encoder_output + time_embedding): the adaLN linears of all
decoder blocks and of the last layer are stacked into ONE GEMM over the tokens ([B*N, D] x [D, 6D*depth + 2D]); the
LayerNorm-modulate kernels read one modulation row per token (rows_per_mod = 1) and the backward writes the per-token modulation
gradients as bf16 rows straight into the gradient matrix of that GEMM (dl_ln_modulate_bwd_tok).  The decoder blocks are the same
DiTEngine._dit_block_fwd / _bwd with a per-token engine.Modulation.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import Tensor

from . import ops, tuning
from .engine import ArenaLayout, DiTDims, Modulation, SideWork, _rup, rope_grid_tables
from .sprint_engine import SprintEngine

N_PART = 32  # partial slabs of the affine LayerNorm gradients of a per-token LayerNorm backward


@dataclass
class DDTDims(DiTDims):
    encoder_depth: int = 8
    decoder_depth: int = 4

    def __post_init__(self) -> None:
        self.embedding_dim = self.inner_dim  # ddt.py:139-176
        super().__post_init__()
        self.depth = self.encoder_depth + self.decoder_depth


class DDTLayout(ArenaLayout):
    def _place(self, d: DDTDims) -> None:
        D, p, add = d.inner_dim, d.patch_size, self.add
        E = D
        enc = [f"layers.{i}." for i in range(d.encoder_depth)]
        dec = [f"decoder_layers.{i}." for i in range(d.decoder_depth)]
        self.prefixes = enc + dec
        for suffix, shp in (("weight", lambda r: (r, E)), ("bias", lambda r: (r,))):
            for i, pre in enumerate(enc):  # per-sample adaLN of the encoder blocks: one [ne*6D, E] matrix
                add(pre + "modulation.lin." + suffix, shp(6 * D), align=1 if i else 64)
        for suffix, shp in (("weight", lambda r: (r, E)), ("bias", lambda r: (r,))):
            for i, pre in enumerate(dec):  # per-token adaLN of the decoder blocks + last layer: one [nd*6D + 2D, D] matrix
                add(pre + "modulation.lin." + suffix, shp(6 * D), align=1 if i else 64)
            add("last_layer.adaLN_modulation.1." + suffix, shp(2 * D), align=1)
        self.mod_rows, self.tmod_rows = d.encoder_depth * 6 * D, d.decoder_depth * 6 * D + 2 * D
        self.mod_w0, self.mod_b0 = enc[0] + "modulation.lin.weight", enc[0] + "modulation.lin.bias"
        self.tmod_w0, self.tmod_b0 = dec[0] + "modulation.lin.weight", dec[0] + "modulation.lin.bias"
        if d.n_classes is not None:
            add("label_embed.embedding.weight", (d.n_classes + (1 if d.classifier_free else 0), E))
        add("time_embed.0.weight", (E, d.frequency_embedding))
        add("time_embed.0.bias", (E,))
        add("time_embed.2.weight", (E, E))
        add("time_embed.2.bias", (E,))
        add("conv_proj_encoder.weight", (D, d.input_channels, p, p))
        add("conv_proj_decoder.weight", (D, d.input_channels, p, p))
        add("last_layer.linear.weight", (p * p * d.output_channels, D))
        add("last_layer.linear.bias", (p * p * d.output_channels,))
        self.block_first = [pre + "norm_1.weight" for pre in self.prefixes]
        for pre in self.prefixes:
            self.add_dit_block(pre, D, d.mlp_ratio * D)


class PerTokenDecoder:
    """DDT decoder shared by the class-conditional and the joint-encoder engines: DiT blocks `first .. first + nd` of the block
    list on ws["xdec_in"], conditioned per token on silu(ws["enc_out"] + time embedding) through ONE stacked adaLN GEMM
    (ws["tmod"]), then the modulated last layer.  Expects ws keys xdec_in, enc_out, sz, tmod, xl, xf, meanf, rstdf, otok, pred, e and
    DiT-style per-block dicts ws["blk"][bi] (with "wg" and "dwbp" in training), layout.tmod_rows / tmod_w0 / tmod_b0."""

    def _decoder_fwd(self, first: int, nd: int, cos: Tensor, sin: Tensor) -> Tensor:
        w, sh, D = self.ws, self.sh, self.d.inner_dim
        B, _, _, _, _, N, M, _, _ = self.geo
        # per-token conditioning of the decoder and the stacked adaLN GEMM of its blocks + last layer
        ops.ddt_cond_fwd(w["enc_out"], w["e"], B, N, w["sz"])
        R = self.layout.tmod_rows
        tb = self.params[self.layout.entries[self.layout.tmod_b0][0] :][:R]
        tm = w["tmod"]
        ops.gemm_nt(w["sz"], sh["@tmod|f"], tm, bias=tb, M=M, N=R, K=D)
        pend = None
        for j in range(nd):
            a = w["blk"][first + j]
            a["xin"] = w["xdec_in"] if pend is None else a["x0"]
            pend = self._dit_block_fwd(a, self.prefixes[first + j], a["xin"], pend, Modulation(tm, None, j * 6 * D, D, 1, tok=True), N,
                                       cos, sin, kb=w.get("kb_d"))
        return self._head_fwd(Modulation(tm, None, nd * 6 * D, D, 1, tok=True), w["xl"], pend)

    def _decoder_bwd(self, dpred: Tensor, first: int, nd: int, cos: Tensor, sin: Tensor, s: dict, sw: SideWork) -> Tensor:
        """backward of _decoder_fwd.  s: chain scratch for N tokens (dxa, dxb, dxm, da, dh, dq, dk, dv); returns the gradient of
        ws["enc_out"] (ws["denc"]); ws["dtemb"] receives the decoder's gradient of the time embedding"""
        w, sh, D = self.ws, self.sh, self.d.inner_dim
        B, _, _, _, _, N, M, _, _ = self.geo
        tm, dtm = w["tmod"], w["dtmod"]
        self._head_bwd(dpred, s["dxm"])
        al = w["blk"][first + nd - 1]
        dx = s["dxa"]
        Modulation(tm, dtm, nd * 6 * D, D, 1, tok=True).ln_bwd(s["dxm"], w["xl"], None, None, 0, w["meanf"], w["rstdf"], None, dx, None,
                                                               gate=(al["t2"], (nd - 1) * 6 * D + 5 * D, al["wg"]["dt2"]))
        for j in reversed(range(nd)):
            bi = first + j
            a = w["blk"][bi]
            prev = (w["blk"][bi - 1]["t2"], (j - 1) * 6 * D + 5 * D, w["blk"][bi - 1]["wg"]["dt2"]) if j > 0 else None
            m = Modulation(tm, dtm, j * 6 * D, D, 1, tok=True, part=a["dwbp"], groups=N_PART)
            dx = self._dit_block_bwd(a, a["wg"], self.prefixes[bi], a["xin"], dx, prev, None, s, m, N, cos, sin, sw, kb=w.get("kb_d"),
                                     dao=w.get("dao_d"))
            self._end_block(sw, bi)
        self._patch_wgrad(dx, "conv_proj_decoder.weight", None)  # decoder patch embedding (the atomic form: no scratch)
        # stacked per-token adaLN GEMM: weight / bias gradients and the gradient of its input silu(z)
        R = self.layout.tmod_rows
        gw_ = self.grads[self.layout.entries[self.layout.tmod_w0][0] :][: R * D].view(R, D)
        gb_ = self.grads[self.layout.entries[self.layout.tmod_b0][0] :][:R]
        # (825 GFLOP at B = 256: through the atomics-free tiled form where its tile divides -- 2.05 -> 1.0 ms -- else the atomic kernel)
        if w.get("tmod_slab") is None or not ops.gemm_tn_group([(dtm, w["sz"], gw_)], w["tmod_slab"]):
            ops.gemm_tn(dtm, w["sz"], gw_)
        ops.colsum(dtm, gb_, M, R)
        ops.gemm_nt(dtm, sh["@tmod|t"], w["dsz"], M=M, N=D, K=R)
        w["dtemb"].zero_()
        ops.ddt_cond_bwd(w["dsz"], w["enc_out"], w["e"], B, N, w["denc"], w["dtemb"])

        return w["denc"]


class DDTEngine(SprintEngine, PerTokenDecoder):
    _conv_name = "conv_proj_encoder.weight"

    def _make_layout(self, d: DDTDims) -> DDTLayout:  # type: ignore[override]
        return DDTLayout(d)

    def _extra_shadows(self, reg) -> None:
        d = self.d
        reg("conv_proj_decoder.weight", d.inner_dim, d.input_channels * d.patch_size**2, dgrad=False)
        reg("@tmod", self.layout.tmod_rows, d.inner_dim)

    def _src(self, name: str, shape: tuple[int, int]) -> Tensor:
        if name == "@tmod":
            off = self.layout.entries[self.layout.tmod_w0][0]
            return self.params[off : off + shape[0] * shape[1]].view(shape)
        return super()._src(name, shape)

    # ------------------------------------------------------------------ workspace
    def _alloc(self, B: int, H: int, W: int, train: bool, k: int | None = None) -> None:  # type: ignore[override]
        d, z = self.d, self._z
        key = (B, H, W, train)
        if self._cached(key):
            return
        D, E, p, L = d.inner_dim, d.embedding_dim, d.patch_size, d.depth
        gh, gw = H // p, W // p
        N = gh * gw
        if N % 64 or (N > 256 and (N % 256 or N > ops.ATTN_MAX_TOKENS)):
            raise NotImplementedError(f"DDT HIP path: token grid {gh}x{gw} must give a multiple of 64 tokens up to 256, or of 256 up "
                                      f"to {ops.ATTN_MAX_TOKENS}")
        M, Bp, F = B * N, _rup(B, 64), d.mlp_ratio * D
        ops.check_row_extent(M, max(2 * F, 6 * D, self.layout.tmod_rows), "DDT HIP path")
        f32 = torch.float32
        R = self.layout.tmod_rows
        w: dict[str, object] = {}
        self._cond_buffers(w, B, H, W, train, train and self._grouped_widths())
        blk = []
        for _ in range(L):
            a = self._dit_block_buffers(B, N, train)
            if train:
                a["dwb"] = z(2, B, 2, D, dtype=f32)        # encoder blocks: per-sample partials
                a["dwbp"] = z(2, N_PART, 2, D, dtype=f32)  # decoder blocks: slab partials of the per-token LayerNorm backward
            blk.append(a)
        w["blk"] = blk
        w["x"] = [z(M, D)]
        w["xdec_in"], w["enc_out"], w["sz"] = z(M, D), z(M, D), z(M, D)
        w["tmod"] = z(M, R)
        w["xl"] = z(M, D)
        if train:
            w[f"s{N}"] = self._dit_chain_buffers(B, N)
            w["dtmod"] = z(M, R)
            if ops.wgrad_tile_ok(R, D) and M % 32 == 0 and M >= 2048:  # two token ranges of the stacked per-token adaLN weight gradient
                w["tmod_slab"] = torch.empty(2 * R * D, device=self.dev, dtype=torch.float32)
            w["dsz"], w["denc"] = z(M, D), z(M, D)
            w["dtemb"] = z(Bp, E, dtype=f32)
            if D <= 512 and tuning.on("DL_QK_INPLACE"):  # scale-gradient partials of the in-place QK-norm backward (ops.qk_inplace_ok)
                w["qk_part"] = torch.empty(1024 * 2 * D, device=self.dev, dtype=f32)
        self._publish(w, key, (B, H, W, gh, gw, N, M, Bp, p * p * d.output_channels), (gh, gw),
                      lambda: rope_grid_tables(gh, gw, d.rope_axes_dim, d.rope_base))

    # ------------------------------------------------------------------ forward
    def forward(self, x: Tensor, t: Tensor, y_eff: Tensor | None, train: bool = True, refresh: bool = True) -> Tensor:  # type: ignore[override]
        d = self.d
        B, C, H, W = x.shape
        assert C == d.input_channels and x.dtype == torch.float32 and x.is_cuda
        self._alloc(B, H, W, train)
        if refresh:
            self.refresh_shadows(force=train)
        w, sh = self.ws, self.sh
        _, _, _, gh, gw, N, M, Bp, Fo = self.geo
        D, L = d.inner_dim, d.depth
        ne = d.encoder_depth
        cos, sin = self._rope[(gh, gw)]
        self._train, self._yeff = train, y_eff
        self._stem_fwd(x, t, y_eff)
        ops.gemm_nt(w["tokP"], sh["conv_proj_decoder.weight|f"], w["xdec_in"], M=M, N=D, K=self._ki)
        self._stage_fwd(range(0, ne), w["x"][0], N, None, w["enc_out"])
        return self._decoder_fwd(ne, L - ne, cos, sin)

    def feature(self, kblk: int) -> Tensor:
        """output of encoder block k (``layers[k]``) of the last train-mode forward"""
        assert self._train and 0 <= kblk < self.d.encoder_depth
        B, N, D = self.geo[0], self.geo[5], self.d.inner_dim
        if kblk + 1 < self.d.encoder_depth:
            return self.ws["blk"][kblk + 1]["x0"].view(B, N, D)
        return self.ws["enc_out"].view(B, N, D)

    # ------------------------------------------------------------------ backward
    def backward(self, dpred: Tensor, dfeats: dict[int, Tensor] | None = None) -> None:
        assert self._train and self.grads is not None
        d, w = self.d, self.ws
        B, _, _, gh, gw, N, _, _, _ = self.geo
        L, ne = d.depth, d.encoder_depth
        dfe = self._dfeat_rows(dfeats)
        cos, sin = self._rope[(gh, gw)]
        w["dmod32"][:B].zero_()
        sw = SideWork(self)
        denc = self._decoder_bwd(dpred, ne, L - ne, cos, sin, w[f"s{N}"], sw)
        dx0 = self._stage_bwd(range(0, ne), denc, N, None, dfe, sw)
        sw.join()
        self._cond_bwd(dx0, extra_demb=w["dtemb"])


# ================================================================================================ joint-encoder form
from .mmdit_engine import STREAMS, JointDims, joint_rope_tables  # noqa: E402
from .sprint_joint_engine import SprintJointEngine  # noqa: E402


@dataclass
class DDTJointDims(JointDims):
    encoder_depth: int = 8
    decoder_depth: int = 4
    n_single_stream_blocks: int = 0  # the last encoder blocks that are MMDiTSingleStreamBlocks (ddt.py:169-199)

    def __post_init__(self) -> None:
        self.embedding_dim = self.inner_dim
        super().__post_init__()
        self.depth = self.encoder_depth + self.decoder_depth

    def validate(self) -> None:
        assert self.n_single_stream_blocks < self.encoder_depth, "n_single_stream_blocks must be less than encoder_depth"
        super().validate()

    def kinds(self) -> list[tuple[str, str]]:
        """(state_dict prefix, 'J' joint | 'S' single-stream | 'D' per-token decoder block) of every block in execution order"""
        nj = self.encoder_depth - self.n_single_stream_blocks
        return ([(f"layers.{i}.", "J" if i < nj else "S") for i in range(self.encoder_depth)]
                + [(f"decoder_layers.{i}.", "D") for i in range(self.decoder_depth)])


class DDTJointLayout(ArenaLayout):
    def _place(self, d: DDTJointDims) -> None:
        D, p, add = d.inner_dim, d.patch_size, self.add
        E, F = D, d.mlp_ratio * D
        kinds = d.kinds()
        self.prefixes = [pre for pre, _ in kinds]
        dec = [pre for pre, k in kinds if k == "D"]
        # per-sample adaLN of the encoder blocks: [input 6D | context 6D] per joint block, 3D per single-stream block
        self.add_stacked_adaln([(pre, k) for pre, k in kinds if k != "D"], D, E, last_layer=False)
        for suffix, shp in (("weight", lambda r: (r, E)), ("bias", lambda r: (r,))):
            for i, pre in enumerate(dec):  # per-token adaLN of the decoder blocks + last layer
                add(pre + "modulation.lin." + suffix, shp(6 * D), align=1 if i else 64)
            add("last_layer.adaLN_modulation.1." + suffix, shp(2 * D), align=1)
        self.mod_off += [0] * len(dec)
        self.tmod_rows = len(dec) * 6 * D + 2 * D
        self.tmod_w0, self.tmod_b0 = dec[0] + "modulation.lin.weight", dec[0] + "modulation.lin.bias"
        add("time_embed.0.weight", (E, d.frequency_embedding))
        add("time_embed.0.bias", (E,))
        add("time_embed.2.weight", (E, E))
        add("time_embed.2.bias", (E,))
        self.add_pooled_mlp(d.pooled_dim, E)
        add("conv_proj_encoder.weight", (D, d.input_channels, p, p))
        add("conv_proj_decoder.weight", (D, d.input_channels, p, p))
        add("context_embed.weight", (D, d.context_dim))
        add("last_layer.linear.weight", (p * p * d.output_channels, D))
        add("last_layer.linear.bias", (p * p * d.output_channels,))
        self.block_first = []
        for pre, kind in kinds:
            if kind == "J":
                self.block_first.append(pre + "input_norm_1.weight")
                self.add_joint_block(pre, D, F)
            elif kind == "S":
                self.block_first.append(pre + "norm.weight")
                self.add_single_block(pre, D, F)
            else:
                self.block_first.append(pre + "norm_1.weight")
                self.add_dit_block(pre, D, F)


class DDTJointEngine(SprintJointEngine, PerTokenDecoder):
    """DDT(simple_ddt=False) (ddt.py:274-344 + 404-464): joint text-image encoder stage (the MMDiTBlock sequence of
    DiTEngine._jstage_fwd; the context half of its last block feeds nothing), then the per-token-conditioned DDT decoder on the
    image rows of the 3-axis RoPE table"""

    _conv_name = "conv_proj_encoder.weight"

    def _make_layout(self, d: DDTJointDims) -> DDTJointLayout:  # type: ignore[override]
        self.kinds = d.kinds()
        return DDTJointLayout(d)

    def _extra_shadows(self, reg) -> None:
        d = self.d
        reg("context_embed.weight", d.inner_dim, d.context_dim, dgrad=False)
        reg("conv_proj_decoder.weight", d.inner_dim, d.input_channels * d.patch_size**2, dgrad=False)
        reg("@tmod", self.layout.tmod_rows, d.inner_dim)

    def _block_shadows(self, reg, pre: str) -> None:
        if dict(self.kinds)[pre] != "D":
            SprintJointEngine._block_shadows(self, reg, pre)
        else:
            super(SprintJointEngine, self)._block_shadows(reg, pre)  # DiT block names

    def _src(self, name: str, shape: tuple[int, int]) -> Tensor:
        if name == "@tmod":
            off = self.layout.entries[self.layout.tmod_w0][0]
            return self.params[off : off + shape[0] * shape[1]].view(shape)
        return super()._src(name, shape)

    def _alloc(self, B: int, H: int, W: int, train: bool, Lc: int = 0, k: int = 0) -> None:  # type: ignore[override]
        d, z, zr = self.d, self._z, self._zr
        key = (B, H, W, train, Lc)
        if self._cached(key):
            return
        D, E, p = d.inner_dim, d.embedding_dim, d.patch_size
        gh, gw = H // p, W // p
        N = gh * gw
        Tf = Lc + N
        Tpf = _rup(Tf, 256)
        if Tpf > ops.ATTN_MAX_TOKENS or (B * N) % 64 or Lc < 1:
            raise NotImplementedError(f"joint DDT HIP path: context + image tokens <= {ops.ATTN_MAX_TOKENS} (got {Lc} + {N}), batch * image tokens a "
                                      f"multiple of 64 (got {B} * {N})")
        pad = ops.attn_needs_padding(N)  # decoder attention on rows padded to a multiple of 256 with masked pad keys (_decoder_fwd)
        Nd = _rup(N, 256) if pad else N
        M, Bp, F = B * N, _rup(B, 64), d.mlp_ratio * D
        ops.check_row_extent(B * Tpf, max(2 * F, 6 * D, self.layout.tmod_rows), "joint DDT HIP path")
        f32 = torch.float32
        Hh, R = d.num_heads, self.layout.tmod_rows
        w: dict[str, object] = {}
        self._cond_buffers(w, B, H, W, train, train and self._grouped_widths())
        w["ctxP"] = zr(B * Lc, _rup(d.context_dim, 64))
        w["x"] = [z(M, D)]
        w["c0"] = zr(B * Lc, D)
        w["kb_f"] = z(B, Tpf, dtype=f32)
        w["kb_f"][:, Tf:] = float("-inf")
        blk = []
        for _, kind in self.kinds:
            if kind == "J":
                per = self._joint_attn_buffers(B, Tpf)
                for st, nt in (("input", N), ("context", Lc)):
                    per[st] = self._joint_stream_buffers(B, nt, train)
            elif kind == "S":
                per = self._joint_attn_buffers(B, Tpf)
                per.update(self._single_stream_buffers(B, Tf, train))
            else:
                per = self._dit_block_buffers(B, N, train, nq=Nd)
                if pad:
                    per["ao"] = z(B * Nd, D)
                if train:
                    per["dwbp"] = z(2, N_PART, 2, D, dtype=f32)
            blk.append(per)
        if pad:
            w["kb_d"] = z(B, Nd, dtype=f32)
            w["kb_d"][:, N:] = float("-inf")
        w["blk"] = blk
        w["xdec_in"], w["enc_out"], w["sz"] = z(M, D), z(M, D), z(M, D)
        w["tmod"] = z(M, R)
        w["xl"] = z(M, D)
        ns = d.n_single_stream_blocks
        if ns:  # outputs of the joint sub-stage, the concatenated [context ; image] latents into / out of the single-stream stage
            w["xj"], w["cj"] = z(M, D), zr(B * Lc, D)
            w["lat0"], w["lat_out"] = zr(B * Tf, D), zr(B * Tf, D)
        if train:
            if ns:
                w["s_l"] = {"dxa": zr(B * Tf, D), "dxb": zr(B * Tf, D), "dxm": zr(B * Tf, D), "dxm2": zr(B * Tf, D), "da": zr(B * Tf, D),
                            "dh": zr(B * Tf, F)}
                w["dlat"], w["dxj"], w["dcj"] = zr(B * Tf, D), z(M, D), zr(B * Lc, D)
            w[f"s_x{N}"] = {"dxa": z(M, D), "dxb": z(M, D), "dxm": z(M, D), "dxm2": z(M, D), "da": z(M, D), "dh": z(M, F),
                            "dq": z(B, Hh, Nd, 64), "dk": z(B, Hh, Nd, 64), "dv": z(B, Hh, Nd, 64)}
            if pad:
                w["dao_d"] = z(B * Nd, D)
            w["s_c"] = {"dxa": zr(B * Lc, D), "dxb": zr(B * Lc, D), "dxm": zr(B * Lc, D), "da": zr(B * Lc, D), "dh": zr(B * Lc, F)}
            w["dao_f"] = z(B * Tpf, D)
            w["dq_f"], w["dk_f"], w["dv_f"] = (z(B, Hh, Tpf, 64) for _ in range(3))
            w["dtmod"] = z(M, R)
            if ops.wgrad_tile_ok(R, D) and M % 32 == 0 and M >= 2048:  # two token ranges of the stacked per-token adaLN weight gradient
                w["tmod_slab"] = torch.empty(2 * R * D, device=self.dev, dtype=torch.float32)
            w["dsz"], w["denc"] = z(M, D), z(M, D)
            w["dtemb"] = z(Bp, E, dtype=f32)
            if D <= 512 and tuning.on("DL_QK_INPLACE") and not pad:  # scale-gradient partials of the in-place QK-norm backward (ops.qk_inplace_ok)
                w["qk_part"] = torch.empty(1024 * 2 * D, device=self.dev, dtype=f32)
        self._publish(w, key, (B, H, W, gh, gw, N, M, Bp, p * p * d.output_channels), (Lc, gh, gw),
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
        D, Cd, ne = d.inner_dim, d.context_dim, d.encoder_depth
        self._train, self._yeff, self._Lc = train, None, Lc
        self._tabs = self._rope[(Lc, gh, gw)]
        self._stem_fwd(x, t, None)
        ops.gemm_nt(w["tokP"], sh["conv_proj_decoder.weight|f"], w["xdec_in"], M=M, N=D, K=self._ki)
        w["ctxP"][:, :Cd].copy_(ctx.reshape(B * Lc, Cd))
        ops.gemm_nt(w["ctxP"], sh["context_embed.weight|f"], w["c0"], M=B * Lc, N=D, K=w["ctxP"].shape[1])
        kb = w["kb_f"]
        if keep is None:
            kb[:, :Lc].zero_()
        else:
            kb[:, :Lc].zero_().masked_fill_(~keep.to(device=kb.device, dtype=torch.bool), float("-inf"))
        nj = ne - d.n_single_stream_blocks
        if nj == ne:
            self._jstage_fwd(range(0, ne), w["x"][0], w["c0"], N, None, kb, w["enc_out"], None)
        else:  # encode_mmddt (ddt.py:352-406): joint blocks, then single-stream blocks on [context ; image]; the decoder is
            T = Lc + N  # conditioned on the image rows of the concatenated latents
            self._jstage_fwd(range(0, nj), w["x"][0], w["c0"], N, None, kb, w["xj"], w["cj"])
            lat0 = w["lat0"]
            ops.copy_rows3d(w["cj"], Lc * D, D, lat0, T * D, D, B, Lc, D)
            ops.copy_rows3d(w["xj"], N * D, D, lat0[Lc:], T * D, D, B, N, D)
            self._sstage_fwd(range(nj, ne), lat0, T, None, kb, w["lat_out"])
            ops.copy_rows3d(w["lat_out"][Lc:], T * D, D, w["enc_out"], N * D, D, B, N, D)
        cos, sin = self._tabs
        return self._decoder_fwd(ne, d.decoder_depth, cos[Lc:], sin[Lc:])

    def feature(self, kblk: int) -> Tensor:
        assert self._train and 0 <= kblk < self.d.encoder_depth
        B, N, D = self.geo[0], self.geo[5], self.d.inner_dim
        ne, nj = self.d.encoder_depth, self.d.encoder_depth - self.d.n_single_stream_blocks
        if kblk + 1 < nj:
            return self.ws["blk"][kblk + 1]["input"]["x0"].view(B, N, D)
        if kblk + 1 == nj:
            return (self.ws["enc_out"] if nj == ne else self.ws["xj"]).view(B, N, D)
        raise NotImplementedError("forward hooks on single-stream blocks (the image rows live inside the concatenated latents)")

    def backward(self, dpred: Tensor, dfeats: dict[int, Tensor] | None = None) -> None:
        assert self._train and self.grads is not None
        d, w = self.d, self.ws
        B, H, W, gh, gw, N, M, Bp, Fo = self.geo
        D, Cd, ne, Lc = d.inner_dim, d.context_dim, d.encoder_depth, self._Lc
        nj = ne - d.n_single_stream_blocks
        dfe = self._dfeat_rows(dfeats)
        cos, sin = self._tabs
        w["dmod32"][:B].zero_()
        sw = SideWork(self)
        denc = self._decoder_bwd(dpred, ne, d.decoder_depth, cos[Lc:], sin[Lc:], w[f"s_x{N}"], sw)
        scr, attn = self._jscratch(N, "f")
        gx, gc = denc, None
        if nj < ne:  # the gradient of the image rows flows back into the concatenated latents; their context rows feed nothing
            T = Lc + N
            dlat = w["dlat"]
            dlat.zero_()
            ops.copy_rows3d(denc, N * D, D, dlat[Lc:], T * D, D, B, N, D)
            dl = self._sstage_bwd(range(nj, ne), dlat, T, None, w["kb_f"], sw, attn=attn)
            ops.copy_rows3d(dl[Lc:], T * D, D, w["dxj"], N * D, D, B, N, D)
            ops.copy_rows3d(dl, T * D, D, w["dcj"], Lc * D, D, B, Lc, D)
            gx, gc = w["dxj"], w["dcj"]
        dx0, dc0 = self._jstage_bwd(range(0, nj), gx, gc, N, None, w["kb_f"], scr, attn, dfe, sw)
        sw.join()
        ops.gemm_tn(dc0, w["ctxP"], self.G("context_embed.weight"), M=D, N=Cd)
        self._cond_bwd(dx0, extra_demb=w["dtemb"])
