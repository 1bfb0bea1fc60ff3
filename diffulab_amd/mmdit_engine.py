"""Host-side runtime of MMDiT with joint text-image blocks (simple_dit=False; reference networks/denoisers/mmdit.py:107-210,
312-439, 789-851): the DiT engine's arena / shadows / conditioning path, with two token streams per block.

Per block, each stream ("input" = image tokens, "context" = text tokens) runs the DiT sub-layer sequence with its own weights and
its own six modulation rows; the two meet only in the attention: the QK-norm + RoPE kernel of each stream writes its window of
the JOINT q / k / v buffers [B, H, Tp, 64] (rows [0, Lc) context, [Lc, Lc + N) image, padded to a multiple of 256), one
attention launch covers the joint sequence with the key-padding mask as an additive key bias, and the two halves of the result
are sliced back per stream.  The 3-axis RoPE table of the joint sequence (text (1..Lc, 0, 0), image (0, h, w)) is built once per
shape; the context stream of the LAST block feeds nothing (mmdit.py:838-842) and is skipped after the attention.  The block
sequence itself is DiTEngine._jstage_fwd / _jstage_bwd (engine.py), run here as ONE stage over every block whose last image-stream
residual stays pending for the final LayerNorm.
"""

from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import Tensor

from . import ops
from .engine import ROW_MAX_DIM, STREAMS, ArenaLayout, DiTDims, DiTEngine, Modulation, SideWork, _rup


@dataclass
class JointDims(DiTDims):
    context_dim: int = 768
    pooled_dim: int = 0  # width of the pooled context embedding (two-output embedder -> mlp_pooled_context); 0: none

    def __post_init__(self) -> None:
        if not self.rope_axes_dim:
            self.rope_axes_dim = [self.head_dim // 3] * 3  # mmdit.py:659-664

    def validate(self) -> None:
        D, E = self.inner_dim, self.embedding_dim
        if self.head_dim != 64:
            raise NotImplementedError(f"HIP attention kernels are built for head_dim 64 (got {self.head_dim})")
        if D % 64 or E % 64 or self.frequency_embedding % 64 or D > ROW_MAX_DIM:
            raise NotImplementedError(f"inner_dim (<= {ROW_MAX_DIM}), embedding_dim and frequency_embedding must be multiples of 64 "
                                      f"(got inner_dim {D})")
        if len(self.rope_axes_dim) != 3 or any(a % 2 for a in self.rope_axes_dim) or sum(self.rope_axes_dim) % 8 or \
                sum(self.rope_axes_dim) > self.head_dim:
            raise NotImplementedError("joint blocks use a 3-axis RoPE (text position, row, col) with even axis widths whose sum is "
                                      f"a multiple of 8 and <= head_dim (got {self.rope_axes_dim})")
        if self.context_dim % 8:
            raise NotImplementedError("context embedding width must be a multiple of 8")
        if self.pooled_dim % 8:
            raise NotImplementedError(f"pooled context embedding width must be a multiple of 8 (got pooled_dim {self.pooled_dim})")
        if self.n_classes is not None:
            raise NotImplementedError("joint blocks are conditioned on a context embedder, not on class labels")


def joint_rope_tables(n_ctx: int, gh: int, gw: int, axes_dim: list[int], base: float) -> tuple[Tensor, Tensor]:
    """cos / sin [n_ctx + gh*gw, sum(axes)/2]: ids of mmdit.py:813-835 (text (t, 0, 0) with t = 1..n_ctx, image (0, h, w)) through
    nn.py:276-307 (angles in fp64, cast to fp32)"""
    pos = torch.zeros(n_ctx + gh * gw, 3, dtype=torch.float64)
    pos[:n_ctx, 0] = torch.arange(1, n_ctx + 1, dtype=torch.float64)
    pos[n_ctx:, 1] = torch.arange(gh, dtype=torch.float64).repeat_interleave(gw)
    pos[n_ctx:, 2] = torch.arange(gw, dtype=torch.float64).repeat(gh)
    cs, sn = [], []
    for a, d in enumerate(axes_dim):
        inv = 1.0 / (torch.tensor(float(base), dtype=torch.float64) ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
        ang = pos[:, a, None] * inv[None, :]
        cs.append(ang.cos().float())
        sn.append(ang.sin().float())
    return torch.cat(cs, 1).contiguous(), torch.cat(sn, 1).contiguous()


class JointLayout(ArenaLayout):
    """the stacked adaLN matrix ([input 6D | context 6D] per block, then the last layer's 2D rows) and its bias first, then stem /
    head, then the blocks"""

    def _place(self, d: JointDims) -> None:
        D, E, p, add = d.inner_dim, d.embedding_dim, d.patch_size, self.add
        self.prefixes = [f"layers.{i}." for i in range(d.depth)]
        first = True
        for pre in self.prefixes:
            for st in STREAMS:
                add(pre + f"modulation_{st}.lin.weight", (6 * D, E), align=64 if first else 1)
                first = False
        add("last_layer.adaLN_modulation.1.weight", (2 * D, E), align=1)
        first = True
        for pre in self.prefixes:
            for st in STREAMS:
                add(pre + f"modulation_{st}.lin.bias", (6 * D,), align=64 if first else 1)
                first = False
        add("last_layer.adaLN_modulation.1.bias", (2 * D,), align=1)
        self.mod_off = [i * 12 * D for i in range(d.depth)]  # modulation columns of every block: [input 6D | context 6D]
        self.mod_rows = d.depth * 12 * D + 2 * D
        self.mod_w0, self.mod_b0 = "layers.0.modulation_input.lin.weight", "layers.0.modulation_input.lin.bias"
        add("time_embed.0.weight", (E, d.frequency_embedding))
        add("time_embed.0.bias", (E,))
        add("time_embed.2.weight", (E, E))
        add("time_embed.2.bias", (E,))
        self.add_pooled_mlp(d.pooled_dim, E)
        add("conv_proj.weight", (D, d.input_channels, p, p))
        add("context_embed.weight", (D, d.context_dim))
        add("last_layer.linear.weight", (p * p * d.output_channels, D))
        add("last_layer.linear.bias", (p * p * d.output_channels,))
        self.block_first = []
        for pre in self.prefixes:
            self.block_first.append(pre + "input_norm_1.weight")
            self.add_joint_block(pre, D, d.mlp_ratio * D)


class JointEngine(DiTEngine):
    context: tuple[Tensor, Tensor | None] | None = None  # (embeddings [B, Lc, context_dim], keep bool [B, Lc] | None) of this step

    def _make_layout(self, d: JointDims) -> JointLayout:  # type: ignore[override]
        return JointLayout(d)

    def _extra_shadows(self, reg) -> None:
        reg("context_embed.weight", self.d.inner_dim, self.d.context_dim, dgrad=False)

    def _block_shadows(self, reg, pre: str) -> None:
        d, dev = self.d, self.dev
        D, F = d.inner_dim, d.mlp_ratio * d.inner_dim
        for st in STREAMS:
            reg(pre + f"attention.qkv_{st}.weight", 3 * D, D)
            reg(pre + f"attention.{st}_proj_out.weight", D, D)
            reg(pre + f"mlp_{st}.0.weight", 2 * F, D)
            self.sh[pre + f"mlp_{st}.0.weight|g"] = torch.zeros(2 * F, D, device=dev, dtype=torch.bfloat16)
            reg(pre + f"mlp_{st}.2.weight", D, F)

    # ------------------------------------------------------------------ workspace
    def _alloc(self, B: int, H: int, W: int, train: bool, Lc: int = 0) -> None:  # type: ignore[override]
        d, z, zr = self.d, self._z, self._zr
        key = (B, H, W, train, Lc)
        if self._cached(key):
            return
        D, p, L = d.inner_dim, d.patch_size, d.depth
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
        w: dict[str, object] = {}
        self._cond_buffers(w, B, H, W, train, train and self._grouped_widths())
        w["ctxP"] = zr(B * Lc, _rup(d.context_dim, 64))
        w["x"] = [z(M, D)]
        w["c0"] = zr(B * Lc, D)
        w["kbias"] = z(B, Tp, dtype=f32)
        w["kbias"][:, T:] = float("-inf")  # padded key rows
        w["q"], w["k"], w["v"] = (z(B, d.num_heads, Tp, 64) for _ in range(3))
        ntok = {"input": N, "context": Lc}
        blk = []
        for _ in range(L):
            per = {"ao": z(B * Tp, D), "lse": z(B, d.num_heads, Tp, dtype=f32)}
            for st in STREAMS:
                per[st] = self._joint_stream_buffers(B, ntok[st], train)
            if train:  # q / k / v of every block are kept for the backward
                per["q"], per["k"], per["v"] = (z(B, d.num_heads, Tp, 64) for _ in range(3))
            blk.append(per)
        w["blk"] = blk
        w["xl"] = z(M, D)
        if train:
            for st in STREAMS:
                mt = B * ntok[st]
                w["s_" + st] = {"dxa": zr(mt, D), "dxb": zr(mt, D), "dxm": zr(mt, D), "da": zr(mt, D), "dh": zr(mt, F)}
            w["dao"] = z(B * Tp, D)
            w["dq"], w["dk"], w["dv"] = (z(B, d.num_heads, Tp, 64) for _ in range(3))
        self._publish(w, key, (B, H, W, gh, gw, N, M, _rup(B, 64), p * p * d.output_channels), (Lc, gh, gw),
                      lambda: joint_rope_tables(Lc, gh, gw, d.rope_axes_dim, d.rope_base))

    # ------------------------------------------------------------------ forward
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
        _, _, _, gh, gw, N, _, _, _ = self.geo
        D, L, Cd = d.inner_dim, d.depth, d.context_dim
        self._train, self._yeff, self._Lc = train, None, Lc
        self._tabs = self._rope[(Lc, gh, gw)]
        mod = self._stem_fwd(x, t, None)
        # context stream input: embeddings -> context_embed (mmdit.py:808-809); key-padding mask -> additive key bias
        w["ctxP"][:, :Cd].copy_(ctx.reshape(B * Lc, Cd))
        ops.gemm_nt(w["ctxP"], sh["context_embed.weight|f"], w["c0"], M=B * Lc, N=D, K=w["ctxP"].shape[1])
        kb = w["kbias"]
        if keep is None:
            kb[:, :Lc].zero_()
        else:
            kb[:, :Lc].zero_().masked_fill_(~keep.to(device=kb.device, dtype=torch.bool), float("-inf"))
        # one joint stage over every block; the final LayerNorm absorbs the image stream's last gated residual
        pend = self._jstage_fwd(range(L), w["x"][0], w["c0"], N, None, kb, None, None)
        return self._head_fwd(Modulation(mod, None, L * 12 * D, D, N), w["xl"], pend)

    def feature(self, kblk: int) -> Tensor:
        """image-stream output of block k of the last train-mode forward (what a hook on ``layers[k]`` sees as output[0])"""
        assert self._train
        B, N, D = self.geo[0], self.geo[5], self.d.inner_dim
        if kblk + 1 < self.d.depth:
            return self.ws["blk"][kblk + 1]["input"]["x0"].view(B, N, D)
        return self.ws["xl"].view(B, N, D)

    # ------------------------------------------------------------------ backward
    def backward(self, dpred: Tensor, dfeats: dict[int, Tensor] | None = None) -> None:
        assert self._train and self.grads is not None
        d, w = self.d, self.ws
        B, N = self.geo[0], self.geo[5]
        D, L, Cd = d.inner_dim, d.depth, d.context_dim
        dfe = self._dfeat_rows(dfeats)
        mod, dmod = w["mod"], w["dmod32"]
        dmod[:B].zero_()
        scr = {"input": w["s_input"], "context": w["s_context"]}
        si = scr["input"]

        self._head_bwd(dpred, si["dxm"])
        al = w["blk"][L - 1]["input"]
        Modulation(mod, dmod, L * 12 * D, D, N).ln_bwd(si["dxm"], w["xl"], None, None, 0, w["meanf"], w["rstdf"], dfe.get(L - 1), si["dxa"],
                                                       None, gate=(al["t2"], (L - 1) * 12 * D + 5 * D, al["wg"]["dt2"]))
        sw = SideWork(self)
        dx0, dc0 = self._jstage_bwd(range(L), si["dxa"], None, N, None, w["kbias"], scr, (w["dao"], w["dq"], w["dk"], w["dv"]), dfe, sw,
                                    pending=True)
        sw.join()
        # context_embed (no gradient flows into the precomputed embeddings)
        ops.gemm_tn(dc0, w["ctxP"], self.G("context_embed.weight"), M=D, N=Cd)
        self._cond_bwd(dx0)
