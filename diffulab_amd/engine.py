"""Host-side runtime of the DiT hot path: parameter arena, bf16 weight shadows, activation workspace and
the forward / backward launch sequences over the C ABI.

MI355X-first choices:
  * all parameters live in ONE flat f32 HBM buffer (and one flat gradient buffer): the optimizer is a single
    fused launch and the data-parallel reduction is a handful of large RCCL collectives on contiguous memory;
  * the adaLN linears of every block (and of the last layer) are stored back to back so the modulation of the
    whole network is ONE GEMM per step (the conditioning vector is layer-invariant);
  * every activation is preallocated (288 GB of HBM3E: keep, don't recompute) so a step performs no
    allocation and the launch sequence is static (hipGraph-capturable);
  * residual stream and GEMM operands are bf16, accumulation / norm statistics / gradients of parameters f32.

One owner per launch sequence: the Python-issued DiT block (_dit_block_fwd / _dit_block_bwd, built from the halves _half1_* /
_half2_* and the attention pair _attn_fwd / _attn_bwd) serves DiTEngine's plain path, the SPRINT / DDT stages and the DDT decoder;
the joint (MMDiT) block stage (_jstage_fwd / _jstage_bwd) runs the same halves per token stream and serves every engine with joint
blocks.  What differs between callers is data: buffers, parameter names (block_names) and the adaLN rows in force (Modulation).

Reference sites restated by the sequences below: mmdit.py:853-928 (simple_dit_forward / forward),
mmdit.py:288-309 (DiTBlock), mmdit.py:75-104 (DiTAttention), mmdit.py:542-549 (ModulatedLastLayer).
"""

from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import torch
from torch import Tensor

from . import ops, tuning


_PARAM_EPOCH = 0


def bump_param_epoch() -> None:
    """to be called by anything that writes parameters through a raw pointer (fused AdamW / EMA kernels):
    torch version counters do not see those writes, and the bf16 weight shadows are keyed on this epoch."""
    global _PARAM_EPOCH
    _PARAM_EPOCH += 1


def _must(ok: bool) -> None:
    """an entry point that may answer DL_ERR_UNSUPPORTED was chosen for a shape it must serve (no assert: -O would drop the call)"""
    if not ok:
        raise RuntimeError("a HIP kernel declined a shape the engine had selected it for")


def _rup(x: int, m: int) -> int:
    return (x + m - 1) // m * m


STREAMS = ("input", "context")  # the two token streams of a joint (MMDiT) block: image, text
ROW_MAX_DIM = 4096  # widest token row of the bf16 regime's row kernels (csrc/norm.hip: one wave per row up to 1024, one workgroup above)
F32_MAX_DIM = 1024  # widest token row of the fp32 regime (csrc/f32.hip, one wave per row)


@functools.lru_cache(maxsize=None)
def block_names(pre: str, st: str | None = None) -> dict[str, str]:
    """parameter name stems of the DiT block `pre` (st None) or of token stream `st` of the joint block `pre`: the two block kinds
    run the same sub-layer sequence (DiTEngine._half1_fwd ...) under different names"""
    if st is None:
        n = dict(n1="norm_1", n2="norm_2", qk="attention.qk_norm", qkv="attention.qkv", proj="attention.proj_out", up="mlp_input.0",
                 down="mlp_input.2")
    else:
        n = dict(n1=f"{st}_norm_1", n2=f"{st}_norm_2", qk=f"attention.qk_norm_{st}", qkv=f"attention.qkv_{st}",
                 proj=f"attention.{st}_proj_out", up=f"mlp_{st}.0", down=f"mlp_{st}.2")
    return {k: pre + v for k, v in n.items()}


@dataclass(slots=True)
class Modulation:
    """the six adaLN chunks (scale1, shift1, gate1, scale2, shift2, gate2) a block's two LayerNorms and gated residuals read -- or
    the two of the final LayerNorm -- as columns [off, off + 6D) of `mat`.  Per sample (`rows` tokens share a row of mat, gradients
    accumulate into the f32 `dmat`, the LayerNorm-affine partials `part` [2, groups, 2, D] hold one group per sample) or per token
    (DDT decoder: rows = 1, tok selects dl_ln_modulate_bwd_tok, which writes bf16 gradient rows into dmat and a fixed number of partial groups)"""
    mat: Tensor
    dmat: Tensor | None   # None: forward only
    off: int
    D: int
    rows: int
    tok: bool = False
    part: Tensor | tuple | None = None   # part[0]: norm_1, part[1]: norm_2
    groups: int = 0

    def col(self, c: int) -> Tensor:
        o = self.off + c * self.D
        return self.mat[:, o : o + self.D]

    def ln_bwd(self, dout: Tensor, x: Tensor, lnw: Tensor | None, lnb: Tensor | None, c: int, mean: Tensor, rstd: Tensor,
               dres: Tensor | None, dx: Tensor, part: Tensor | None, gate: tuple | None = None) -> None:
        """backward of the LayerNorm-modulate on chunks c (scale), c + 1 (shift): dx = dres + its data gradient.  Every
        LayerNorm-modulate backward also runs the backward of the gated residual that follows it in the chain (x_new = x + gate * t):
        it has the residual-stream gradient dx in registers, so dt = gate * dx and dgate += dx * t cost one extra row read / write
        instead of a separate pass over dx.  gate = (t, column of that gate in mat, dt) or None"""
        D, o, mat, dmat = self.D, self.off + c * self.D, self.mat, self.dmat
        kw = {}
        if gate is not None:
            t, go, dt = gate
            kw = dict(gate_t=t, gate=mat[:, go : go + D], dt=dt, dgate=dmat[:, go : go + D])
        if self.tok:
            ops.ln_modulate_bwd_tok(dout, x, lnw, lnb, mat[:, o : o + D], mean, rstd, dres, dx, dmat[:, o : o + D],
                                    dmat[:, o + D : o + 2 * D], part, **kw)
        else:
            ops.ln_modulate_bwd(dout, x, lnw, lnb, mat[:, o : o + D], self.rows, mean, rstd, dres, dx, dmat[:, o : o + D],
                                dmat[:, o + D : o + 2 * D], part, **kw)


def _other(s: dict, cur: Tensor | None) -> Tensor:
    """ping-pong target of the next LayerNorm backward in the chain scratch s (never the buffer it reads)"""
    return s["dxb"] if (cur is not None and cur.data_ptr() == s["dxa"].data_ptr()) else s["dxa"]


@dataclass
class DiTDims:
    input_channels: int = 4
    output_channels: int = 4
    inner_dim: int = 384
    embedding_dim: int = 384
    num_heads: int = 6
    mlp_ratio: int = 4
    patch_size: int = 2
    depth: int = 12
    rope_base: float = 10_000.0
    frequency_embedding: int = 256
    n_classes: int | None = 1000
    classifier_free: bool = True
    rope_axes_dim: list[int] = field(default_factory=list)

    def __post_init__(self) -> None:
        if not self.rope_axes_dim:
            hd = self.inner_dim // self.num_heads
            self.rope_axes_dim = [hd // 2, hd // 2]

    @property
    def head_dim(self) -> int:
        return self.inner_dim // self.num_heads

    def validate(self) -> None:
        D, E = self.inner_dim, self.embedding_dim
        if self.head_dim != 64:
            raise NotImplementedError(f"HIP attention kernels are built for head_dim 64 (got {self.head_dim})")
        if D % 64 or E % 64 or self.frequency_embedding % 64:
            raise NotImplementedError("inner_dim, embedding_dim and frequency_embedding must be multiples of 64")
        if D > ROW_MAX_DIM:
            raise NotImplementedError(f"the bf16 regime's row kernels take inner_dim <= {ROW_MAX_DIM} (got {D})")
        if sum(self.rope_axes_dim) > self.head_dim or sum(self.rope_axes_dim) % 8:
            raise NotImplementedError("rotary width must be a multiple of 8 and <= head_dim")
        if len(self.rope_axes_dim) != 2:
            raise NotImplementedError("simple_dit uses a 2-axis (row, col) RoPE")


def rope_grid_tables(gh: int, gw: int, axes_dim: list[int], base: float) -> tuple[Tensor, Tensor]:
    """cos/sin tables [gh*gw, sum(axes)/2] of the 2-D grid, angles in fp64 then cast to fp32 exactly like
    nn.py:276-307 applied to the meshgrid(indexing='ij') ids of mmdit.py:871-886 (row axis first)."""
    pos = (torch.arange(gh, dtype=torch.float64).repeat_interleave(gw), torch.arange(gw, dtype=torch.float64).repeat(gh))
    cs, sn = [], []
    for p, d in zip(pos, axes_dim):
        inv = 1.0 / (torch.tensor(float(base), dtype=torch.float64) ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
        ang = p[:, None] * inv[None, :]
        cs.append(ang.cos().float())
        sn.append(ang.sin().float())
    return torch.cat(cs, 1).contiguous(), torch.cat(sn, 1).contiguous()


class ArenaLayout:
    """name -> (offset, shape) inside the flat f32 arena.  A subclass places its entries in `_place` with `add`; every entry starts
    on a 256-byte boundary unless placed with align=1 (adjacent to the one before), and the arena ends on one."""

    def __init__(self, *args, **kwargs) -> None:
        self.entries: dict[str, tuple[int, tuple[int, ...]]] = {}
        self.size = 0
        self._place(*args, **kwargs)
        self.size = _rup(self.size, 64)

    def _place(self, *args, **kwargs) -> None:
        raise NotImplementedError

    def add(self, name: str, shape: tuple[int, ...], align: int = 64) -> None:
        self.size = _rup(self.size, align)
        self.entries[name] = (self.size, shape)
        self.size += math.prod(shape)

    def add_dit_block(self, pre: str, D: int, F: int) -> None:
        """the parameters of a DiTBlock except its adaLN linear"""
        self.add(pre + "norm_1.weight", (D,))
        self.add(pre + "norm_1.bias", (D,), align=1)  # [w; b] adjacent: one reduce writes both gradients
        self.add(pre + "norm_2.weight", (D,))
        self.add(pre + "norm_2.bias", (D,), align=1)
        self.add(pre + "attention.qk_norm.query_norm.scale", (D,))
        self.add(pre + "attention.qk_norm.key_norm.scale", (D,), align=1)
        self.add(pre + "attention.qkv.weight", (3 * D, D))
        self.add(pre + "attention.proj_out.weight", (D, D))
        self.add(pre + "mlp_input.0.weight", (2 * F, D))
        self.add(pre + "mlp_input.2.weight", (D, F))

    def add_joint_block(self, pre: str, D: int, F: int) -> None:
        """the parameters of an MMDiTBlock (both token streams) except its adaLN linears"""
        for st in STREAMS:
            for n in (1, 2):
                self.add(pre + f"{st}_norm_{n}.weight", (D,))
                self.add(pre + f"{st}_norm_{n}.bias", (D,), align=1)
            self.add(pre + f"attention.qk_norm_{st}.query_norm.scale", (D,))
            self.add(pre + f"attention.qk_norm_{st}.key_norm.scale", (D,), align=1)
            self.add(pre + f"attention.qkv_{st}.weight", (3 * D, D))
            self.add(pre + f"attention.{st}_proj_out.weight", (D, D))
            self.add(pre + f"mlp_{st}.0.weight", (2 * F, D))
            self.add(pre + f"mlp_{st}.2.weight", (D, F))

    def add_single_block(self, pre: str, D: int, F: int) -> None:
        """the parameters of an MMDiTSingleStreamBlock except its adaLN linear"""
        self.add(pre + "norm.weight", (D,))
        self.add(pre + "norm.bias", (D,), align=1)
        self.add(pre + "attention.qk_norm.query_norm.scale", (D,))
        self.add(pre + "attention.qk_norm.key_norm.scale", (D,), align=1)
        self.add(pre + "attention.qkv.weight", (3 * D, D))
        self.add(pre + "attention.proj_out.weight", (D, D))
        self.add(pre + "mlp.0.weight", (2 * F, D))
        self.add(pre + "mlp.2.weight", (D, F))

    def add_stacked_adaln(self, kinds: list[tuple[str, str]], D: int, E: int, last_layer: bool) -> None:
        """the per-sample adaLN linears of the blocks `kinds` ((prefix, 'J' joint | 'S' single-stream)) back to back as ONE
        [mod_rows, E] matrix, then their biases: [input 6D | context 6D] per joint block, 3D per single-stream block, then
        (last_layer) the last layer's 2D rows.  Sets mod_off (first modulation column of every block), mod_rows, mod_w0 / mod_b0"""
        def mods(suffix: str, width) -> list:
            names = []
            for pre, kind in kinds:
                if kind == "J":
                    names += [(pre + f"modulation_{st}.lin.{suffix}", width(6)) for st in STREAMS]
                else:
                    names.append((pre + f"modulation.1.{suffix}", width(3)))
            return names

        self.mod_off, off = [], 0
        for _, kind in kinds:
            self.mod_off.append(off)
            off += (12 if kind == "J" else 3) * D
        self.mod_rows = off + (2 * D if last_layer else 0)
        for suffix, width in (("weight", lambda r: (r * D, E)), ("bias", lambda r: (r * D,))):
            names = mods(suffix, width)
            for i, (n, shp) in enumerate(names):
                self.add(n, shp, align=1 if i else 64)
            if suffix == "weight":
                self.mod_w0 = names[0][0]
            else:
                self.mod_b0 = names[0][0]
            if last_layer:
                self.add("last_layer.adaLN_modulation.1." + suffix, width(2), align=1)

    def add_pooled_mlp(self, P: int, E: int) -> None:
        """mlp_pooled_context = Linear(P, 2E) -> SiLU -> Linear(2E, E) of a joint form behind a two-output context embedder
        (mmdit.py:650-657); P = 0: the embedder has no pooled output and nothing is placed"""
        if P:
            self.add("mlp_pooled_context.0.weight", (2 * E, P))
            self.add("mlp_pooled_context.0.bias", (2 * E,))
            self.add("mlp_pooled_context.2.weight", (E, 2 * E))
            self.add("mlp_pooled_context.2.bias", (E,))

    def view(self, flat: Tensor, name: str) -> Tensor:
        off, shape = self.entries[name]
        return flat[off : off + math.prod(shape)].view(shape)


class ParamLayout(ArenaLayout):
    """Order: adaLN weights of all blocks + last layer (one [L*6D+2D, E] matrix), their biases, then everything else."""

    def _place(self, d: DiTDims, prefixes: list[str] | None = None, extra: tuple[tuple[str, tuple[int, ...]], ...] = ()) -> None:
        """prefixes: state_dict prefix of every adaLN-zero block in execution order (default ``layers.{i}.``);
        extra: further non-block parameters (SPRINT's mask token and fuse linear), placed with the stem / head entries"""
        D, E, p, add = d.inner_dim, d.embedding_dim, d.patch_size, self.add
        self.prefixes = prefixes = list(prefixes) if prefixes is not None else [f"layers.{i}." for i in range(d.depth)]
        nb = len(prefixes)

        # -- contiguous adaLN matrix / bias (rows are multiples of 64*... so no padding is inserted between them)
        for i, pre in enumerate(prefixes):
            add(pre + "modulation.lin.weight", (6 * D, E), align=1 if i else 64)
        add("last_layer.adaLN_modulation.1.weight", (2 * D, E), align=1)
        for i, pre in enumerate(prefixes):
            add(pre + "modulation.lin.bias", (6 * D,), align=1 if i else 64)
        add("last_layer.adaLN_modulation.1.bias", (2 * D,), align=1)
        self.mod_rows = nb * 6 * D + 2 * D
        self.mod_w0, self.mod_b0 = prefixes[0] + "modulation.lin.weight", prefixes[0] + "modulation.lin.bias"
        self.block_first = [pre + "norm_1.weight" for pre in prefixes]
        if d.n_classes is not None:
            add("label_embed.embedding.weight", (d.n_classes + (1 if d.classifier_free else 0), E))
        add("time_embed.0.weight", (E, d.frequency_embedding))
        add("time_embed.0.bias", (E,))
        add("time_embed.2.weight", (E, E))
        add("time_embed.2.bias", (E,))
        add("conv_proj.weight", (D, d.input_channels, p, p))
        add("last_layer.linear.weight", (p * p * d.output_channels, D))
        add("last_layer.linear.bias", (p * p * d.output_channels,))
        for name, shape in extra:
            add(name, shape)
        for pre in prefixes:
            self.add_dit_block(pre, D, d.mlp_ratio * D)


class DiTEngine:
    _conv_name = "conv_proj.weight"  # patch-embedding convolution of the (encoder) token stream
    pooled: Tensor | None = None  # pooled context embedding [B, pooled_dim] of this step (joint forms with dims.pooled_dim > 0)

    def __init__(self, dims: DiTDims, device: torch.device | str = "cuda") -> None:
        dims.validate()
        self.d = dims
        self.dev = torch.device(device)
        self._ki = _rup(dims.input_channels * dims.patch_size**2, 64)   # K of the patch-embedding GEMM (zero-padded)
        self._ko = _rup(dims.output_channels * dims.patch_size**2, 64)  # K of the last linear's data gradient
        self._pooled_dim = getattr(dims, "pooled_dim", 0)  # width of the pooled context embedding (joint forms; 0: none)
        self.layout = self._make_layout(dims)
        self.prefixes = self.layout.prefixes
        self.params: Tensor | None = None
        self.grads: Tensor | None = None
        self._shadow_key: tuple | None = None
        self.manual_version = 0
        self.param_version = 0  # sum of the parameters' own version counters, set by the owning module before every forward
        self._ws_key: tuple | None = None
        self._ws_cache: dict[tuple, tuple] = {}
        self._cast_table = None
        self._cast_table_ptr = 0
        self._rope: dict[tuple[int, int], tuple[Tensor, Tensor]] = {}
        self.reducer = None  # optional training.dp.GradReducer: gets ready(lo, hi) as gradient ranges complete
        self._build_shadows()
        ent = self.layout.entries
        starts = [ent[n][0] for n in self.layout.block_first] + [self.layout.size]
        self.layer_ranges = [(starts[i], starts[i + 1]) for i in range(len(self.prefixes))]

    def _make_layout(self, dims: DiTDims) -> ParamLayout:
        return ParamLayout(dims)

    # ------------------------------------------------------------------ parameters
    def bind(self, params: Tensor, grads: Tensor | None) -> None:
        assert params.dtype == torch.float32 and params.numel() == self.layout.size and params.is_cuda
        self.params, self.grads = params, grads
        self._shadow_key = None
        self._blk_cache: dict[tuple, object] = {}
        self._pviews: dict[str, Tensor] = {}
        self._gviews: dict[str, Tensor] = {}

    def P(self, name: str) -> Tensor:
        v = self._pviews.get(name)  # (views of the arena are cached: creating one costs ~3 us and a block uses a dozen)
        if v is None:
            v = self._pviews[name] = self.layout.view(self.params, name)
        return v

    def G(self, name: str) -> Tensor:
        v = self._gviews.get(name)
        if v is None:
            v = self._gviews[name] = self.layout.view(self.grads, name)
        return v

    def _build_shadows(self) -> None:
        """bf16 copies consumed by the MFMA GEMMs: W [out, rup64(in)] for forward, W^T [in, rup64(out)] for dgrad."""
        d, dev = self.d, self.dev
        D, E = d.inner_dim, d.embedding_dim
        self.sh: dict[str, Tensor] = {}
        self._casts: list[tuple[str, tuple[int, int], str | None, str | None]] = []

        def reg(name: str, R: int, C: int, fwd: bool = True, dgrad: bool = True) -> None:
            f = t = None
            if fwd:
                f = name + "|f"
                self.sh[f] = torch.zeros(R, _rup(C, 64), device=dev, dtype=torch.bfloat16)
            if dgrad:
                t = name + "|t"
                self.sh[t] = torch.zeros(C, _rup(R, 64), device=dev, dtype=torch.bfloat16)
            self._casts.append((name, (R, C), f, t))

        self.mod_name = self.layout.mod_w0  # start of the stacked [mod_rows, E] matrix
        reg("@mod", self.layout.mod_rows, E)
        reg("time_embed.0.weight", E, d.frequency_embedding, dgrad=False)
        reg("time_embed.2.weight", E, E)
        if self._pooled_dim:
            reg("mlp_pooled_context.0.weight", 2 * E, self._pooled_dim, dgrad=False)
            reg("mlp_pooled_context.2.weight", E, 2 * E)
        reg(self._conv_name, D, d.input_channels * d.patch_size**2, dgrad=False)
        reg("last_layer.linear.weight", d.patch_size**2 * d.output_channels, D)
        self._extra_shadows(reg)
        for pre in self.prefixes:
            self._block_shadows(reg, pre)

    def _block_shadows(self, reg, pre: str) -> None:
        d, dev = self.d, self.dev
        D = d.inner_dim
        reg(pre + "attention.qkv.weight", 3 * D, D)
        reg(pre + "attention.proj_out.weight", D, D)
        reg(pre + "mlp_input.0.weight", 2 * d.mlp_ratio * D, D)
        self.sh[pre + "mlp_input.0.weight|g"] = torch.zeros(2 * d.mlp_ratio * D, D, device=dev, dtype=torch.bfloat16)
        reg(pre + "mlp_input.2.weight", D, d.mlp_ratio * D)

    def _extra_shadows(self, reg) -> None:  # hook: shadows of further linears (subclasses)
        pass

    def _src(self, name: str, shape: tuple[int, int]) -> Tensor:
        if name == "@mod":
            off = self.layout.entries[self.mod_name][0]
            return self.params[off : off + shape[0] * shape[1]].view(shape)
        return self.P(name).view(shape)

    def refresh_shadows(self, force: bool = False) -> None:
        ver = 0 if self.params.is_inference() else self.params._version
        # writes THROUGH a parameter (load_state_dict on a flattened model, a stock optimizer, p.copy_) bump that parameter's
        # version counter, not the arena's: the owning module passes the sum of those counters as param_version
        key = (self.params.data_ptr(), ver, self.manual_version, _PARAM_EPOCH, self.param_version)
        if not force and key == self._shadow_key:
            return
        if self._cast_table is None or self._cast_table_ptr != self.params.data_ptr():
            ent = []  # one device table for all shadows (incl. the row-permuted MLP-up copy of the fused SwiGLU kernel)
            for name, shape, f, t in self._casts:
                g = self.sh.get(name + "|g")
                ent.append((self._src(name, shape), self.sh[f] if f else None, self.sh[t] if t else None, g))
            self._cast_table, self._cast_table_ptr = ops.CastTable(ent), self.params.data_ptr()
        self._cast_table.run()
        self._shadow_key = key

    def _side_stream(self) -> "torch.cuda.Stream":
        if getattr(self, "_side", None) is None:
            mask = tuning.text("DL_SIDE_CU_MASK")  # e.g. "i4" = every 4th CU, "b128" = the first 128 CUs
            if mask:
                self._side = ops.masked_stream(mask, self.dev)
            elif tuning.on("DL_SIDE_LOW_PRIORITY"):
                self._side = ops.low_priority_stream(self.dev)
            else:
                self._side = torch.cuda.Stream(device=self.dev)
        return self._side

    def params_changed(self) -> None:
        """call after writing the parameter arena through a raw pointer (fused AdamW)."""
        self.manual_version += 1

    # ------------------------------------------------------------------ workspace
    def _z(self, *shape, dtype: torch.dtype = torch.bfloat16) -> Tensor:
        with torch.inference_mode(False):  # workspaces outlive an inference_mode() sampler loop
            return torch.zeros(*shape, device=self.dev, dtype=dtype)

    def _zr(self, rows: int, *rest, dtype: torch.dtype = torch.bfloat16) -> Tensor:
        """row buffer: zero rows pad it to a multiple of 64 for the weight-gradient GEMMs"""
        return self._z(_rup(rows, 64), *rest, dtype=dtype)[:rows]

    def _cached(self, key: tuple) -> bool:
        """select the workspace of `key` if it exists (workspaces are kept per shape: captured hipGraphs have their addresses baked in)"""
        if key == self._ws_key:
            return True
        if key in self._ws_cache:
            self.ws, self.geo = self._ws_cache[key]
            self._ws_key = key
            return True
        return False

    def _publish(self, w: dict, key: tuple, geo: tuple, rope_key: tuple, rope_fn) -> None:
        """make w the current workspace and cache it; rope_fn() -> the (cos, sin) tables of rope_key if they are not built yet"""
        self.ws, self._ws_key, self.geo = w, key, geo
        if len(self._ws_cache) >= 8:  # bound the cache: drop the oldest shape (its graphs are dropped by the module too)
            self._ws_cache.pop(next(iter(self._ws_cache)))
        self._ws_cache[key] = (w, geo)
        if rope_key not in self._rope:
            c, s = rope_fn()
            self._rope[rope_key] = (c.to(self.dev), s.to(self.dev))

    def _cond_buffers(self, w: dict, B: int, H: int, W: int, train: bool, grouped: bool) -> None:
        """stem, conditioning path and head of a B x H x W batch.  grouped: the block weight gradients run as atomics-free grouped
        launches (dl_gemm_tn_group) through the partial slabs of ws["tn_slab"]"""
        d, z, f32 = self.d, self._z, torch.float32
        D, E, p = d.inner_dim, d.embedding_dim, d.patch_size
        M, Bp, Fo, R = B * (H // p) * (W // p), _rup(B, 64), p * p * d.output_channels, self.layout.mod_rows
        w["tokP"] = z(M, self._ki)  # patchified input, K padded to 64
        w["temb"], w["pre1"], w["h1"] = z(Bp, d.frequency_embedding), z(Bp, E), z(Bp, E)
        w["e"], w["emb"], w["se"] = z(Bp, E, dtype=f32), z(Bp, E, dtype=f32), z(Bp, E)
        w["mod"] = z(Bp, R)
        if self._pooled_dim:  # mlp_pooled_context: zero-padded input, hidden pre-activation / activation, f32 output
            w["poolP"], w["ppre1"], w["ph1"], w["pe"] = z(Bp, _rup(self._pooled_dim, 64)), z(Bp, 2 * E), z(Bp, 2 * E), z(Bp, E, dtype=f32)
            if train:
                w["dph1"], w["dppre1"] = z(Bp, 2 * E, dtype=f32), z(Bp, 2 * E)
        w["meanf"], w["rstdf"], w["xf"] = z(M, dtype=f32), z(M, dtype=f32), z(M, D)
        w["otok"] = z(M, _rup(Fo, 8), dtype=f32)
        w["pred"] = z(B, d.output_channels, H, W, dtype=f32)
        if not train:
            return
        w["dO"] = z(M, self._ko)
        w["dmod"] = z(Bp, R)                  # bf16 operand of the modulation GEMMs' backward
        w["dmod32"] = z(Bp, R, dtype=f32)     # f32 accumulator the block kernels add into
        w["dse"], w["demb"], w["demb16"] = z(Bp, E, dtype=f32), z(Bp, E, dtype=f32), z(Bp, E)
        w["dh1"], w["dpre1"] = z(Bp, E, dtype=f32), z(Bp, E)
        w["scr_last"], w["scr_conv"] = z(_rup(Fo, 8), D, dtype=f32), z(D, self._ki, dtype=f32)
        # scratch of the bit-reproducible small GEMMs / column sums of the head and the conditioning path (partial images per split,
        # folded in a fixed order: ops.gemm_tn / gemm_nt / colsum with scratch=): two images of the stacked adaLN weight gradient is
        # the largest user
        w["det_scr"] = torch.empty(max(2 * R * E, 1 << 22), device=self.dev, dtype=f32)
        # partial slabs of the grouped weight-gradient launch (the linears of a block in one atomics-free launch): 8 token ranges
        # (fewer above D = 1024) x (4 + 3 mlp_ratio) D^2 floats; one set, the side stream runs the blocks one after the other
        if grouped:
            w["tn_slab"] = torch.empty(ops.WgradGroups.slab_floats(D, d.mlp_ratio * D), device=self.dev, dtype=f32)

    def _grouped_widths(self) -> bool:
        """the linears of a block are whole tiles of the grouped weight-gradient launch (ops.WgradGroups); DL_WGRAD_GROUP=0 is the
        A/B switch back to one atomic launch per linear"""
        return ops.WgradGroups.widths_ok(self.d.inner_dim, self.d.mlp_ratio * self.d.inner_dim) and tuning.on("DL_WGRAD_GROUP")

    def _dit_block_buffers(self, B: int, nt: int, train: bool, nq: int | None = None) -> dict:
        """what a DiT block of a staged engine (SPRINT, DDT) keeps of its forward over B * nt tokens; q / k / v / lse hold nq >= nt
        rows per (sample, head) (padded attention).  Training adds the inputs of the weight-gradient GEMMs (wg)."""
        d, z, f32 = self.d, self._z, torch.float32
        D, Hh, F, mt = d.inner_dim, d.num_heads, d.mlp_ratio * d.inner_dim, B * nt
        nq = nt if nq is None else nq
        a = {"x0": z(mt, D), "mean1": z(mt, dtype=f32), "rstd1": z(mt, dtype=f32), "xm1": z(mt, D), "qkv": z(mt, 3 * D),
             "q": z(B, Hh, nq, 64), "k": z(B, Hh, nq, 64), "v": z(B, Hh, nq, 64), "rrms": z(mt, 2, dtype=f32), "a": z(mt, D),
             "lse": z(B, Hh, nq, dtype=f32), "t1": z(mt, D), "x1": z(mt, D), "mean2": z(mt, dtype=f32), "rstd2": z(mt, dtype=f32),
             "xm2": z(mt, D), "u": ops.mlp_u_buffer(z, mt, D, F, train), "h": z(mt, F), "t2": z(mt, D)}
        if train:
            a["wg"] = {"dt2": z(mt, D), "du": z(mt, 2 * F), "dt1": z(mt, D), "dqkv": z(mt, 3 * D)}
        return a

    def _joint_stream_buffers(self, B: int, nt: int, train: bool) -> dict:
        """what one token stream of a joint (MMDiT) block keeps of its forward over B * nt tokens (row buffers: a stream's token count
        need not be a multiple of 64)"""
        d, zr, f32 = self.d, self._zr, torch.float32
        D, F, mt = d.inner_dim, d.mlp_ratio * d.inner_dim, B * nt
        a = {"x0": zr(mt, D), "mean1": zr(mt, dtype=f32), "rstd1": zr(mt, dtype=f32), "xm1": zr(mt, D), "qkv": zr(mt, 3 * D),
             "rrms": zr(mt, 2, dtype=f32), "a": zr(mt, D), "t1": zr(mt, D), "x1": zr(mt, D), "mean2": zr(mt, dtype=f32),
             "rstd2": zr(mt, dtype=f32), "xm2": zr(mt, D), "u": ops.mlp_u_buffer(zr, mt, D, F, train), "h": zr(mt, F), "t2": zr(mt, D)}
        if train:
            a["wg"] = {"dt2": zr(mt, D), "du": zr(mt, 2 * F), "dt1": zr(mt, D), "dqkv": zr(mt, 3 * D)}
            a["dwb"] = self._z(2, B, 2, D, dtype=f32)
        return a

    def _single_stream_buffers(self, B: int, T: int, train: bool) -> dict:
        """what a single-stream (MMDiTSingleStreamBlock) block keeps of its forward over the B * T concatenated tokens"""
        d, zr, f32 = self.d, self._zr, torch.float32
        D, F, mt = d.inner_dim, d.mlp_ratio * d.inner_dim, B * T
        a = {"x0": zr(mt, D), "mean": zr(mt, dtype=f32), "rstd": zr(mt, dtype=f32), "m": zr(mt, D), "qkv": zr(mt, 3 * D),
             "rrms": zr(mt, 2, dtype=f32), "a": zr(mt, D), "ta": zr(mt, D), "u": ops.mlp_u_buffer(zr, mt, D, F, train), "h": zr(mt, F),
             "t": zr(mt, D)}
        if train:
            a["wg"] = {"dt": zr(mt, D), "du": zr(mt, 2 * F), "dqkv": zr(mt, 3 * D)}
            a["dwb"] = self._z(1, B, 2, D, dtype=f32)
        return a

    def _joint_attn_buffers(self, B: int, Tp: int) -> dict:
        """q / k / v, output and log-sum-exp of an attention over Tp (padded) joint tokens per sample"""
        z, Hh = self._z, self.d.num_heads
        return {"ao": z(B * Tp, self.d.inner_dim), "lse": z(B, Hh, Tp, dtype=torch.float32), "q": z(B, Hh, Tp, 64),
                "k": z(B, Hh, Tp, 64), "v": z(B, Hh, Tp, 64)}

    def _alloc(self, B: int, H: int, W: int, train: bool) -> None:
        key = (B, H, W, train)
        if self._cached(key):
            return
        d, z = self.d, self._z
        D, p, L = d.inner_dim, d.patch_size, d.depth
        gh, gw = H // p, W // p
        N = gh * gw
        M = B * N
        # token grids the attention kernels do not take as they are (not a multiple of 64 up to 256 / of 256 beyond: non-square and
        # multi-aspect-ratio latents): q / k / v rows padded to a multiple of 256 per (sample, head), pad keys masked (dl_attn_*_ex)
        pad = ops.attn_needs_padding(N)
        Nd = _rup(N, 256) if pad else N
        if pad and type(self) is DiTEngine and Nd <= ops.ATTN_MAX_TOKENS and M % 64:
            raise NotImplementedError(f"token grid {gh}x{gw} ({N} tokens) in the bf16 regime: batch * tokens must be a multiple of 64 (got "
                                      f"{B} * {N}); the fp32 regime (precision_type=\"no\" / set_precision(\"fp32\")) takes any grid and batch")
        if Nd > ops.ATTN_MAX_TOKENS or (pad and type(self) is not DiTEngine):
            raise NotImplementedError(f"token grid {gh}x{gw}: the bf16 regime's attention takes up to {ops.ATTN_MAX_TOKENS} tokens"
                                      + ("" if type(self) is DiTEngine else ", N % 64 == 0 up to 256 or N % 256 == 0 beyond, in this engine")
                                      + f" (got {N}); the fp32 regime (precision_type=\"no\" / set_precision(\"fp32\")) takes any grid")
        Bp = _rup(B, 64)
        Fo = p * p * d.output_channels
        ops.check_row_extent(B * Nd, max(2 * d.mlp_ratio * D, 6 * D), "DiT bf16 path")
        f32 = torch.float32
        w: dict[str, object] = {}
        self._cond_buffers(w, B, H, W, train, train and self._grouped_wgrad(M))
        nl = L if train else 1                    # inference reuses one block's buffers for every layer
        # MLP backward with recomputed pre-activations (csrc/mlp_bwd.hip): the training forward then stores h only and no
        # [M, 2F] pre-activation buffer exists (403 MB per block at B = 256); shapes without that kernel keep u
        F_ = d.mlp_ratio * D
        rc_u = train and type(self) is DiTEngine and ops.mlp_recompute_ok(M, D, F_)
        w["mlp_recompute"] = rc_u
        w["x"] = [z(M, D) for _ in range((L + 1) if train else 2)]
        per = []
        for _ in range(nl):
            per.append({
                "mean1": z(M, dtype=f32), "rstd1": z(M, dtype=f32), "xm1": z(M, D), "qkv": z(M, 3 * D),
                "q": z(B, d.num_heads, Nd, 64), "k": z(B, d.num_heads, Nd, 64),
                "v": None if ops.v_in_place(N) else z(B, d.num_heads, Nd, 64),  # (N <= 256: V is read in place from qkv)
                "ao": z(B * Nd, D) if pad else None,
                "rrms": z(M, 2, dtype=f32), "a": z(M, D), "lse": z(B, d.num_heads, Nd, dtype=f32), "t1": z(M, D),
                "x1": z(M, D), "mean2": z(M, dtype=f32), "rstd2": z(M, dtype=f32), "xm2": z(M, D),
                "u": None if rc_u else z(M, 2 * d.mlp_ratio * D), "h": z(M, d.mlp_ratio * D), "t2": z(M, D),
            })
        w["layers"] = per
        # QK-norm on load (dl_gemm_nt_ssq + dl_attn_fwd_qkn): per-block sums of squares of the q / k rows, zeroed once per forward (one
        # buffer per block also in inference: the GEMM epilogues ADD into it)
        if pad:
            w["kb"] = z(B, Nd, dtype=f32)
            w["kb"][:, N:] = float("-inf")
        if self._qkn_on_load(M, N):
            w["ssq_all"] = z(L, M, 2, dtype=f32)
        if train:
            w["dxa"], w["dxb"] = z(M, D), z(M, D)
            w["dxm"], w["da"] = z(M, D), z(M, D)
            w["dh"] = z(M, d.mlp_ratio * D)
            # per-block inputs of the weight-gradient GEMMs (consumed asynchronously on the side stream)
            w["wg"] = [{"dt2": z(M, D), "du": z(M, 2 * d.mlp_ratio * D), "dt1": z(M, D), "dqkv": z(M, 3 * D)}
                       for _ in range(L)]
            # N <= 256 and D <= 512: dQ / dK / dV leave the attention backward token-major inside the dqkv rows and the QK-norm
            # backward works in place (its per-workgroup scale-gradient partials land in qk_part): no dq / dk buffers
            # (from 32768 token rows: at the CIFAR config's 8192 rows the in-place pair is 5 % of a 6.7 ms step SLOWER)
            if ops.v_in_place(N) and D <= 512 and M >= 32768 and type(self) is DiTEngine and tuning.on("DL_QK_INPLACE"):
                w["qk_part"] = torch.empty(1024 * 2 * D, device=self.dev, dtype=f32)
                w["dq"] = w["dk"] = None
            else:
                w["dq"], w["dk"] = z(B, d.num_heads, Nd, 64), z(B, d.num_heads, Nd, 64)
            w["dv"] = None if ops.v_in_place(N) else z(B, d.num_heads, Nd, 64)
            if pad:
                w["dao"] = z(B * Nd, D)
            w["dwb"] = z(2 * L, B, 2, D, dtype=f32)  # per-norm partials: folded on the side stream, cleared while read
        self._publish(w, key, (B, H, W, gh, gw, N, M, Bp, Fo), (gh, gw), lambda: rope_grid_tables(gh, gw, d.rope_axes_dim, d.rope_base))

    def _stem_fwd(self, x: Tensor, t: Tensor, y_eff: Tensor | None, x0: Tensor | None = None, patch_gemm: bool = True) -> Tensor:
        """patch embedding into ``x0`` (default ws["x"][0]) and the conditioning path: time MLP (+ label row) -> SiLU -> the
        stacked adaLN GEMM of every block and of the last layer.  Returns the modulation matrix bf16 [Bp, mod_rows].
        patch_gemm=False leaves the patch-embedding GEMM to the caller (row-complete path: it needs the modulation rows)."""
        d, w, sh = self.d, self.ws, self.sh
        B, _, _, _, _, _, M, _, _ = self.geo
        D, E = d.inner_dim, d.embedding_dim
        ops.patchify(x, w["tokP"], d.patch_size, ops.PATCH_CPP)
        if patch_gemm:
            ops.gemm_nt(w["tokP"], sh[self._conv_name + "|f"], w["x"][0] if x0 is None else x0, M=M, N=D, K=self._ki)
        ops.timestep_embedding(t, w["temb"][:B])
        ops.gemm_nt(w["temb"], sh["time_embed.0.weight|f"], w["h1"], bias=self.P("time_embed.0.bias"), act=ops.ACT_SILU,
                    pre_out=w["pre1"], M=B, N=E, K=d.frequency_embedding)
        ops.gemm_nt(w["h1"], sh["time_embed.2.weight|f"], w["e"], bias=self.P("time_embed.2.bias"), M=B, N=E, K=E)
        if self._pooled_dim:
            self._pooled_fwd(B)
        else:
            table = self.P("label_embed.embedding.weight") if d.n_classes is not None else None
            ops.cond_combine_fwd(w["e"][:B], table, y_eff if table is not None else None, w["emb"][:B], w["se"][:B])
        mod_bias = self.params[self.layout.entries[self.layout.mod_b0][0] :][: self.layout.mod_rows]
        ops.gemm_nt(w["se"], sh["@mod|f"], w["mod"], bias=mod_bias, M=B, N=self.layout.mod_rows, K=E)
        return w["mod"]

    def _pooled_fwd(self, B: int) -> None:
        """emb = mlp_pooled_context(pooled) + time embedding (mmdit.py:800-806) and its SiLU: the two linears as small-M GEMMs like
        the time MLP's, the add and the SiLU in the dense combine kernel"""
        d, w, sh = self.d, self.ws, self.sh
        E, P = d.embedding_dim, self._pooled_dim
        pooled = self.pooled
        assert pooled is not None and tuple(pooled.shape) == (B, P), "pooled context embedding [B, pooled_dim] not set for this step"
        w["poolP"][:B, :P].copy_(pooled)
        ops.gemm_nt(w["poolP"], sh["mlp_pooled_context.0.weight|f"], w["ph1"], bias=self.P("mlp_pooled_context.0.bias"), act=ops.ACT_SILU,
                    pre_out=w["ppre1"], M=B, N=2 * E, K=w["poolP"].shape[1])
        ops.gemm_nt(w["ph1"], sh["mlp_pooled_context.2.weight|f"], w["pe"], bias=self.P("mlp_pooled_context.2.bias"), M=B, N=E, K=2 * E)
        ops.cond_combine_dense_fwd(w["e"][:B], w["pe"][:B], w["emb"][:B], w["se"][:B])

    def _pooled_bwd(self, B: int, det: Tensor | None) -> None:
        """backward of mlp_pooled_context from ws["demb"] / ws["demb16"] (the gradient of the combined embedding), gradients into
        the arena through the same small GEMMs / column sums as the time MLP's"""
        d, w, sh = self.d, self.ws, self.sh
        E, P = d.embedding_dim, self._pooled_dim
        ops.colsum(w["demb"], self.G("mlp_pooled_context.2.bias"), B, E, scratch=det)
        ops.gemm_tn(w["demb16"], w["ph1"], self.G("mlp_pooled_context.2.weight"), scratch=det)
        ops.gemm_nt(w["demb16"], sh["mlp_pooled_context.2.weight|t"], w["dph1"], M=B, N=2 * E, K=E)
        ops.silu_bwd(w["dph1"][:B], w["ppre1"][:B], w["dppre1"][:B])
        ops.gemm_tn(w["dppre1"], w["poolP"], self.G("mlp_pooled_context.0.weight"), M=2 * E, N=P, scratch=det)
        ops.colsum(w["dppre1"], self.G("mlp_pooled_context.0.bias"), B, 2 * E, scratch=det)

    def _main_wgs(self) -> int:
        """workgroup budget of the persistent main-chain kernels (0 = one per CU).  DL_DP_RESERVE_CUS = r > 0: with a gradient reducer
        attached the grids leave r compute units to RCCL's channel workgroups.  Measured with the stand-in of scripts/lab/occupied_cus.py
        (round 4): the headline shape's tile counts are whole multiples of 256, so 248 workgroups run an extra, nearly empty round --
        20.7 -> 24.1 ms per step WITHOUT any foreign workgroup, 26.2 vs 24.6 ms with 16 of them resident for half the step -- a loss;
        the shipped default is therefore 0 and the reducer's measured choice between overlapped buckets and one exchange after the
        backward (training/dp.py) stays the mechanism."""
        explicit = tuning.integer("DL_MAIN_WGS", 0)
        if explicit:
            return explicit
        reserve = tuning.integer("DL_DP_RESERVE_CUS", 0)
        if reserve and self.reducer is not None and getattr(self.reducer, "enabled", True):
            if getattr(self, "_cus", None) is None:
                self._cus = torch.cuda.get_device_properties(self.dev).multi_processor_count
            return max(8, (self._cus - reserve) & ~7)
        return 0

    # ------------------------------------------------------------------ native block driver (csrc/block.hip)
    def _native_blocks(self) -> bool:
        """one C call per block and direction (dl_dit_block_fwd / _bwd) instead of ~25 launches from Python; DL_NATIVE_BLOCK=0 is the
        A/B switch back to the Python-issued sequence (identical kernels, identical order)"""
        return type(self) is DiTEngine and tuning.on("DL_NATIVE_BLOCK") and not (self.geo is not None and ops.attn_needs_padding(self.geo[5]))

    def _block_args(self, i: int, train: bool):
        """the dl_dit_block_t of block i on the current workspace (cached: every pointer is fixed once arena and workspace exist)"""
        key = (self._ws_key, i, self.reducer is None, self._main_wgs())
        blk = self._blk_cache.get(key)
        if blk is not None:
            return blk
        from ._block import DitBlock

        d, w, sh = self.d, self.ws, self.sh
        B, _, _, gh, gw, N, M, Bp, Fo = self.geo
        D, L, F = d.inner_dim, d.depth, d.mlp_ratio * d.inner_dim
        pre, mo = f"layers.{i}.", i * 6 * D
        mod, xs = w["mod"], w["x"]
        a = w["layers"][i if train else 0]
        xin = xs[i] if train else xs[i & 1]
        cos, sin = self._rope[(gh, gw)]
        mrow = lambda off: mod.data_ptr() + 2 * off  # noqa: E731  (row view mod[:, off:]: bf16)
        blk = DitBlock()
        blk.B, blk.N, blk.D, blk.H, blk.F = B, N, D, d.num_heads, F
        blk.ld_mod = mod.stride(0)
        blk.ldw_d, blk.ldw_f = sh[pre + "attention.qkv.weight|f"].stride(0), sh[pre + "mlp_input.2.weight|f"].stride(0)
        blk.ldwt_d, blk.ldwt_f2 = sh[pre + "attention.proj_out.weight|t"].stride(0), sh[pre + "mlp_input.0.weight|t"].stride(0)
        blk.ldwt_3d = sh[pre + "attention.qkv.weight|t"].stride(0)
        blk.rot, blk.eps = sum(d.rope_axes_dim), 1e-5
        blk.max_workgroups = self._main_wgs()
        prev = None
        if i > 0:
            ap = w["layers"][(i - 1) if train else 0]
            prev = (ap["x1"], ap["t2"], mrow((i - 1) * 6 * D + 5 * D))
        blk.set(x_in=xin, pend_x=prev[0] if prev else None, pend_t=prev[1] if prev else None, pend_gate=prev[2] if prev else None,
                scale1=mrow(mo), shift1=mrow(mo + D), gate1=mrow(mo + 2 * D), scale2=mrow(mo + 3 * D), shift2=mrow(mo + 4 * D),
                gate2=mrow(mo + 5 * D),
                ln1_w=self.P(pre + "norm_1.weight"), ln1_b=self.P(pre + "norm_1.bias"), ln2_w=self.P(pre + "norm_2.weight"),
                ln2_b=self.P(pre + "norm_2.bias"), qn_scale=self.P(pre + "attention.qk_norm.query_norm.scale"),
                kn_scale=self.P(pre + "attention.qk_norm.key_norm.scale"),
                w_qkv=sh[pre + "attention.qkv.weight|f"], w_proj=sh[pre + "attention.proj_out.weight|f"],
                w_up=sh[pre + "mlp_input.0.weight|f"], w_up_perm=sh[pre + "mlp_input.0.weight|g"], w_down=sh[pre + "mlp_input.2.weight|f"],
                wt_qkv=sh[pre + "attention.qkv.weight|t"], wt_proj=sh[pre + "attention.proj_out.weight|t"],
                wt_up=sh[pre + "mlp_input.0.weight|t"], wt_down=sh[pre + "mlp_input.2.weight|t"], rope_cos=cos, rope_sin=sin,
                xm1=a["xm1"], mean1=a["mean1"], rstd1=a["rstd1"], qkv=a["qkv"], q=a["q"], k=a["k"], v=a["v"], rrms=a["rrms"], a=a["a"],
                lse=a["lse"], t1=a["t1"], x1=a["x1"], xm2=a["xm2"], mean2=a["mean2"], rstd2=a["rstd2"], u=a["u"], h=a["h"], t2=a["t2"],
                ssq=w["ssq_all"][i] if "ssq_all" in w else None)
        rows = self._row_gemms(M, N)
        blk.row_gemms = 0
        if rows:
            if i + 1 < L:
                nx, mn, nxt = w["layers"][(i + 1) if train else 0], (i + 1) * 6 * D, f"layers.{i + 1}."
                lnw, lnb, blk.next_eps = self.P(nxt + "norm_1.weight"), self.P(nxt + "norm_1.bias"), 1e-5
                xm_n, mu_n, rs_n = nx["xm1"], nx["mean1"], nx["rstd1"]
            else:
                mn, lnw, lnb, blk.next_eps = L * 6 * D, None, None, 1e-6
                xm_n, mu_n, rs_n = w["xf"], w["meanf"], w["rstdf"]
            blk.set(next_ln_w=lnw, next_ln_b=lnb, next_scale=mrow(mn), next_shift=mrow(mn + D),
                    next_x=xs[i + 1] if train else xs[(i + 1) & 1], next_xm=xm_n, next_mean=mu_n, next_rstd=rs_n)
            # bit 1: QK-norm + RoPE in the qkv epilogue (measured slightly slower inside the step: opt-in); bit 2: the LayerNorm-affine
            # partials of all blocks are folded by ONE launch at the end of the backward (not with a gradient reducer attached: it
            # wants every block's range final as soon as the block is done)
            # bit 3: the forward as one per-sample chain launch where the library serves the block that way (csrc/block_fused.hip)
            blk.row_gemms = (1 | (2 if tuning.on("DL_ROW_GEMM_QK") else 0) | (4 if self.reducer is None else 0)
                             | (8 if tuning.on("DL_BLOCK_CHAIN") else 0))
        if train and self.grads is not None:
            g, dmod = w["wg"][i], w["dmod32"]
            blk.ld_dmod = dmod.stride(0)
            drow = lambda off: dmod.data_ptr() + 4 * off  # noqa: E731
            pg = None
            if i > 0:
                mp = (i - 1) * 6 * D
                pg = (w["layers"][i - 1]["t2"], mrow(mp + 5 * D), w["wg"][i - 1]["dt2"], drow(mp + 5 * D))
            blk.set(dt2=g["dt2"], dx_in=w["dxa"], dx_mid=w["dxb"], dx_out=w["dxa"], dh=w["dh"], du=g["du"], dxm=w["dxm"], dt1=g["dt1"],
                    da=w["da"], dq=w["dq"], dk=w["dk"], dv=w["dv"], dqkv=g["dqkv"], dfeat=None,
                    dscale1=drow(mo), dshift1=drow(mo + D), dgate1=drow(mo + 2 * D), dscale2=drow(mo + 3 * D), dshift2=drow(mo + 4 * D),
                    dwb1=w["dwb"][2 * i], dwb2=w["dwb"][2 * i + 1],
                    prev_t2=pg[0] if pg else None, prev_gate2=pg[1] if pg else None, prev_dt2=pg[2] if pg else None,
                    prev_dgate2=pg[3] if pg else None,
                    g_qkv=self.G(pre + "attention.qkv.weight"), g_proj=self.G(pre + "attention.proj_out.weight"),
                    g_up=self.G(pre + "mlp_input.0.weight"), g_down=self.G(pre + "mlp_input.2.weight"),
                    g_ln1=self.G(pre + "norm_1.weight"), g_ln2=self.G(pre + "norm_2.weight"),
                    g_qk_scale=self.G(pre + "attention.qk_norm.query_norm.scale"), tn_slab=w.get("tn_slab"),
                    qk_partials=w.get("qk_part"))
            blk.tn_slab_floats = w["tn_slab"].numel() if "tn_slab" in w else 0
        self._blk_cache[key] = blk
        return blk

    # ------------------------------------------------------------------ forward
    def forward(self, x: Tensor, t: Tensor, y_eff: Tensor | None, train: bool = True, refresh: bool = True) -> Tensor:
        """x f32 [B,C,H,W]; t f32 [B] (flow: in [0,1]; ddpm: indices as floats, both fed unscaled like the
        reference); y_eff int64 [B] labels AFTER the classifier-free drop, or None.  Returns pred f32 [B,Co,H,W]
        (a workspace buffer: consume it before the next forward)."""
        d = self.d
        B, C, H, W = x.shape
        assert C == d.input_channels and x.dtype == torch.float32 and x.is_cuda
        self._alloc(B, H, W, train)
        if refresh:  # (False while a hipGraph of this forward is being captured: the replay path refreshes eagerly)
            self.refresh_shadows(force=train)  # a training forward always follows a parameter update
        w, sh = self.ws, self.sh
        _, _, _, gh, gw, N, M, _, _ = self.geo
        D, L = d.inner_dim, d.depth
        cos, sin = self._rope[(gh, gw)]
        self._train = train
        self._yeff = y_eff

        fused = self._row_gemms(M, N)
        if "ssq_all" in w:
            w["ssq_all"].zero_()
        mod = self._stem_fwd(x, t, y_eff, patch_gemm=not fused)
        xs = w["x"]
        if fused:
            if self._native_blocks():
                a0 = w["layers"][0]
                _must(ops.ln_modulate_gemm_fwd(w["tokP"], sh[self._conv_name + "|f"], None, None, self.P("layers.0.norm_1.weight"),
                                               self.P("layers.0.norm_1.bias"), mod[:, 0:D], mod[:, D : 2 * D], N, 1e-5, None, xs[0],
                                               a0["xm1"], a0["mean1"], a0["rstd1"], K=self._ki))
                for i in range(L):
                    ops.dit_block_fwd(self._block_args(i, train), train)
            else:
                self._forward_row_gemms(mod, train)
            return self._head_fwd(None, w["xf"])

        pend = None  # (x_base, t, gate) of the sub-layer whose residual add is still pending (_half1_fwd)
        native = self._native_blocks()
        for i in range(L):
            a = w["layers"][i if train else 0]
            if native:
                ops.dit_block_fwd(self._block_args(i, train), train)
                pend = (a["x1"], a["t2"], mod[:, i * 6 * D + 5 * D : i * 6 * D + 6 * D])
                continue
            pend = self._dit_block_fwd(a, f"layers.{i}.", xs[i] if train else xs[i & 1], pend, Modulation(mod, None, i * 6 * D, D, N), N,
                                       cos, sin, kb=w.get("kb"))
        return self._head_fwd(Modulation(mod, None, L * 6 * D, D, N), xs[L] if train else xs[L & 1], pend)

    # ------------------------------------------------------------------ block launch sequences (every bf16 transformer engine)
    def _half1_fwd(self, a: dict, nm: dict, xin: Tensor, pend: tuple | None, m: Modulation, nt: int, cos: Tensor, sin: Tensor,
                   q: Tensor, k: Tensor, v: Tensor | None, pos: Tensor | None = None, n_off: int = 0) -> None:
        """first half of a DiT block, or of one token stream of a joint block (nm: block_names), over nt tokens per sample:
        LayerNorm-modulate -> qkv GEMM -> QK-norm + RoPE + head split into rows [n_off, n_off + nt) of q / k / v.
        The gated residual of every sub-layer (x += gate * f(...)) is applied by the NEXT LayerNorm-modulate kernel, which has to read
        the residual stream anyway: the projection / MLP-down GEMMs stay plain stores (fast 256x384 tiles) and write t1 / t2, which
        the backward needs for the gate gradients.  pend = (x_base, t, gate) of that pending add (its sum is written to xin), or
        None: xin holds the block input"""
        n1w, n1b = self.P(nm["n1"] + ".weight"), self.P(nm["n1"] + ".bias")
        if pend is None:
            ops.ln_modulate_fwd(xin, n1w, n1b, m.col(0), m.col(1), m.rows, 1e-5, a["xm1"], a["mean1"], a["rstd1"])
        else:
            ops.ln_modulate_fwd(pend[0], n1w, n1b, m.col(0), m.col(1), m.rows, 1e-5, a["xm1"], a["mean1"], a["rstd1"], t=pend[1],
                                gate=pend[2], x_out=xin)
        ops.gemm_nt(a["xm1"], self.sh[nm["qkv"] + ".weight|f"], a["qkv"])
        ops.qk_norm_rope_fwd(a["qkv"], self.P(nm["qk"] + ".query_norm.scale"), self.P(nm["qk"] + ".key_norm.scale"), cos, sin, q, k, v,
                             a["rrms"], self.geo[0], nt, self.d.num_heads, 64, sum(self.d.rope_axes_dim), pos=pos, n_off=n_off)

    def _half2_fwd(self, a: dict, nm: dict, xin: Tensor, m: Modulation) -> tuple:
        """second half: attention output a["a"] -> projection -> LayerNorm-modulate (with the gated residual of the attention branch,
        x1 = xin + gate1 * t1) -> SwiGLU MLP.  Returns the pending residual (x1, t2, gate2) for the next LayerNorm"""
        sh = self.sh
        ops.gemm_nt(a["a"], sh[nm["proj"] + ".weight|f"], a["t1"])
        ops.ln_modulate_fwd(xin, self.P(nm["n2"] + ".weight"), self.P(nm["n2"] + ".bias"), m.col(3), m.col(4), m.rows, 1e-5, a["xm2"],
                            a["mean2"], a["rstd2"], t=a["t1"], gate=m.col(2), x_out=a["x1"])
        u = a["u"] if self._train else None  # (stationary: the h-only launch takes the panel-in-registers kernel, csrc/gemm_stationary.hip)
        if not ops.gemm_nt_swiglu(a["xm2"], sh[nm["up"] + ".weight|g"], u, a["h"], stationary=u is None):
            assert a["u"] is not None, "the recompute mode is only chosen for shapes the fused MLP-up kernel serves"
            ops.gemm_nt(a["xm2"], sh[nm["up"] + ".weight|f"], a["u"])  # small / ragged shapes: unfused pair
            ops.swiglu_fwd(a["u"], a["h"])
        ops.gemm_nt(a["h"], sh[nm["down"] + ".weight|f"], a["t2"])
        return a["x1"], a["t2"], m.col(5)

    def _attn_fwd(self, a: dict, nt: int, kb: Tensor | None) -> None:
        """self-attention of a DiT block over nt tokens per sample, in the form the block has buffers for"""
        B, Hh, D = self.geo[0], self.d.num_heads, self.d.inner_dim
        if a.get("ao") is not None:  # token grids the kernels do not take as they are (multi-aspect-ratio buckets: 28 x 36, 24 x 40
            # ...): q / k / v live in rows padded to a multiple of 256 per (sample, head); the pad keys are masked through the key
            # bias kb, the pad queries' outputs never copied out
            Np = a["q"].shape[2]
            ops.attn_fwd_ex(a["q"], a["k"], a["v"], a["ao"], a["lse"], B, Hh, Np, Np, 64, 64**-0.5, kb)
            ops.copy_rows3d(a["ao"], Np * D, D, a["a"], nt * D, D, B, nt, D)
        elif ops.v_in_place(nt):  # up to 256 tokens the kernels address V (and dV) inside the token-major qkv (dqkv) rows
            ops.attn_fwd_qkv(a["q"], a["k"], a["qkv"], a["a"], a["lse"], B, Hh, nt, 64, 64**-0.5)
        else:
            ops.attn_fwd(a["q"], a["k"], a["v"], a["a"], a["lse"], B, Hh, nt, 64, 64**-0.5)

    def _dit_block_fwd(self, a: dict, pre: str, xin: Tensor, pend: tuple | None, m: Modulation, nt: int, cos: Tensor, sin: Tensor,
                       pos: Tensor | None = None, kb: Tensor | None = None) -> tuple:
        """one adaLN-zero DiT block `pre` issued from Python on the buffers a; pos: RoPE table row of every token (None: its index in
        the sequence); kb: key bias of the padded attention.  Returns the pending residual of its MLP branch"""
        nm = block_names(pre)
        self._half1_fwd(a, nm, xin, pend, m, nt, cos, sin, a["q"], a["k"], None if ops.v_in_place(nt) else a["v"], pos)
        self._attn_fwd(a, nt, kb)
        return self._half2_fwd(a, nm, xin, m)

    def _head_fwd(self, m: Modulation | None, x: Tensor, pend: tuple | None = None) -> Tensor:
        """final LayerNorm-modulate of x (pend: of the pending residual, whose sum is written to x; m None: ws["xf"] is already
        there) -> last linear -> unpatchify.  Returns ws["pred"]"""
        w = self.ws
        M, Fo = self.geo[6], self.geo[8]
        if m is not None and pend is None:
            ops.ln_modulate_fwd(x, None, None, m.col(0), m.col(1), m.rows, 1e-6, w["xf"], w["meanf"], w["rstdf"])
        elif m is not None:
            ops.ln_modulate_fwd(pend[0], None, None, m.col(0), m.col(1), m.rows, 1e-6, w["xf"], w["meanf"], w["rstdf"], t=pend[1],
                                gate=pend[2], x_out=x)
        ops.gemm_nt(w["xf"], self.sh["last_layer.linear.weight|f"], w["otok"], bias=self.P("last_layer.linear.bias"), M=M, N=Fo,
                    K=self.d.inner_dim)
        ops.unpatchify(w["otok"], w["pred"], self.d.patch_size)
        return w["pred"]

    def _half2_bwd(self, a: dict, g: dict, nm: dict, s: dict, m: Modulation, dx: Tensor | None, sw: "SideWork") -> Tensor:
        """backward of _half2_fwd.  g: the block's inputs of the weight-gradient GEMMs (g["dt2"] was produced by the LayerNorm
        backward before this one in the chain); s: chain scratch; dx: residual-stream gradient (None: zero so far).  Leaves the
        gradient of the attention output in s["da"] and returns the residual-stream gradient at x1's input"""
        sh = self.sh
        sw.wgrad(g["dt2"], a["h"], nm["down"] + ".weight")
        ops.mlp_swiglu_bwd(g["dt2"], sh[nm["down"] + ".weight|t"], a["xm2"], sh[nm["up"] + ".weight|g"], a["u"], s["dh"], g["du"])
        sw.wgrad(g["du"], a["xm2"], nm["up"] + ".weight")
        ops.gemm_nt(g["du"], sh[nm["up"] + ".weight|t"], s["dxm"])
        nx = _other(s, dx)
        m.ln_bwd(s["dxm"], a["x1"], self.P(nm["n2"] + ".weight"), self.P(nm["n2"] + ".bias"), 3, a["mean2"], a["rstd2"], dx, nx,
                 m.part[1], gate=(a["t1"], m.off + 2 * m.D, g["dt1"]))
        sw.fold(m.part[1], nm["n2"] + ".weight", m.groups)
        sw.wgrad(g["dt1"], a["a"], nm["proj"] + ".weight")
        ops.gemm_nt(g["dt1"], sh[nm["proj"] + ".weight|t"], s["da"])
        return nx

    def _half1_bwd(self, a: dict, g: dict, nm: dict, s: dict, m: Modulation, xin: Tensor, dx: Tensor | None, prev: tuple | None,
                   dres: Tensor | None, sw: "SideWork") -> Tensor:
        """backward of _half1_fwd from g["dqkv"] on.  xin: the block input; prev = (t2, column of gate2, dt2) of the block before in
        the chain, whose gated residual this LayerNorm absorbed (None: none did); dres: auxiliary-loss gradient on that block's
        output (= this block's input).  Returns the residual-stream gradient at the block input"""
        sw.wgrad(g["dqkv"], a["xm1"], nm["qkv"] + ".weight")
        ops.gemm_nt(g["dqkv"], self.sh[nm["qkv"] + ".weight|t"], s["dxm"])
        if dres is not None and dx is not None:
            ops.add_bf16(dx, dres, dx)
        nx = _other(s, dx)
        m.ln_bwd(s["dxm"], xin, self.P(nm["n1"] + ".weight"), self.P(nm["n1"] + ".bias"), 0, a["mean1"], a["rstd1"], dx, nx, m.part[0],
                 gate=prev)
        sw.fold(m.part[0], nm["n1"] + ".weight", m.groups)
        return nx

    def _attn_bwd(self, a: dict, g: dict, nm: dict, s: dict, nt: int, cos: Tensor, sin: Tensor, pos: Tensor | None,
                  kb: Tensor | None, dao: Tensor | None) -> None:
        """s["da"] -> g["dqkv"]: backward of _attn_fwd and of QK-norm + RoPE.  dao: padded copy of da (padded attention)"""
        w = self.ws
        B, Hh, D, rot = self.geo[0], self.d.num_heads, self.d.inner_dim, sum(self.d.rope_axes_dim)
        sq, sk = self.P(nm["qk"] + ".query_norm.scale"), self.P(nm["qk"] + ".key_norm.scale")
        dscale = self._qk_scale_sink(nm["qk"]) if self._input_only else self.G(nm["qk"] + ".query_norm.scale")
        if ops.qk_inplace_ok(w, B, nt):  # dQ, dK, dV token-major into dqkv; the QK-norm backward transforms the q / k thirds in place
            ops.attn_bwd_tok(a["q"], a["k"], a["qkv"], a["a"], s["da"], a["lse"], g["dqkv"], B, Hh, nt, 64, 64**-0.5)
            _must(ops.qk_norm_rope_bwd_inplace(a["qkv"], sq, sk, cos, sin, a["rrms"], g["dqkv"], dscale, w["qk_part"], B, nt, Hh, 64, rot,
                                                pos=pos))
            return
        v_in_place = ops.v_in_place(nt)
        if a.get("ao") is not None:
            Np = a["q"].shape[2]
            ops.copy_rows3d(s["da"], nt * D, D, dao, Np * D, D, B, nt, D)  # (the pad rows of dao stay zero)
            ops.attn_bwd_ex(a["q"], a["k"], a["v"], a["ao"], dao, a["lse"], s["dq"], s["dk"], s["dv"], B, Hh, Np, Np, 64, 64**-0.5, kb)
        elif v_in_place:  # dV goes straight into the v third of dqkv
            ops.attn_bwd_qkv(a["q"], a["k"], a["qkv"], a["a"], s["da"], a["lse"], s["dq"], s["dk"], g["dqkv"], B, Hh, nt, 64, 64**-0.5)
        else:
            ops.attn_bwd(a["q"], a["k"], a["v"], a["a"], s["da"], a["lse"], s["dq"], s["dk"], s["dv"], B, Hh, nt, 64, 64**-0.5)
        ops.qk_norm_rope_bwd(s["dq"], s["dk"], None if v_in_place else s["dv"], a["qkv"], sq, sk, cos, sin, a["rrms"], g["dqkv"], dscale,
                             B, nt, Hh, 64, rot, pos=pos)

    def _dit_block_bwd(self, a: dict, g: dict, pre: str, xin: Tensor, dx: Tensor, prev: tuple | None, dres: Tensor | None, s: dict,
                       m: Modulation, nt: int, cos: Tensor, sin: Tensor, sw: "SideWork", pos: Tensor | None = None,
                       kb: Tensor | None = None, dao: Tensor | None = None) -> Tensor:
        """backward of _dit_block_fwd (arguments as in the halves): dx at the block output -> returned dx at the block input"""
        nm = block_names(pre)
        dx = self._half2_bwd(a, g, nm, s, m, dx, sw)
        self._attn_bwd(a, g, nm, s, nt, cos, sin, pos, kb, dao)
        return self._half1_bwd(a, g, nm, s, m, xin, dx, prev, dres, sw)

    def _grouped_wgrad(self, M: int) -> bool:
        """the four weight gradients of a block as ONE launch without atomics (csrc/gemm_w4.hip, dl_gemm_tn_group): every linear of
        the block must be a whole number of 384 x 192 tiles.  DL_WGRAD_GROUP=0 is the A/B switch back to four atomic launches."""
        D, F = self.d.inner_dim, self.d.mlp_ratio * self.d.inner_dim
        return (type(self) is DiTEngine and ops.WgradGroups.shapes_ok(D, F, M) and tuning.on("DL_WGRAD_GROUP"))

    def _qkn_on_load(self, M: int, N: int) -> bool:
        # (dl_gemm_nt_ssq runs the persistent 256 x 384 tiles: it wants >= 64 of them, i.e. 22 samples of 256 tokens at D = 384)
        return (self._row_gemms(M, N) and self.d.inner_dim % 384 == 0 and (M // 256) * (3 * self.d.inner_dim // 384) >= 64
                and tuning.on("DL_QKN_ON_LOAD") and not tuning.on("DL_ROW_GEMM_QK"))

    def _row_gemms(self, M: int, N: int) -> bool:
        """the row-complete GEMM path (csrc/gemm_ln.hip): LayerNorm-modulate forward / backward and QK-norm + RoPE run as epilogues
        of the GEMMs that feed them.  D == 384 with 256 tokens per sample (one 256 x 384 tile = one sample's whole rows)"""
        return type(self) is DiTEngine and ops.v_in_place(N) and ops.row_gemm_ok(M, self.d.inner_dim, N)

    def _forward_row_gemms(self, mod: Tensor, train: bool) -> None:
        """block chain of forward() with every LayerNorm-modulate in the epilogue of the GEMM in front of it: the patch embedding
        carries LN1 of block 0, the projection carries LN2 of its block, the MLP-down GEMM carries LN1 of the NEXT block (or the
        final LayerNorm); the qkv GEMM carries QK-norm + RoPE + the head split"""
        d, w, sh = self.d, self.ws, self.sh
        B, _, _, gh, gw, N, M, _, _ = self.geo
        D, L, Hh = d.inner_dim, d.depth, d.num_heads
        cos, sin = self._rope[(gh, gw)]
        rot = sum(d.rope_axes_dim)
        xs = w["x"]
        lay = lambda i: w["layers"][i if train else 0]  # noqa: E731
        xbuf = lambda i: xs[i] if train else xs[i & 1]  # noqa: E731
        fused_qk = tuning.on("DL_ROW_GEMM_QK")
        a0 = lay(0)
        _must(ops.ln_modulate_gemm_fwd(w["tokP"], sh[self._conv_name + "|f"], None, None, self.P("layers.0.norm_1.weight"),
                                        self.P("layers.0.norm_1.bias"), mod[:, 0:D], mod[:, D : 2 * D], N, 1e-5, None, xbuf(0),
                                        a0["xm1"], a0["mean1"], a0["rstd1"], K=self._ki))
        for i in range(L):
            a, xin, pre, mo = lay(i), xbuf(i), f"layers.{i}.", i * 6 * D
            if "ssq_all" in w:
                ssq = w["ssq_all"][i]
                _must(ops.gemm_nt_ssq(a["xm1"], sh[pre + "attention.qkv.weight|f"], a["qkv"], ssq, stationary=True))
                ops.attn_fwd_qkn(a["qkv"], ssq, self.P(pre + "attention.qk_norm.query_norm.scale"),
                                 self.P(pre + "attention.qk_norm.key_norm.scale"), cos, sin, a["q"] if train else None,
                                 a["k"] if train else None, a["rrms"] if train else None, a["a"], a["lse"], B, Hh, N, 64, rot, 64**-0.5)
            elif fused_qk:
                _must(ops.gemm_nt_qk_norm_rope(a["xm1"], sh[pre + "attention.qkv.weight|f"],
                                                self.P(pre + "attention.qk_norm.query_norm.scale"),
                                                self.P(pre + "attention.qk_norm.key_norm.scale"), cos, sin, a["qkv"], a["q"], a["k"],
                                                a["rrms"], B, N, Hh, 64, rot))
            else:
                ops.gemm_nt(a["xm1"], sh[pre + "attention.qkv.weight|f"], a["qkv"])
                ops.qk_norm_rope_fwd(a["qkv"], self.P(pre + "attention.qk_norm.query_norm.scale"),
                                     self.P(pre + "attention.qk_norm.key_norm.scale"), cos, sin, a["q"], a["k"], None, a["rrms"], B, N,
                                     Hh, 64, rot)
            if "ssq_all" not in w:
                ops.attn_fwd_qkv(a["q"], a["k"], a["qkv"], a["a"], a["lse"], B, Hh, N, 64, 64**-0.5)
            _must(ops.ln_modulate_gemm_fwd(a["a"], sh[pre + "attention.proj_out.weight|f"], xin, mod[:, mo + 2 * D : mo + 3 * D],
                                            self.P(pre + "norm_2.weight"), self.P(pre + "norm_2.bias"), mod[:, mo + 3 * D : mo + 4 * D],
                                            mod[:, mo + 4 * D : mo + 5 * D], N, 1e-5, a["t1"], a["x1"], a["xm2"], a["mean2"], a["rstd2"]))
            u = a["u"] if train else None
            if not ops.gemm_nt_swiglu(a["xm2"], sh[pre + "mlp_input.0.weight|g"], u, a["h"], stationary=u is None):
                raise RuntimeError("the row-complete path needs the fused MLP-up kernel")
            if i + 1 < L:
                nx, mn, nxt = lay(i + 1), (i + 1) * 6 * D, f"layers.{i + 1}."
                lnw, lnb, eps = self.P(nxt + "norm_1.weight"), self.P(nxt + "norm_1.bias"), 1e-5
                xm_n, mu_n, rs_n = nx["xm1"], nx["mean1"], nx["rstd1"]
            else:
                mn, lnw, lnb, eps = L * 6 * D, None, None, 1e-6
                xm_n, mu_n, rs_n = w["xf"], w["meanf"], w["rstdf"]
            _must(ops.ln_modulate_gemm_fwd(a["h"], sh[pre + "mlp_input.2.weight|f"], a["x1"], mod[:, mo + 5 * D : mo + 6 * D], lnw, lnb,
                                            mod[:, mn : mn + D], mod[:, mn + D : mn + 2 * D], N, eps, a["t2"], xbuf(i + 1), xm_n, mu_n,
                                            rs_n))

    # ------------------------------------------------------------------ joint (MMDiT) block stage
    def _jstage_fwd(self, blocks, x_in: Tensor, c_in: Tensor, nx: int, pos: Tensor | None, kb: Tensor, x_out: Tensor | None,
                    c_out: Tensor | None) -> tuple | None:
        """MMDiTBlocks `blocks` on (image stream x_in [B*nx, D], context stream c_in [B*Lc, D]) of an engine with joint blocks
        (self._Lc context tokens, self._tabs the joint RoPE tables, layout.mod_off the blocks' modulation columns).  Each stream
        runs the DiT halves with its own weights and its own six modulation chunks; the streams meet in ONE attention launch over
        the joint q / k / v rows ([0, Lc) context, [Lc, Lc + nx) image) with the key-padding mask as the additive key bias kb.
        Outputs materialised into x_out / c_out (rows may be strided); c_out None: the context half of the last block feeds nothing
        and is skipped; x_out None: the pending residual of the image stream is returned for the caller's next LayerNorm"""
        d, w = self.d, self.ws
        B, Lc = self.geo[0], self._Lc
        D, Hh = d.inner_dim, d.num_heads
        cos, sin = self._tabs
        mod = w["mod"]
        Tp = kb.shape[1]
        streams = (("input", nx, Lc, 0, pos), ("context", Lc, 0, 6 * D, None))
        cur = {"input": x_in, "context": c_in}
        pend: dict[str, tuple | None] = {"input": None, "context": None}
        blocks = list(blocks)
        for bi in blocks:
            per, pre, base = w["blk"][bi], self.prefixes[bi], self.layout.mod_off[bi]
            q, k, v = (per["q"], per["k"], per["v"]) if "q" in per else (w["q"], w["k"], w["v"])  # (inference may share one set)
            for st, nt, off, mc, ps in streams:
                a = per[st]
                a["xin"] = cur[st] if pend[st] is None else a["x0"]
                self._half1_fwd(a, block_names(pre, st), a["xin"], pend[st], Modulation(mod, None, base + mc, D, nt), nt, cos[off:],
                                sin[off:], q, k, v, ps, off)
            ops.attn_fwd_ex(q, k, v, per["ao"], per["lse"], B, Hh, Tp, Tp, 64, 64**-0.5, kb)
            for st, nt, off, mc, ps in streams:
                if st == "context" and c_out is None and bi == blocks[-1]:  # (the reference computes and discards it)
                    continue
                a = per[st]
                ops.copy_rows3d(per["ao"][off:], Tp * D, D, a["a"], nt * D, D, B, nt, D)
                pend[st] = self._half2_fwd(a, block_names(pre, st), a["xin"], Modulation(mod, None, base + mc, D, nt))
        if x_out is None:
            return pend["input"]
        ops.gated_residual_fwd(*pend["input"], nx, x_out)
        if c_out is not None:
            ops.gated_residual_fwd(*pend["context"], Lc, c_out)
        return None

    def _jstage_bwd(self, blocks, dx_x: Tensor, dx_c: Tensor | None, nx: int, pos: Tensor | None, kb: Tensor, scr: dict, att: tuple,
                    dfe: dict, sw: "SideWork", pending: bool = False):
        """backward of _jstage_fwd.  dx_x / dx_c: gradients at the stage outputs (contiguous, overwritten; dx_c None: the context output
        was not produced); scr: chain scratch of each stream; att: (dao, dq, dk, dv) over the padded joint rows; pending: the image
        output was handed on as a pending residual, whose backward the caller's LayerNorm backward has run (dfe of the last block
        included).  Returns the gradients at the stage inputs (image, context)."""
        d, w = self.d, self.ws
        B, Lc = self.geo[0], self._Lc
        D, Hh = d.inner_dim, d.num_heads
        cos, sin = self._tabs
        rot = sum(d.rope_axes_dim)
        mod, dmod = w["mod"], w["dmod32"]
        Tp = kb.shape[1]
        streams = (("input", nx, Lc, 0, pos), ("context", Lc, 0, 6 * D, None))
        dao, dq, dk, dv = att
        blocks = list(blocks)
        last = blocks[-1]
        dx: dict[str, Tensor | None] = {"input": dx_x, "context": dx_c}  # residual-stream gradients (None: zero so far)
        if not pending:
            if last in dfe:
                ops.add_bf16(dx_x, dfe[last], dx_x)
            for st, nt, off, mc, ps in streams:  # backward of the materialised last residual of each stream
                if dx[st] is None:
                    continue
                a, mo = w["blk"][last][st], self.layout.mod_off[last] + mc
                ops.gate_bwd(dx[st], a["t2"], mod[:, mo + 5 * D : mo + 6 * D], nt, a["wg"]["dt2"], dmod[:, mo + 5 * D : mo + 6 * D])
        skip_ctx_last = dx_c is None
        for j in reversed(range(len(blocks))):
            bi = blocks[j]
            per, pre = w["blk"][bi], self.prefixes[bi]
            ms = {st: Modulation(mod, dmod, self.layout.mod_off[bi] + mc, D, nt, part=per[st]["dwb"], groups=B) for st, nt, _, mc, _ in streams}
            dao.zero_()
            for st, nt, off, mc, ps in streams:
                if st == "context" and skip_ctx_last and bi == last:
                    continue
                a, s = per[st], scr[st]
                dx[st] = self._half2_bwd(a, a["wg"], block_names(pre, st), s, ms[st], dx[st], sw)
                ops.copy_rows3d(s["da"], nt * D, D, dao[off:], Tp * D, D, B, nt, D)
            ops.attn_bwd_ex(per["q"], per["k"], per["v"], per["ao"], dao, per["lse"], dq, dk, dv, B, Hh, Tp, Tp, 64, 64**-0.5, kb)
            for st, nt, off, mc, ps in streams:
                a, nm = per[st], block_names(pre, st)
                ops.qk_norm_rope_bwd(dq, dk, dv, a["qkv"], self.P(nm["qk"] + ".query_norm.scale"), self.P(nm["qk"] + ".key_norm.scale"),
                                     cos[off:], sin[off:], a["rrms"], a["wg"]["dqkv"], self.G(nm["qk"] + ".query_norm.scale"), B, nt, Hh,
                                     64, rot, pos=ps, n_off=off)
                prev = dres = None
                if j > 0:
                    bp = blocks[j - 1]
                    ap = w["blk"][bp][st]
                    prev = (ap["t2"], self.layout.mod_off[bp] + mc + 5 * D, ap["wg"]["dt2"])
                    dres = dfe.get(bp) if st == "input" else None
                dx[st] = self._half1_bwd(a, a["wg"], nm, scr[st], ms[st], a["xin"], dx[st], prev, dres, sw)
            self._end_block(sw, bi)
        return dx["input"], dx["context"]

    # ------------------------------------------------------------------ backward
    def feature(self, k: int) -> Tensor:
        """output of block k of the last train-mode forward: the residual stream after the block, bf16 [B, N, D] (a view of
        the workspace, valid until the next forward) -- what a forward hook on ``layers[k]`` observes in the reference"""
        assert self._train, "block outputs are only kept by the train-mode launch sequence"
        B, _, _, _, _, N, _, _, _ = self.geo
        return self.ws["x"][k + 1].view(B, N, self.d.inner_dim)

    def backward(self, dpred: Tensor, dfeats: dict[int, Tensor] | None = None, need_dx: bool = False,
                 input_only: bool = False) -> Tensor | None:
        """accumulates d(loss)/d(param) into the flat gradient arena (+=) for the last train-mode forward.
        dfeats: {block index k: gradient of an auxiliary loss w.r.t. feature(k)} (RePA), added to the residual-stream gradient.
        need_dx: also returns d(loss)/d(x) of the input latents, f32 [B, C, H, W] (one dl_patch_embed_dgrad launch on the gradient at
        block 0's input, behind the patch weight gradient).  input_only: the data-gradient chain alone -- no weight gradient, no
        LayerNorm-affine fold, no conditioning path, no side stream, no reducer call; the gradient arena is not written."""
        assert self._train and self.grads is not None
        if input_only:
            self._input_only = True
            try:
                return self._backward_input_only(dpred, dfeats)
            finally:
                self._input_only = False
        dfeats = self._dfeat_rows(dfeats)
        d, w, sh = self.d, self.ws, self.sh
        B, _, _, gh, gw, N, M, _, _ = self.geo
        D, E, L = d.inner_dim, d.embedding_dim, d.depth
        cos, sin = self._rope[(gh, gw)]
        mod, dmod, xs = w["mod"], w["dmod32"], w["x"]  # dmod: f32 accumulator, cast to bf16 (w["dmod"]) after the loop
        dmod[:B].zero_()
        s = {k: w[k] for k in ("dxa", "dxb", "dxm", "da", "dh", "dq", "dk", "dv")}  # chain scratch

        # head: last linear + final adaLN, which runs the gated residual backward of the last block's MLP branch
        fused = self._row_gemms(M, N)
        self._head_bwd(dpred, None if fused else w["dxm"], scratch=w["det_scr"])
        mo, ml = L * 6 * D, (L - 1) * 6 * D
        dx = w["dxa"]
        if fused:  # (row-complete GEMMs: the LayerNorm backward is the epilogue of the data-gradient GEMM in front of it)
            _must(ops.ln_modulate_gemm_bwd(w["dO"], sh["last_layer.linear.weight|t"], xs[L], None, None, mod[:, mo : mo + D], N,
                                            w["meanf"], w["rstdf"], dfeats.get(L - 1), dx, dmod[:, mo : mo + D],
                                            dmod[:, mo + D : mo + 2 * D], None, gate_t=w["layers"][L - 1]["t2"],
                                            gate=mod[:, ml + 5 * D : ml + 6 * D], dt=w["wg"][L - 1]["dt2"],
                                            dgate=dmod[:, ml + 5 * D : ml + 6 * D], K=self._ko))
        else:
            Modulation(mod, dmod, mo, D, N).ln_bwd(w["dxm"], xs[L], None, None, 0, w["meanf"], w["rstdf"], dfeats.get(L - 1), dx, None,
                                                   gate=(w["layers"][L - 1]["t2"], ml + 5 * D, w["wg"][L - 1]["dt2"]))

        # Workgroup cap of the side-stream weight gradients (of 256 CUs).  Four atomic launches per block: 96: 24.5, 128: 24.1, 160:
        # 24.4, 192: 24.8, 256: 25.8 ms/step (round 2).  The grouped launch (one per block, no atomics) wants the whole chip: every
        # kernel of the step is then one workgroup per CU and the two streams simply take turns (64: 23.8, 96: 22.4, 128: 22.3,
        # 192: 22.1, 256: 21.7 ms/step; the same launches inline on the main stream: 21.9).  strict: a grouped launch that declines
        # raises instead of falling back to atomics (the B = 256 step is bit-reproducible).  DL_WGRAD_SERIAL is the A/B switch to
        # weight gradients inline on the main stream
        serial = tuning.on("DL_WGRAD_SERIAL")
        sw = SideWork(self, grouped_wgs=256, serial=serial, strict=True)
        main, side = sw.main, sw.side

        # Data parallel: the stacked adaLN matrix (L*6D x E, a quarter of the parameters) would only be final in _cond_bwd, i.e. its
        # 42 MB would be reduced after the backward has ended.  Every block's 6D rows of the modulation gradient are final when that
        # block's backward is (its MLP gate chunk was written by the block above), so the block's slice of the weight gradient is
        # computed right there on the side stream and handed to the reducer with the block's own range; the last three blocks ask
        # for an immediate flush, which leaves a few megabytes for finish().
        early_mod = self.reducer is not None and type(self) is DiTEngine and tuning.on("DL_DP_EARLY_MOD")
        self._early_mod_done = early_mod
        w_mod = self.layout.entries[self.mod_name][0]
        b_mod = self.layout.entries[self.layout.mod_b0][0]

        def early_mod_rows(r0: int, r1: int) -> None:
            ops.cast2d_f32_to_bf16(w["dmod32"][:B, r0:r1], w["dmod"][:B, r0:r1])
            ops.gemm_tn(w["dmod"][:, r0:r1], w["se"], self.grads[w_mod + r0 * E : w_mod + r1 * E].view(r1 - r0, E))
            ops.colsum(w["dmod"][:, r0:r1], self.grads[b_mod + r0 : b_mod + r1], B, r1 - r0)

        def block_done(i: int) -> None:  # this block's gradient range is final once BOTH streams are past this point
            if self.reducer is None:
                return
            if early_mod:
                sw.run(lambda: early_mod_rows(i * 6 * D, (i + 1) * 6 * D))
            ev_side = side.record_event()
            self.reducer.ready(*self.layer_ranges[i], extra_events=(ev_side,))
            if early_mod:
                self.reducer.ready(w_mod + i * 6 * D * E, w_mod + (i + 1) * 6 * D * E, flush=i < 3)

        native = self._native_blocks() and not serial
        inline_wgrad = tuning.on("DL_WGRAD_INLINE")  # TUNING: the grouped weight gradients on the main stream
        defer_fold = fused and self.reducer is None  # LayerNorm-affine partials of every block: one batched fold after the loop
        for i in reversed(range(L)):
            dres = dfeats.get(i - 1)  # auxiliary-loss gradient on the output of block i-1 (= this block's input)
            if native:
                blk = self._block_args(i, True)
                blk.set(dfeat=dres)
                ops.dit_block_bwd(blk, main.cuda_stream, main.cuda_stream if inline_wgrad else side.cuda_stream, sw.side_wgs)
            elif fused:
                dx = self._block_bwd_row_gemms(i, dx, dres, s, sw, not defer_fold)
            else:
                prev = (w["layers"][i - 1]["t2"], (i - 1) * 6 * D + 5 * D, w["wg"][i - 1]["dt2"]) if i > 0 else None
                m = Modulation(mod, dmod, i * 6 * D, D, N, part=(w["dwb"][2 * i], w["dwb"][2 * i + 1]), groups=B)
                dx = self._dit_block_bwd(w["layers"][i], w["wg"][i], f"layers.{i}.", xs[i], dx, prev, dres, s, m, N, cos, sin, sw,
                                         kb=w.get("kb"), dao=w.get("dao"))
            block_done(i)
        # Without a gradient reducer nothing reads the weight gradients before the optimizer, so the join with the side stream comes
        # LAST: the LayerNorm-affine fold and the conditioning backward (~0.3 ms of small main-stream kernels) run under the grouped
        # weight-gradient launch of the first block instead of behind it.  (Data parallel: _cond_bwd ends in reducer.finish(), which
        # must see every range final -- the join stays in front.)
        join_last = self.reducer is None and tuning.on("DL_JOIN_LAST")
        if not join_last:
            sw.join()
        if defer_fold:  # dwb [2L, B, 2, D]: rows 2i -> norm_1 of block i, 2i + 1 -> norm_2; [w; b] of a norm are adjacent in the arena
            ent = self.layout.entries
            stride = ent[self.prefixes[1] + "norm_1.weight"][0] - ent[self.prefixes[0] + "norm_1.weight"][0] if L > 1 else 0
            for j, nm in enumerate(("norm_1.weight", "norm_2.weight")):
                ops.reduce_rows_batched_f32(w["dwb"][j], 2 * B * 2 * D, self.G(self.prefixes[0] + nm), stride, L, B, 2 * D)

        self._cond_bwd(dx)
        if join_last:
            sw.join()
        return self._input_grad(dx) if need_dx else None

    # ------------------------------------------------------------------ gradient of the input latents
    _input_only = False  # True while _backward_input_only runs: the shared backward pieces then leave the gradient arena alone

    def _input_grad(self, dx: Tensor) -> Tensor:
        """d(loss)/d(input latents) f32 [B, C, H, W] from the gradient dx of the patch-embedded tokens (block 0's input)"""
        B, H, W = self.geo[0], self.geo[1], self.geo[2]
        dimg = torch.empty(B, self.d.input_channels, H, W, device=self.dev, dtype=torch.float32)
        return ops.patch_embed_dgrad(dx, self.P(self._conv_name), dimg, self.d.patch_size)

    def _qk_scale_sink(self, qk: str) -> Tensor:
        """where the QK-norm backward leaves its scale gradients ([query; key], adjacent in the arena) during an input-gradient-only
        backward: a scratch of the same extent, never read"""
        ent = self.layout.entries
        (q0, qs), (k0, ks) = ent[qk + ".query_norm.scale"], ent[qk + ".key_norm.scale"]
        n = k0 - q0 + math.prod(ks)
        sink = getattr(self, "_qk_sink", None)
        if sink is None or sink.numel() < n:
            sink = self._qk_sink = self._z(n, dtype=torch.float32)
        return sink[: math.prod(qs)]

    def _backward_input_only(self, dpred: Tensor, dfeats: dict[int, Tensor] | None) -> Tensor:
        """backward() reduced to its data-gradient chain: the Python-issued block sequence that matches the forward's saved
        activations (row-complete GEMMs or the plain one; the native C sequence launches the same kernels as these) with the
        weight gradients and folds of SideWork made no-ops, everything on the caller's stream.  Writes workspace buffers only."""
        dfeats = self._dfeat_rows(dfeats)
        d, w, sh = self.d, self.ws, self.sh
        B, _, _, gh, gw, N, M, _, _ = self.geo
        D, L = d.inner_dim, d.depth
        cos, sin = self._rope[(gh, gw)]
        mod, dmod, xs = w["mod"], w["dmod32"], w["x"]
        dmod[:B].zero_()
        s = {k: w[k] for k in ("dxa", "dxb", "dxm", "da", "dh", "dq", "dk", "dv")}
        fused = self._row_gemms(M, N)
        ops.patchify(dpred, w["dO"], d.patch_size, ops.PATCH_PPC)
        if not fused:
            ops.gemm_nt(w["dO"], sh["last_layer.linear.weight|t"], w["dxm"], M=M, N=D, K=self._ko)
        mo, ml = L * 6 * D, (L - 1) * 6 * D
        dx = w["dxa"]
        if fused:
            _must(ops.ln_modulate_gemm_bwd(w["dO"], sh["last_layer.linear.weight|t"], xs[L], None, None, mod[:, mo : mo + D], N,
                                            w["meanf"], w["rstdf"], dfeats.get(L - 1), dx, dmod[:, mo : mo + D],
                                            dmod[:, mo + D : mo + 2 * D], None, gate_t=w["layers"][L - 1]["t2"],
                                            gate=mod[:, ml + 5 * D : ml + 6 * D], dt=w["wg"][L - 1]["dt2"],
                                            dgate=dmod[:, ml + 5 * D : ml + 6 * D], K=self._ko))
        else:
            Modulation(mod, dmod, mo, D, N).ln_bwd(w["dxm"], xs[L], None, None, 0, w["meanf"], w["rstdf"], dfeats.get(L - 1), dx, None,
                                                   gate=(w["layers"][L - 1]["t2"], ml + 5 * D, w["wg"][L - 1]["dt2"]))
        sw = _NoSideWork()
        for i in reversed(range(L)):
            dres = dfeats.get(i - 1)
            if fused:  # (the LayerNorm-affine partials it writes into ws["dwb"] are overwritten, never added to, by a later backward)
                dx = self._block_bwd_row_gemms(i, dx, dres, s, sw, False)
            else:
                prev = (w["layers"][i - 1]["t2"], (i - 1) * 6 * D + 5 * D, w["wg"][i - 1]["dt2"]) if i > 0 else None
                m = Modulation(mod, dmod, i * 6 * D, D, N, part=(None, None), groups=B)
                dx = self._dit_block_bwd(w["layers"][i], w["wg"][i], f"layers.{i}.", xs[i], dx, prev, dres, s, m, N, cos, sin, sw,
                                         kb=w.get("kb"), dao=w.get("dao"))
        return self._input_grad(dx)

    def _block_bwd_row_gemms(self, i: int, dx: Tensor, dres: Tensor | None, s: dict, sw: "SideWork", fold: bool) -> Tensor:
        """backward of block i of _forward_row_gemms: the sequence of _dit_block_bwd with each LayerNorm-modulate backward as the
        epilogue of the data-gradient GEMM in front of it (dl_ln_modulate_gemm_bwd).  fold False: the LayerNorm-affine partials stay
        in ws["dwb"] for the caller's batched fold"""
        d, w, sh = self.d, self.ws, self.sh
        _, _, _, gh, gw, N, _, _, _ = self.geo
        D = d.inner_dim
        mod, dmod = w["mod"], w["dmod32"]
        a, g, nm, mo = w["layers"][i], w["wg"][i], block_names(f"layers.{i}."), i * 6 * D
        sw.wgrad(g["dt2"], a["h"], nm["down"] + ".weight")
        ops.mlp_swiglu_bwd(g["dt2"], sh[nm["down"] + ".weight|t"], a["xm2"], sh[nm["up"] + ".weight|g"], a["u"], s["dh"], g["du"])
        sw.wgrad(g["du"], a["xm2"], nm["up"] + ".weight")
        nx = _other(s, dx)
        _must(ops.ln_modulate_gemm_bwd(g["du"], sh[nm["up"] + ".weight|t"], a["x1"], self.P(nm["n2"] + ".weight"),
                                        self.P(nm["n2"] + ".bias"), mod[:, mo + 3 * D : mo + 4 * D], N, a["mean2"], a["rstd2"], dx, nx,
                                        dmod[:, mo + 3 * D : mo + 4 * D], dmod[:, mo + 4 * D : mo + 5 * D], w["dwb"][2 * i + 1],
                                        gate_t=a["t1"], gate=mod[:, mo + 2 * D : mo + 3 * D], dt=g["dt1"],
                                        dgate=dmod[:, mo + 2 * D : mo + 3 * D]))
        if fold:
            sw.fold(w["dwb"][2 * i + 1], nm["n2"] + ".weight", self.geo[0])
        dx = nx
        sw.wgrad(g["dt1"], a["a"], nm["proj"] + ".weight")
        ops.gemm_nt(g["dt1"], sh[nm["proj"] + ".weight|t"], s["da"])
        self._attn_bwd(a, g, nm, s, N, *self._rope[(gh, gw)], None, None, None)
        sw.wgrad(g["dqkv"], a["xm1"], nm["qkv"] + ".weight")
        if dres is not None:
            ops.add_bf16(dx, dres, dx)
        nxt = {}
        if i > 0:  # gated residual of the previous block's MLP branch
            mp = (i - 1) * 6 * D
            nxt = dict(gate_t=w["layers"][i - 1]["t2"], gate=mod[:, mp + 5 * D : mp + 6 * D], dt=w["wg"][i - 1]["dt2"],
                       dgate=dmod[:, mp + 5 * D : mp + 6 * D])
        nx = _other(s, dx)
        _must(ops.ln_modulate_gemm_bwd(g["dqkv"], sh[nm["qkv"] + ".weight|t"], w["x"][i], self.P(nm["n1"] + ".weight"),
                                        self.P(nm["n1"] + ".bias"), mod[:, mo : mo + D], N, a["mean1"], a["rstd1"], dx, nx,
                                        dmod[:, mo : mo + D], dmod[:, mo + D : mo + 2 * D], w["dwb"][2 * i], **nxt))
        if fold:
            sw.fold(w["dwb"][2 * i], nm["n1"] + ".weight", self.geo[0])
        return nx

    def _head_bwd(self, dpred: Tensor, dxm: Tensor | None, scratch: Tensor | None = None) -> None:
        """backward of the last linear: dpred patchified into ws["dO"], its weight gradient (through an f32 slab padded to 8 rows
        when the output features are ragged) and bias gradient, and (dxm not None) the data gradient into dxm.  scratch: the
        bit-reproducible forms of the small GEMM / column sum (ops.gemm_tn)"""
        d, w = self.d, self.ws
        M, Fo, D = self.geo[6], self.geo[8], d.inner_dim
        ops.patchify(dpred, w["dO"], d.patch_size, ops.PATCH_PPC)
        gl = self.G("last_layer.linear.weight")
        if Fo % 8 == 0:
            ops.gemm_tn(w["dO"], w["xf"], gl, M=Fo, N=D, scratch=scratch)
        else:
            w["scr_last"].zero_()
            ops.gemm_tn(w["dO"], w["xf"], w["scr_last"], M=_rup(Fo, 8), N=D, scratch=scratch)
            ops.reduce_rows_f32(w["scr_last"], gl, 1, Fo * D)
        ops.colsum(w["dO"], self.G("last_layer.linear.bias"), M, Fo, scratch=scratch)
        if dxm is not None:
            ops.gemm_nt(w["dO"], self.sh["last_layer.linear.weight|t"], dxm, M=M, N=D, K=self._ko)

    def _dfeat_rows(self, dfeats: dict[int, Tensor] | None) -> dict[int, Tensor]:
        """the auxiliary-loss gradients {block index: d(loss)/d(feature(k))} as contiguous bf16 token rows [B*N, D]"""
        return {k: g.reshape(-1, self.d.inner_dim).to(torch.bfloat16).contiguous() for k, g in (dfeats or {}).items()}

    def _patch_wgrad(self, dx: Tensor, name: str, scratch: Tensor | None) -> None:
        """weight gradient of the patch-embedding convolution `name` from the gradient dx of its tokens (through an f32 slab padded
        to 8 columns when the patch features are ragged); scratch: the bit-reproducible form of the GEMM (ops.gemm_tn)"""
        d, w = self.d, self.ws
        D, Fi = d.inner_dim, d.input_channels * d.patch_size**2
        gc = self.G(name).view(D, Fi)
        if Fi % 8 == 0:
            ops.gemm_tn(dx, w["tokP"], gc, M=D, N=Fi, scratch=scratch)
        else:
            w["scr_conv"].zero_()
            ops.gemm_tn(dx, w["tokP"], w["scr_conv"], M=D, N=_rup(Fi, 8), scratch=scratch)
            gc.add_(w["scr_conv"][:, :Fi])  # ragged edge (e.g. RGB p=2 -> 12 features): torch slice-add, not on the hot path

    def _end_block(self, sw: "SideWork", bi: int) -> None:
        """end of block bi's backward in a staged engine: its pending weight gradients are issued and, data parallel, its gradient
        range is handed to the reducer behind the side stream's work so far"""
        sw.flush()
        if self.reducer is not None:
            self.reducer.ready(*self.layer_ranges[bi], extra_events=(sw.side.record_event(),))

    def _cond_bwd(self, dx: Tensor, extra_demb: Tensor | None = None) -> None:
        """backward of _stem_fwd: dx = gradient of the patch-embedded tokens; the modulation gradient was accumulated in
        ws["dmod32"] by the block kernels.  extra_demb: f32 [>= B, E] further gradient of the time embedding (DDT's decoder)"""
        d, w, sh = self.d, self.ws, self.sh
        B, _, _, _, _, _, M, _, _ = self.geo
        D, E = d.inner_dim, d.embedding_dim
        dmod = w["dmod32"]
        det = w.get("det_scr")  # scratch of the bit-reproducible small GEMMs / column sums (None: the atomic forms)
        self._patch_wgrad(dx, self._conv_name, det)  # (no gradient flows to the input latents)

        # conditioning path: every adaLN linear at once, then the time MLP and the label table
        R = self.layout.mod_rows
        g_modw = self.grads[self.layout.entries[self.mod_name][0] :][: R * E].view(R, E)
        g_modb = self.grads[self.layout.entries[self.layout.mod_b0][0] :][:R]
        L6 = len(self.prefixes) * 6 * D if getattr(self, "_early_mod_done", False) else 0
        if L6:  # the blocks' rows were cast, multiplied and handed to the reducer as the blocks finished (backward: block_done)
            ops.cast2d_f32_to_bf16(dmod[:B, L6:], w["dmod"][:B, L6:])
            dmod = w["dmod"]
            ops.gemm_tn(dmod[:, L6:], w["se"], g_modw[L6:], scratch=det)
            ops.colsum(dmod[:, L6:], g_modb[L6:], B, R - L6, scratch=det)
        else:
            ops.cast_f32_to_bf16(dmod[:B], w["dmod"][:B])
            dmod = w["dmod"]
            ops.gemm_tn(dmod, w["se"], g_modw, scratch=det)
            ops.colsum(dmod, g_modb, B, R, scratch=det)
        ops.gemm_nt(dmod, sh["@mod|t"], w["dse"], M=B, N=E, K=R, scratch=det)
        table = d.n_classes is not None
        if self._pooled_dim:  # demb reaches both MLPs; extra_demb (DDT's decoder) is a gradient of the time embedding alone
            ops.cond_combine_dense_bwd(w["dse"][:B], w["emb"][:B], w["demb"][:B], w["demb16"][:B])
            self._pooled_bwd(B, det)
        else:
            ops.cond_combine_bwd(w["dse"][:B], w["emb"][:B], self._yeff if table else None, w["demb"][:B], w["demb16"][:B],
                                 self.G("label_embed.embedding.weight") if table else None)
        if extra_demb is not None:
            w["demb"][:B].add_(extra_demb[:B])
            ops.cast_f32_to_bf16(w["demb"][:B], w["demb16"][:B])
        ops.colsum(w["demb"], self.G("time_embed.2.bias"), B, E, scratch=det)
        ops.gemm_tn(w["demb16"], w["h1"], self.G("time_embed.2.weight"), scratch=det)
        ops.gemm_nt(w["demb16"], sh["time_embed.2.weight|t"], w["dh1"], M=B, N=E, K=E)
        ops.silu_bwd(w["dh1"][:B], w["pre1"][:B], w["dpre1"][:B])
        ops.gemm_tn(w["dpre1"], w["temb"], self.G("time_embed.0.weight"), scratch=det)
        ops.colsum(w["dpre1"], self.G("time_embed.0.bias"), B, E, scratch=det)
        if self.reducer is not None:
            if L6:
                w_mod = self.layout.entries[self.mod_name][0]
                self.reducer.ready(0, w_mod)
                self.reducer.ready(w_mod + L6 * E, self.layer_ranges[0][0])
            else:
                self.reducer.ready(0, self.layer_ranges[0][0])
            self.reducer.finish()


class _StrictWgradGroups(ops.WgradGroups):
    """WgradGroups for a backward that must stay free of atomics: a grouped launch that declines its problems raises"""

    def _issue(self, key: int) -> None:
        probs = self.pending.pop(key, [])
        if probs:
            self.launch(lambda: _must(ops.gemm_tn_group(probs, self.slab, max_wgs=self.max_wgs)))


class _NoSideWork:
    """SideWork of an input-gradient-only backward: nothing off the data-gradient chain is launched"""

    def wgrad(self, dy: Tensor, x: Tensor, name: str) -> None:
        pass

    def fold(self, partial: Tensor | None, name: str, groups: int) -> None:
        pass

    def flush(self) -> None:
        pass

    def join(self) -> None:
        pass


class SideWork:
    """the side-stream half of a bf16 transformer engine's backward.  The four weight-gradient GEMMs of a block and the
    LayerNorm-affine folds are off the dependency chain (nothing downstream reads them), so they run on a SIDE HIP stream, each launch
    behind an event recorded on the main stream when it is issued: they overlap the HBM-bound kernels of the main chain (gate / SwiGLU
    / adaLN / QK-norm backward), which leave the matrix pipes idle.  Their inputs (dt2, du, dt1, dqkv) live in per-block buffers so
    the main chain never overwrites something the side stream still reads.  The linears of a block (per token stream) are collected
    and issued as ONE atomics-free dl_gemm_tn_group launch where the workspace has a grouped-launch slab (ops.WgradGroups), else as
    one atomic launch each.  grouped_wgs: default workgroup cap with the slab; serial: the weight gradients (not the folds) run
    inline on the main stream, uncapped; strict: see _StrictWgradGroups.
    Built where the backward begins to issue side work: the side stream waits for everything the main stream has issued so far."""

    def __init__(self, eng: DiTEngine, grouped_wgs: int = 128, serial: bool = False, strict: bool = False) -> None:
        self.G, self.width = eng.G, 2 * eng.d.inner_dim
        self.main = torch.cuda.current_stream()
        self.side = eng._side_stream()
        self.side.wait_stream(self.main)
        slab = eng.ws.get("tn_slab")
        self.side_wgs = tuning.integer("DL_SIDE_WGS", grouped_wgs if slab is not None else 128)  # cap of the side-stream launches (of 256 CUs)
        self.wgs, self.launch = (0, lambda fn: fn()) if serial else (self.side_wgs, self.run)
        groups = _StrictWgradGroups if strict else ops.WgradGroups
        self.groups = groups(slab, self.launch, max_wgs=self.wgs) if slab is not None else None

    def run(self, fn) -> None:
        """fn() on the side stream, behind everything the main stream has issued so far"""
        ev = self.main.record_event()
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            fn()

    def wgrad(self, dy: Tensor, x: Tensor, name: str) -> None:
        """G(name) += dy^T x"""
        if self.groups is not None:
            self.groups.add(dy, x, self.G(name))
        else:
            self.launch(lambda: ops.gemm_tn(dy, x, self.G(name), max_wgs=self.wgs))

    def flush(self) -> None:
        """issue the grouped weight gradients still pending (at every block end)"""
        if self.groups is not None:
            self.groups.flush()

    def fold(self, partial: Tensor, name: str, groups: int) -> None:
        """[groups, 2, D] partial sums of a LayerNorm's affine gradients -> its adjacent [w; b] gradient (partials cleared)"""
        self.run(lambda: ops.reduce_rows_f32(partial, self.G(name), groups, self.width, clear=True))

    def join(self) -> None:
        self.main.wait_stream(self.side)
