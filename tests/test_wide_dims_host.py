"""CPU checks of the wide-row limits (inner_dim up to 4096 in the bf16 regime): every transformer form constructs at the wide widths
with the reference's state_dict layout, the widths beyond stay refused, the fp32 regime refuses wide models by name, and the row
kernels' C entry points validate the width before any device work (so the refusals are testable without a GPU)."""

from __future__ import annotations

import ctypes

import pytest
import torch

from diffulab_amd import _lib, ops
from oracle import ddt as oddt
from oracle import dit as odit
from oracle import mmdit as ommdit
from oracle import sprint as osprint

FAKE = ctypes.c_void_p(256)  # never dereferenced: validation returns first
WIDE = [1152, 1536, 2048, 4096]
CD = 96  # context width of the joint forms


def _device(D):
    # D = 4096 blocks hold ~0.5 G parameters per joint form: build those on the meta device (the same constructor and checks, no data)
    return torch.device("meta") if D >= 4096 else torch.device("cpu")


def _kw(D, **extra):
    return dict(input_channels=4, output_channels=4, inner_dim=D, embedding_dim=64, num_heads=D // 64, mlp_ratio=1, patch_size=2,
                **extra)


def _joint_rope(D):
    return [20, 22, 22]  # the default [dh // 3] * 3 = [21, 21, 21] has odd axis widths, which the joint engines refuse


def _ctx():
    from diffulab_amd.networks.embedders import PrecomputedEmbedder

    return PrecomputedEmbedder(torch.zeros(1, 8, CD), null_embedding_seq_len=2)


def _shapes(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.mark.parametrize("D", WIDE)
def test_class_conditional_mmdit_constructs(D):
    from diffulab_amd import MMDiT

    kw = _kw(D, depth=1, n_classes=10, classifier_free=True)
    with _device(D):
        m = MMDiT(simple_dit=True, **kw)
    assert _shapes(m) == odit.param_shapes(odit.DiTConfig(**kw))
    assert m.precisions == ("bf16",)


@pytest.mark.parametrize("D", WIDE)
@pytest.mark.parametrize("ns", [0, 1])
def test_joint_mmdit_constructs(D, ns):
    from diffulab_amd import MMDiT

    kw = _kw(D, depth=2, rope_axes_dim=_joint_rope(D), classifier_free=True)
    with _device(D):
        m = MMDiT(simple_dit=False, context_embedder=_ctx(), n_single_stream_blocks=ns, **kw)
    assert _shapes(m) == ommdit.param_shapes(ommdit.JointConfig(context_dim=CD, n_single_stream_blocks=ns, **kw))


@pytest.mark.parametrize("D", WIDE)
def test_sprint_constructs(D):
    from diffulab_amd import SprintDiT

    kw = _kw(D, encoder_depth=1, deep_layers_depth=1, decoder_depth=1, n_classes=10, classifier_free=True)
    with _device(D):
        m = SprintDiT(simple_dit=True, **kw)
    assert _shapes(m) == osprint.param_shapes(osprint.SprintConfig(**kw))
    assert m.precisions == ("bf16",)


@pytest.mark.parametrize("D", WIDE)
def test_joint_sprint_with_single_stream_blocks_constructs(D):
    from diffulab_amd import SprintDiT

    kw = _kw(D, encoder_depth=1, deep_layers_depth=2, n_single_stream_blocks=1, decoder_depth=1, rope_axes_dim=_joint_rope(D),
             classifier_free=True)
    with _device(D):
        m = SprintDiT(simple_dit=False, context_embedder=_ctx(), **kw)
    assert _shapes(m) == osprint.joint_param_shapes(osprint.SprintJointConfig(context_dim=CD, **kw))


@pytest.mark.parametrize("D", WIDE)
def test_ddt_constructs(D):
    from diffulab_amd import DDT

    kw = {k: v for k, v in _kw(D, encoder_depth=1, decoder_depth=1, n_classes=10, classifier_free=True).items() if k != "embedding_dim"}
    with _device(D):
        m = DDT(simple_ddt=True, **kw)
    assert _shapes(m) == oddt.param_shapes(oddt.DDTConfig(**kw))
    assert m.precisions == ("bf16",)


@pytest.mark.parametrize("D", WIDE)
def test_joint_ddt_constructs(D):
    from diffulab_amd import DDT

    kw = {k: v for k, v in _kw(D, encoder_depth=1, decoder_depth=1, rope_axes_dim=_joint_rope(D), classifier_free=True).items()
          if k != "embedding_dim"}
    with _device(D):
        m = DDT(simple_ddt=False, context_embedder=_ctx(), **kw)
    assert _shapes(m) == oddt.joint_param_shapes(oddt.DDTJointConfig(context_dim=CD, **kw))


@pytest.mark.parametrize("D,H", [(4160, 65), (1536, 12), (2048, 16)])
def test_beyond_4096_and_other_head_dims_refused(D, H):
    from diffulab_amd import MMDiT

    with pytest.raises(NotImplementedError, match="4096" if D > 4096 else "head_dim 64"):
        with torch.device("meta"):
            MMDiT(simple_dit=True, **dict(_kw(D, depth=1, n_classes=10), num_heads=H))
    with pytest.raises(NotImplementedError):
        with torch.device("meta"):
            MMDiT(simple_dit=False, context_embedder=_ctx(), **dict(_kw(D, depth=1, rope_axes_dim=_joint_rope(D)), num_heads=H))


@pytest.mark.parametrize("form", ["mmdit", "sprint", "ddt"])
def test_wide_class_conditional_model_refuses_fp32(form):
    from diffulab_amd import DDT, MMDiT, SprintDiT

    kw = _kw(1152, n_classes=10)
    if form == "mmdit":
        m = MMDiT(simple_dit=True, depth=1, **kw)
    elif form == "sprint":
        m = SprintDiT(simple_dit=True, encoder_depth=1, deep_layers_depth=1, decoder_depth=1, **kw)
    else:
        m = DDT(simple_ddt=True, encoder_depth=1, decoder_depth=1, **{k: v for k, v in kw.items() if k != "embedding_dim"})
    assert m.precisions == ("bf16",)
    with pytest.raises(NotImplementedError, match="inner_dim <= 1024") as e:
        m.set_precision("fp32")
    assert "bf16" in str(e.value) and "1152" in str(e.value)
    assert m.precision == "bf16"
    m.set_precision("bf16")  # the bf16 regime stays available


def test_narrow_class_conditional_model_keeps_fp32():
    from diffulab_amd import MMDiT

    m = MMDiT(simple_dit=True, depth=1, **_kw(1024, n_classes=10))
    assert m.precisions == ("bf16", "fp32")
    m.set_precision("fp32")
    assert m.precision == "fp32"


def test_trainer_prepare_refuses_fp32_for_a_wide_model(tmp_path):
    from diffulab_amd import Diffuser, MMDiT
    from diffulab_amd.training.trainers.common import Trainer

    m = MMDiT(simple_dit=True, depth=1, **_kw(1152, n_classes=10))
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=2)
    class _T(Trainer):  # prepare() alone: the precision check is its first step, before any device placement
        train = training_step = validation_step = None

    tr = _T.__new__(_T)
    tr.precision_type = "no"
    with pytest.raises(NotImplementedError, match="precision_type=bf16") as e:
        tr.prepare(d, None)
    assert "inner_dim <= 1024" in str(e.value)


# ---------------------------------------------------------------- C entry points: D = 4160 and D % 8 != 0 are refused before any launch

def _ln_fwd(D):
    return ("dl_ln_modulate_fwd", [FAKE, None, None, FAKE, FAKE, D, 64, ctypes.c_float(1e-6), FAKE, FAKE, FAKE, None, None, 0, None,
                                   64, D, None])


def _ln_bwd(D):
    return ("dl_ln_modulate_bwd", [FAKE, FAKE, None, None, FAKE, D, 64, FAKE, FAKE, None, FAKE, FAKE, FAKE, D, None, None, None, 0, None,
                                   None, 64, D, None])


def _ln_bwd_tok(D):
    return ("dl_ln_modulate_bwd_tok", [FAKE, FAKE, None, None, FAKE, D, FAKE, FAKE, None, FAKE, FAKE, FAKE, D, None, 0, None, None, 0,
                                       None, None, 64, D, None])


def _gate_bwd(D):
    return ("dl_gate_bwd", [FAKE, FAKE, FAKE, D, 64, FAKE, FAKE, D, 64, D, None])


def _qk_fwd(H, dh):
    return ("dl_qk_norm_rope_fwd", [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 64, H, dh, 0, ctypes.c_float(1e-6), None])


def _qk_fwd_ex(H, dh):
    return ("dl_qk_norm_rope_fwd_ex", [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 64, H, dh, 0, ctypes.c_float(1e-6), None,
                                       64, 0, None])


def _qk_bwd(H, dh):
    return ("dl_qk_norm_rope_bwd", [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 64, H, dh, 0, None])


def _qk_bwd_ex(H, dh):
    return ("dl_qk_norm_rope_bwd_ex", [FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1, 64, H, dh, 0, None, 64, 0,
                                       None])


ROW_CALLS = [_ln_fwd, _ln_bwd, _ln_bwd_tok, _gate_bwd]
QK_CALLS = [_qk_fwd, _qk_fwd_ex, _qk_bwd, _qk_bwd_ex]


@pytest.mark.parametrize("call", ROW_CALLS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("D,needle", [(4160, "4096"), (8192, "4096"), (1540, "multiple of 8")])
def test_row_entry_points_refuse_width(call, D, needle):
    L = _lib.lib()
    name, args = call(D)
    with pytest.raises(RuntimeError, match=name) as e:
        L.call(name, *args)
    assert needle in str(e.value) and str(D) in str(e.value)


@pytest.mark.parametrize("call", QK_CALLS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("H,dh,needle", [(65, 64, "4096"), (128, 64, "4096"), (16, 12, "dh=12")])
def test_qk_entry_points_refuse_width(call, H, dh, needle):
    L = _lib.lib()
    name, args = call(H, dh)
    with pytest.raises(RuntimeError, match=name.replace("_ex", "")) as e:
        L.call(name, *args)
    assert needle in str(e.value)


def test_row_extent_guard_at_4096_wide_mlp():
    """at D = 4096 with mlp_ratio 4 the MLP rows are 16384 wide: 2^31 / 16384 = 131072 token rows; 65536 token rows of the SwiGLU
    up-projection (2 F = 32768 columns) already reach 2^31 and are refused by the guard the engines call"""
    D, F = 4096, 4 * 4096
    ops.check_row_extent(65536, 3 * D, "qkv")
    ops.check_row_extent(65535, 2 * F, "mlp up")
    with pytest.raises(NotImplementedError, match="2\\^31"):
        ops.check_row_extent(65536, 2 * F, "mlp up")


def test_grouped_wgrad_slab_bounded_above_1024():
    WG = ops.WgradGroups
    for D in (256, 384, 640, 1024):  # unchanged up to 1024: eight token ranges
        assert WG.slab_floats(D, 4 * D) == 8 * (4 * D * D + 3 * D * 4 * D)
    for D in (1152, 1536, 2048, 4096):
        per = 4 * D * D + 3 * D * 4 * D
        assert per <= WG.slab_floats(D, 4 * D) < 8 * per
    assert WG.slab_floats(4096, 4 * 4096) == 4 * 4096 * 4096 + 3 * 4096 * 4 * 4096  # one range: 1.07 G floats, not 8.6 G


def test_dit_engine_refuses_65536_token_rows_at_4096_wide_mlp4():
    """the engine's own guard at that edge, before any allocation: 16 samples of 64 x 64 tokens = 65536 rows at D = 4096, mlp_ratio 4"""
    from diffulab_amd.engine import DiTDims, DiTEngine

    dims = DiTDims(inner_dim=4096, embedding_dim=64, num_heads=64, mlp_ratio=4, depth=1, n_classes=10)
    eng = DiTEngine(dims, torch.device("meta"))
    with pytest.raises(NotImplementedError, match="65536 token rows x 32768 columns"):
        eng._alloc(16, 128, 128, True)
