"""CPU checks of gradient clipping by global norm: the chain-length arithmetic the GPU test's error bound is derived from, the new
constructor arguments and their defaults, and the header entries."""

import inspect
import re

from diffulab_amd import _lib, ops


def test_grad_sumsq_chain_arithmetic():
    """256 threads x 4 float4 per workgroup and iteration (4096 floats), at most 512 workgroups: a per-thread accumulator grows by
    one term per iteration; + 1 head / tail element + 12 levels of in-workgroup tree (4 over the thread's 16 accumulators, 6 inside
    the wave, 2 over the 4 waves)"""
    assert ops.grad_sumsq_chain(0) == 0 and ops.grad_sumsq_slots(0) == 0
    for n in (1, 3):  # (no whole float4: head / tail elements only)
        assert ops.grad_sumsq_chain(n) == 13 and ops.grad_sumsq_slots(n) == 1, n
    for n in (4, 63, 257, 4096):
        assert ops.grad_sumsq_chain(n) == 1 + 13 and ops.grad_sumsq_slots(n) == 1, n
    assert ops.grad_sumsq_slots(4096 + 4) == 2 and ops.grad_sumsq_chain(4096 + 4) == 14
    assert ops.grad_sumsq_slots(512 * 4096) == 512 and ops.grad_sumsq_chain(512 * 4096) == 14
    assert ops.grad_sumsq_slots(512 * 4096 + 4) == 512 and ops.grad_sumsq_chain(512 * 4096 + 4) == 15  # the second grid pass
    assert ops.grad_sumsq_chain(3_000_001) == 15  # 733 tiles over 512 workgroups
    assert ops.grad_sumsq_chain(2**31 - 1) == 1024 + 13
    last = 0
    for n in (1, 2**20, 2**28, 2**31 - 1):
        c = ops.grad_sumsq_chain(n)
        assert last <= c <= 4096, (n, c)
        last = c


def test_grad_sumsq_refuses_a_slot_range_past_the_partials_buffer():
    """argument validation happens before any device work: dummy non-null pointers are never dereferenced"""
    import ctypes

    buf = ctypes.create_string_buffer(256)
    P = ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)
    L = _lib.lib()
    rc = L.cdll.dl_grad_sumsq(P, ctypes.c_int64(3_000_001), P, ctypes.c_int64(1), ctypes.c_int64(512), None)
    assert rc < 0 and "dl_grad_sumsq" in L.cdll.dl_last_error().decode()
    rc = L.cdll.dl_grad_sumsq(ctypes.c_void_p(P.value + 2), ctypes.c_int64(8), P, ctypes.c_int64(0), ctypes.c_int64(8), None)
    assert rc < 0


def test_constructors_take_max_grad_norm_defaulting_to_none():
    from diffulab_amd.training import BaseTrainer, FusedAdamW
    from diffulab_amd.training.utils import clip_grad_norm_

    for cls in (BaseTrainer, FusedAdamW):
        prm = inspect.signature(cls.__init__).parameters["max_grad_norm"]
        assert prm.default is None, cls
    sig = inspect.signature(clip_grad_norm_)
    assert list(sig.parameters) == ["parameters", "max_norm", "grad_scale"] and sig.parameters["grad_scale"].default == 1.0


def test_trainer_keeps_the_bound(tmp_path):
    from diffulab_amd.training import BaseTrainer

    assert BaseTrainer(n_epoch=1, save_path=tmp_path, project_name="a").max_grad_norm is None
    assert BaseTrainer(n_epoch=1, save_path=tmp_path, project_name="b", max_grad_norm=1).max_grad_norm == 1.0


def test_header_declares_the_clipping_entry_points_under_optimizer_side():
    text = open(_lib.HEADER_PATH).read()
    side = text[text.index("optimizer side"):]
    protos = _lib.parse_header()
    for name in ("dl_grad_sumsq", "dl_grad_sumsq_slots", "dl_grad_sumsq_chain", "dl_clip_coef", "dl_adamw_step_clip",
                 "dl_adamw_step_dev_clip", "dl_scale_inplace"):
        assert name in protos and re.search(r"DL_API\s+\w+\s+%s\(" % name, side), name
    assert "torch.nn.utils.clip_grad_norm_" in side and "accelerate" in side
    assert protos["dl_adamw_step_clip"][2][-2:] == ["coef", "stream"] and protos["dl_adamw_step_dev_clip"][2][-2:] == ["coef", "stream"]
    for name in ("grad_sumsq", "clip_coef", "adamw_step_clip", "adamw_step_dev_clip", "scale_inplace", "grad_sumsq_chain"):
        assert callable(getattr(ops, name)), name
