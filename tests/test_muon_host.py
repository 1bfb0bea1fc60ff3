"""CPU checks of the fused Muon: ``optimizer=muon`` resolves to ``FusedMuon`` with the YAML's hyper-parameters, the constructor
validates what ``torch.optim.Muon`` validates (same messages), the Muon / auxiliary split of the smallest DiT, ``use_muon``, the
tables ``ops.MuonPlan`` builds, and the C entry points refuse what is out of contract before any device work."""

import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from diffulab_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_optimizer_muon_config_resolves_to_fused_muon():
    from diffulab_amd.config import instantiate, load_config
    from diffulab_amd.training import FusedArenaOptimizer, FusedMuon

    c = load_config(os.path.join(ROOT, "configs"), "train_mnist_flow_matching", ["optimizer=muon"])
    assert c.optimizer._target_ == "torch.optim.Muon"  # (torch's string stays)
    ps = [torch.nn.Parameter(torch.zeros(64, 128)), torch.nn.Parameter(torch.zeros(7))]
    opt = instantiate(c.optimizer, params=ps)
    assert type(opt) is FusedMuon and isinstance(opt, FusedArenaOptimizer) and isinstance(opt, torch.optim.Optimizer)
    g = opt.param_groups[0]
    assert (g["lr"], g["weight_decay"], g["momentum"], g["nesterov"], g["eps"], g["ns_steps"], g["adjust_lr_fn"]) == (
        1e-3, 0.1, 0.95, True, 1e-7, 5, None)
    assert g["ns_coefficients"] == (3.4445, -4.7750, 2.0315)
    assert (g["aux_lr"], g["aux_betas"], g["aux_eps"], g["aux_weight_decay"], g["use_muon"]) == (None, (0.9, 0.999), 1e-8, 1e-2, None)
    assert opt.grad_scale == 1.0 and opt.max_grad_norm is None and opt.last_grad_norm is None
    assert [opt.is_muon(p, g) for p in ps] == [True, False]


BAD_ARGS = [dict(lr=-1.0), dict(momentum=-0.5), dict(weight_decay=-1e-4), dict(adjust_lr_fn="rms"), dict(lr=torch.zeros(2))]
GOOD_ARGS = [dict(), dict(lr=0.0), dict(momentum=0.0, nesterov=False), dict(adjust_lr_fn="original"), dict(adjust_lr_fn="match_rms_adamw"),
             dict(ns_steps=0), dict(ns_steps=99, eps=1e-6, ns_coefficients=(3.0, -3.2, 1.2))]
NAMES = ("lr", "weight_decay", "momentum", "nesterov", "ns_coefficients", "eps", "ns_steps", "adjust_lr_fn")


def test_constructor_shares_names_defaults_and_messages_with_torchs():
    from diffulab_amd.training import FusedMuon

    sig, ref = inspect.signature(FusedMuon.__init__).parameters, inspect.signature(torch.optim.Muon.__init__).parameters
    assert list(sig)[: len(ref)] == list(ref)  # (same names in the same order, the additions after them)
    for name in NAMES:
        assert sig[name].default == ref[name].default, name
    aw = inspect.signature(torch.optim.AdamW.__init__).parameters
    assert sig["aux_lr"].default is None and sig["max_grad_norm"].default is None
    assert (sig["aux_betas"].default, sig["aux_eps"].default, sig["aux_weight_decay"].default) == (
        aw["betas"].default, aw["eps"].default, aw["weight_decay"].default)

    def one():
        return [torch.nn.Parameter(torch.zeros(64, 64))]

    for kw in BAD_ARGS:
        msgs = []
        for cls in (torch.optim.Muon, FusedMuon):
            with pytest.raises(ValueError) as e:
                cls(one(), **kw)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], kw
    for kw in GOOD_ARGS:
        a, b = (cls(one(), **kw) for cls in (torch.optim.Muon, FusedMuon))
        for k in NAMES:
            assert a.defaults[k] == b.defaults[k], (kw, k)
    # torch raises these from the first step, inside _zeropower_via_newtonschulz: the same messages, at construction
    from torch.optim._muon import _zeropower_via_newtonschulz

    for kw in (dict(ns_steps=100), dict(ns_coefficients=(1.0, 2.0))):
        with pytest.raises(ValueError) as want:
            _zeropower_via_newtonschulz(torch.zeros(64, 64), kw.get("ns_coefficients", (1.0, 1.0, 1.0)), kw.get("ns_steps", 5), 1e-7)
        with pytest.raises(ValueError) as got:
            FusedMuon(one(), **kw)
        assert str(got.value) == str(want.value), kw
    # unlike torch's class: a whole model, 1-D tensors included
    model = torch.nn.Sequential(torch.nn.Linear(64, 128), torch.nn.LayerNorm(128))
    with pytest.raises(ValueError, match="only supports 2D"):
        torch.optim.Muon(model.parameters())
    for params in (model, model.parameters()):
        opt = FusedMuon(params)
        assert [opt.is_muon(p, opt.param_groups[0]) for p in opt.param_groups[0]["params"]] == [True, False, False, False]


def small_dit():
    """the depth-2 DiT at DiT-S/2's widths (configs/model/dit_s2.yaml: six heads of 64, embedding_dim 384, a null class)"""
    from diffulab_amd import MMDiT

    return MMDiT(simple_dit=True, inner_dim=384, embedding_dim=384, num_heads=6, depth=2, n_classes=10, classifier_free=True, patch_size=2,
                 input_channels=4)


def test_muon_and_auxiliary_split_of_the_smallest_dit():
    from diffulab_amd.training import FusedMuon

    m = small_dit()
    opt = FusedMuon(m.parameters())
    names = {id(p): n for n, p in m.named_parameters()}
    g = opt.param_groups[0]
    muon = {names[id(p)] for p in g["params"] if opt.is_muon(p, g)}
    want = {f"layers.{i}.{s}.weight" for i in range(2) for s in ("modulation.lin", "attention.qkv", "attention.proj_out", "mlp_input.0",
                                                                  "mlp_input.2")}
    want |= {"time_embed.0.weight", "time_embed.2.weight", "last_layer.adaLN_modulation.1.weight"}
    assert muon == want
    shapes = {n: tuple(p.shape) for n, p in m.named_parameters()}
    assert shapes["label_embed.embedding.weight"] == (11, 384) and shapes["last_layer.linear.weight"] == (16, 384)
    assert shapes["conv_proj.weight"][0] == 384 and len(shapes["conv_proj.weight"]) == 4
    assert not muon & {"label_embed.embedding.weight", "last_layer.linear.weight", "conv_proj.weight"}
    assert all(len(shapes[n]) != 2 or n in muon or min(shapes[n]) % 64 or max(shapes[n]) % 64 for n in shapes)
    # an embedding table of 1023 classes has 1024 rows: selected
    assert FusedMuon.qualifies(torch.empty(1024, 384)) and not FusedMuon.qualifies(torch.empty(1001, 384))


def test_use_muon_per_param_group():
    from diffulab_amd.training import FusedMuon

    a, b, c = (torch.nn.Parameter(torch.zeros(s)) for s in ((128, 64), (64, 64), (16, 384)))
    opt = FusedMuon([{"params": [a]}, {"params": [b, c], "use_muon": False}])
    g0, g1 = opt.param_groups
    assert opt.is_muon(a, g0) and not opt.is_muon(b, g1) and not opt.is_muon(c, g1)
    FusedMuon([{"params": [a, b], "use_muon": True}])
    with pytest.raises(ValueError, match=r"\(16, 384\)"):
        FusedMuon([{"params": [a, c], "use_muon": True}])


def test_begin_graph_mode_is_refused():
    from diffulab_amd.training import FusedMuon

    opt = FusedMuon([torch.nn.Parameter(torch.zeros(64, 64))])
    with pytest.raises(NotImplementedError, match="FusedMuon"):
        opt.begin_graph_mode()
    assert not opt.in_graph_mode()


def test_plan_tables_tile_the_buffer():
    mats = [(5, 64, 128, 1.0), (5 + 64 * 128 + 3, 128, 64, 2.0**0.5), (30000, 192, 448, 1.0)]
    n = 30000 + 192 * 448 + 7
    for phase in range(4):
        plan = ops.MuonPlan(n, mats, phase, "cpu")
        ck, mt = plan.chunks_host.numpy(), plan.mats_host.numpy()
        assert ck[0, 0] == 0 and (ck[1:, 0] == ck[:-1, 0] + ck[:-1, 1]).all() and ck[-1, 0] + ck[-1, 1] == n
        assert ck[:, 1].min() >= 1 and ck[:, 1].max() <= ops.MUON_CHUNK and plan.n_chunks == len(ck) and plan.has_aux
        for i, (off, r, c, ratio) in enumerate(mats):
            mine = ck[ck[:, 2] == i]
            assert mine[0, 0] == off and mine[:, 1].sum() == r * c
            assert (mt[i, 8], mt[i, 9]) == (np.flatnonzero(ck[:, 2] == i)[0], len(mine))
            assert np.uint32(mt[i, 3]).view(np.float32) == np.float32(ratio)
            # chunk boundaries inside a range fall on 16-byte boundaries of the buffer
            assert ((mine[1:, 0] + phase) % 4 == 0).all()
        assert list(mt[:, 6]) == [0, 1, 2, 11] and list(mt[:, 7]) == [0, 2, 4, 25]
        assert list(mt[:3, 4]) == [0, 8192, 16384] and list(mt[:3, 5]) == [0, 4096, 8192]
        assert plan.x_cap == 16384 + 192 * 448 and plan.a_cap == 8192 + 192 * 192
    assert ops.MuonPlan(100, [], 0, "cpu").has_aux and not ops.MuonPlan(64 * 64, [(0, 64, 64, 1.0)], 0, "cpu").has_aux
    assert ops.muon_ratio(128, 64, None) == 2.0**0.5 and ops.muon_ratio(64, 128, "original") == 1.0
    assert ops.muon_ratio(64, 128, "match_rms_adamw") == 0.2 * 128**0.5


def _dummy():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)


def test_entry_points_refuse_out_of_contract_arguments_before_any_launch():
    """argument validation happens before any device work: the device pointers are dummies that are never dereferenced, the host
    tables are real"""
    keep, P = _dummy()
    L = _lib.lib()
    f, i64, ci = ctypes.c_float, ctypes.c_int64, ctypes.c_int
    names = ("dl_muon_pre", "dl_muon_orthogonalize", "dl_muon_post")
    for name in names:
        assert name in L.protos
    plan = ops.MuonPlan(64 * 128 + 16, [(16, 64, 128, 1.0)], 0, "cpu")
    n = plan.n

    def tables(rows=64, cols=128, off=16, xoff=0):
        mt = plan.mats_host.clone()
        mt[0, 0], mt[0, 1], mt[0, 2], mt[0, 4] = off, rows, cols, xoff
        return mt

    def pre(p=P, g=P, m=P, v=P, n=n, mt=None, ck=None, n_mat=1, xws=P, partials=P, momentum=0.95, chunks_dev=P, mats_dev=P):
        mt = plan.mats_host if mt is None else mt
        ck = plan.chunks_host if ck is None else ck
        rc = L.cdll.dl_muon_pre(p, g, m, v, i64(n), ctypes.c_void_p(ck.data_ptr()), chunks_dev, i64(len(ck)),
                                ctypes.c_void_p(mt.data_ptr()), mats_dev, i64(n_mat), xws, i64(plan.x_cap), partials, i64(len(ck)), f(1e-3),
                                f(0.9), f(0.999), f(1e-8), f(0.01), f(0.1), f(0.001), f(momentum), f(1.0), None, ci(1), None)
        return rc, L.cdll.dl_last_error().decode()

    def orth(mt=None, mats_dev=P, partials=P, norms=P, xws=P, aws=P, ns_steps=5, n_mat=1):
        mt = plan.mats_host if mt is None else mt
        rc = L.cdll.dl_muon_orthogonalize(ctypes.c_void_p(mt.data_ptr()), mats_dev, i64(n_mat), partials, norms, xws, i64(plan.x_cap), aws,
                                          i64(plan.a_cap), f(1e-7), f(3.4445), f(-4.775), f(2.0315), ci(ns_steps), None)
        return rc, L.cdll.dl_last_error().decode()

    def post(p=P, n=n, mt=None, mats_dev=P, xo=P, n_mat=1):
        mt = plan.mats_host if mt is None else mt
        rc = L.cdll.dl_muon_post(p, i64(n), ctypes.c_void_p(mt.data_ptr()), mats_dev, i64(n_mat), xo, i64(plan.x_cap), f(1e-3), f(0.1), None)
        return rc, L.cdll.dl_last_error().decode()

    short = plan.chunks_host[:-1].contiguous()
    swapped = plan.chunks_host.clone()
    swapped[1, 2] = -1  # a chunk inside the matrix marked auxiliary
    bad = {
        pre: [dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(n=0), dict(xws=None), dict(partials=None), dict(chunks_dev=None),
              dict(mats_dev=None), dict(momentum=-0.1), dict(ck=short), dict(ck=swapped), dict(n=n + 1), dict(mt=tables(off=17)),
              dict(mt=tables(xoff=64)), dict(p=ctypes.c_void_p(P.value + 2))],
        orth: [dict(mats_dev=None), dict(partials=None), dict(norms=None), dict(xws=None), dict(aws=None), dict(ns_steps=-1),
               dict(ns_steps=100), dict(n_mat=0), dict(xws=ctypes.c_void_p(P.value + 8))],
        post: [dict(p=None), dict(xo=None), dict(mats_dev=None), dict(n=0), dict(n=64 * 128), dict(n_mat=0)],
    }
    for fn, name in zip((pre, orth, post), names):
        for kw in bad[fn]:
            rc, msg = fn(**kw)
            assert rc == -1 and name in msg, (name, kw, rc, msg)  # DL_ERR_INVALID
        # a dimension that is not a multiple of 64, or past the limits: DL_ERR_UNSUPPORTED with the shape in the message
        for rows, cols in ((96, 128), (64, 100), (64, 32768 + 64), (4096 + 64, 8192)):
            rc, msg = fn(mt=tables(rows, cols))
            assert rc == -3 and name in msg and f"{rows} x {cols}" in msg, (name, rows, cols, rc, msg)
    del keep


def test_header_declares_the_muon_entry_points():
    text = open(_lib.HEADER_PATH).read()
    m = re.search(r"enum \{ DL_MUON_MAT_FIELDS = (\d+), DL_MUON_CHUNK_FIELDS = (\d+), DL_MUON_CHUNK = (\d+) \}", text)
    assert m and tuple(int(x) for x in m.groups()) == (ops.MUON_MAT_FIELDS, ops.MUON_CHUNK_FIELDS, ops.MUON_CHUNK)
    for name in ("dl_muon_pre", "dl_muon_orthogonalize", "dl_muon_post"):
        assert re.search(r"DL_API\s+int\s+%s\(" % name, text), name
    assert "dl_muon_orthogonalize" in _lib._VALUE_RETURNING  # (it returns its launch count)
