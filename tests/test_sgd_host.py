"""CPU checks of the fused SGD: ``optimizer=sgd`` resolves to ``FusedSGD`` with the YAML's hyper-parameters, the C entry points refuse
what is out of contract before any device work, the constructor validates what ``torch.optim.SGD``'s does, and a
``torch.optim.SGD`` state dict loads."""

import ctypes
import inspect
import os
import re

import pytest
import torch

from diffulab_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_optimizer_sgd_config_resolves_to_fused_sgd():
    from diffulab_amd.config import instantiate, load_config
    from diffulab_amd.training import FusedAdamW, FusedArenaOptimizer, FusedSGD

    c = load_config(os.path.join(ROOT, "configs"), "train_cifar10_flow_matching", ["optimizer=sgd"])
    assert c.optimizer._target_ == "torch.optim.SGD"  # (the reference's string stays)
    ps = [torch.nn.Parameter(torch.zeros(3, 5)), torch.nn.Parameter(torch.zeros(7))]
    opt = instantiate(c.optimizer, params=ps)
    assert type(opt) is FusedSGD and isinstance(opt, FusedArenaOptimizer) and isinstance(opt, torch.optim.Optimizer)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"], g["dampening"], g["maximize"]) == (1e-3, 0.9, 1e-4, True, 0, False)
    assert opt.grad_scale == 1.0 and opt.max_grad_norm is None and opt.last_grad_norm is None
    assert issubclass(FusedAdamW, FusedArenaOptimizer)
    # what hydra may pass along is accepted (and ignored)
    instantiate(dict(c.optimizer, foreach=None, fused=None, differentiable=False), params=ps)


def _dummy():
    buf = ctypes.create_string_buffer(256)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)


def test_entry_points_refuse_out_of_contract_arguments_before_any_launch():
    """argument validation happens before any device work: dummy non-null pointers are never dereferenced"""
    keep, P = _dummy()
    L = _lib.lib()
    f, i64, ci = ctypes.c_float, ctypes.c_int64, ctypes.c_int
    L.protos["dl_sgd_step"], L.protos["dl_sgd_step_dev"]  # (declared in the header, so lib() set their prototypes)

    def host(p=P, g=P, buf=P, n=8, mom=0.9, damp=0.0, flags=0):
        rc = L.cdll.dl_sgd_step(p, g, buf, i64(n), f(0.1), f(mom), f(damp), f(0.0), f(1.0), None, ci(flags), None)
        return rc, L.cdll.dl_last_error().decode()

    def dev(p=P, g=P, buf=P, n=8, hyper=P, flags=0):
        rc = L.cdll.dl_sgd_step_dev(p, g, buf, i64(n), hyper, None, ci(flags), None)
        return rc, L.cdll.dl_last_error().decode()

    bad_host = [dict(p=None), dict(g=None), dict(n=0), dict(n=-4), dict(buf=None),  # (momentum 0.9 without a buffer)
                dict(flags=ops.SGD_NESTEROV, mom=0.0), dict(flags=ops.SGD_NESTEROV, mom=0.0, buf=None),
                dict(flags=ops.SGD_NESTEROV, damp=0.1), dict(flags=8), dict(p=ctypes.c_void_p(P.value + 2))]
    for kw in bad_host:
        rc, msg = host(**kw)
        assert rc < 0 and re.search(r"\bdl_sgd_step\b", msg), (kw, rc, msg)
    bad_dev = [dict(p=None), dict(g=None), dict(n=0), dict(hyper=None), dict(flags=ops.SGD_FIRST),
               dict(flags=ops.SGD_NESTEROV, buf=None), dict(flags=8), dict(g=ctypes.c_void_p(P.value + 1))]
    for kw in bad_dev:
        rc, msg = dev(**kw)
        assert rc < 0 and "dl_sgd_step_dev" in msg, (kw, rc, msg)
    del keep


def test_header_declares_the_sgd_entry_points_under_optimizer_side():
    text = open(_lib.HEADER_PATH).read()
    side = text[text.index("optimizer side"):]
    protos = _lib.parse_header()
    assert protos["dl_sgd_step"][2] == ["p", "g", "buf", "n", "lr", "momentum", "dampening", "weight_decay", "grad_scale", "coef",
                                        "flags", "stream"]
    assert protos["dl_sgd_step_dev"][2] == ["p", "g", "buf", "n", "hyper", "coef", "flags", "stream"]
    for name in ("dl_sgd_step", "dl_sgd_step_dev"):
        assert re.search(r"DL_API\s+int\s+%s\(" % name, side), name
    assert "configs/optimizer/sgd.yaml" in side and "base_trainer.py:149" in side
    m = re.search(r"enum \{ DL_SGD_NESTEROV = (\d+), DL_SGD_FIRST = (\d+), DL_SGD_MAXIMIZE = (\d+) \}", side)
    assert m and tuple(int(x) for x in m.groups()) == (ops.SGD_NESTEROV, ops.SGD_FIRST, ops.SGD_MAXIMIZE)
    assert callable(ops.sgd_step) and callable(ops.sgd_step_dev)


BAD_ARGS = [dict(lr=-1.0), dict(momentum=-0.5), dict(weight_decay=-1e-4), dict(nesterov=True), dict(nesterov=True, momentum=0.0),
            dict(nesterov=True, momentum=0.9, dampening=0.1)]
GOOD_ARGS = [dict(), dict(lr=0.0), dict(momentum=0.9, nesterov=True), dict(momentum=0.5, dampening=0.3, weight_decay=0.01),
             dict(momentum=0.9, dampening=0.1, maximize=True)]


def test_constructor_validates_what_torchs_does():
    from diffulab_amd.training import FusedSGD

    sig, ref = inspect.signature(FusedSGD.__init__).parameters, inspect.signature(torch.optim.SGD.__init__).parameters
    for name in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
        assert sig[name].default == ref[name].default, name
    assert sig["max_grad_norm"].default is None
    for kw in BAD_ARGS:
        msgs = []
        for cls in (torch.optim.SGD, FusedSGD):
            with pytest.raises(ValueError) as e:
                cls([torch.nn.Parameter(torch.zeros(2))], **kw)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1], kw
    for kw in GOOD_ARGS:
        a, b = (cls([torch.nn.Parameter(torch.zeros(2))], **kw) for cls in (torch.optim.SGD, FusedSGD))
        for k in ("lr", "momentum", "dampening", "weight_decay", "nesterov", "maximize"):
            assert a.defaults[k] == b.defaults[k], (kw, k)


def test_load_state_dict_accepts_a_torch_sgd_checkpoint():
    from diffulab_amd.training import FusedSGD

    def params():
        torch.manual_seed(0)
        return [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))]

    ref_p = params()
    ref = torch.optim.SGD(ref_p, lr=0.1, momentum=0.9, nesterov=True, weight_decay=1e-4)
    for p in ref_p:
        p.grad = torch.ones_like(p)
    ref.step()
    sd = ref.state_dict()
    opt = FusedSGD(params(), lr=0.5)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["nesterov"], g["weight_decay"]) == (0.1, 0.9, True, 1e-4)
    for p, q in zip(opt.param_groups[0]["params"], ref_p):
        assert torch.equal(opt.state[p]["momentum_buffer"], ref.state[q]["momentum_buffer"])
    # a checkpoint taken before the first step (no buffers yet), and this class's own layout
    FusedSGD(params(), lr=0.5).load_state_dict(torch.optim.SGD(params(), lr=0.1, momentum=0.9).state_dict())
    own = FusedSGD(params(), lr=0.1, momentum=0.9)
    own.state[own.param_groups[0]["params"][0]].update(step=4, buf=torch.arange(22.0))
    again = FusedSGD(params(), lr=0.5)
    again.load_state_dict(own.state_dict())
    st = again.state[again.param_groups[0]["params"][0]]
    assert st["step"] == 4 and torch.equal(st["buf"], torch.arange(22.0))
