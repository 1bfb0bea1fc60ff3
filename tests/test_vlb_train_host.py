"""Host tests of L_vlb training with loss-aware timestep sampling (Nichol & Dhariwal 2021, sec. 3.3): the arguments
`GaussianDiffusion` takes and refuses, the numpy resampler of tests/vlb_train_common.py against hand-worked cases, the restatement's
hand-written derivative of the bound with respect to the mean output against torch autograd in fp64, the sampler state's
`state_dict` round trip, the data-parallel gather helper on two gloo ranks, and the shipped config.  No GPU, no library call.
"""

import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import gd_param_common as gp
import vlb_train_common as vt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEARNED = {"sampler_parameters": {"var_type": "learned_range"}}


def GD(**kw):
    from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion

    return GaussianDiffusion(**kw)


# ------------------------------------------------------------------------------------------------------------------ arguments
def test_defaults_and_accepted_arguments():
    gd = GD()
    assert gd.loss_type == "mse" and gd.timestep_sampler == "uniform" and gd.timestep_sampler_state is None
    t = gd.draw_timesteps(7, device="cuda")  # "uniform" ignores the device
    assert t.device.type == "cpu" and t.dtype == torch.int32 and t.shape == (7,)
    gd = GD(loss_type="vlb", timestep_sampler="loss_second_moment", **LEARNED)
    s = gd.timestep_sampler_state
    assert (s.n_steps, s.history_per_term, s.uniform_prob) == (1000, 10, 0.001)
    gd = GD(timestep_sampler="loss_second_moment", sampler_history=3, sampler_uniform_prob=0.0, loss_weighting="min_snr")
    assert gd.timestep_sampler_state.history_per_term == 3 and gd.loss_type == "mse"
    from diffulab_amd import Diffuser

    d = Diffuser(torch.nn.Linear(1, 1), sampling_method="ddpm", model_type="gaussian_diffusion",
                 extra_args={"loss_type": "vlb", "timestep_sampler": "loss_second_moment", "sampler_history": 4, **LEARNED})
    assert d.diffusion.loss_type == "vlb" and d.diffusion.timestep_sampler_state.history_per_term == 4


@pytest.mark.parametrize("kw,names", [
    ({"loss_type": "vlb"}, ("loss_type", "var_type")),  # fixed variances: the variance is not trained
    ({"loss_type": "vlb", "sampler_parameters": {"var_type": "fixed_large"}}, ("loss_type", "var_type")),
    ({"loss_type": "vlb", "loss_weighting": "min_snr", **LEARNED}, ("loss_weighting",)),
    ({"loss_type": "vlb", "latent_diffusion": True, **LEARNED}, ("latent_diffusion",)),
    ({"loss_type": "l2"}, ("loss_type",)),
    ({"timestep_sampler": "importance"}, ("timestep_sampler",)),
    ({"timestep_sampler": "loss_second_moment", "sampler_history": 0}, ("sampler_history",)),
    ({"timestep_sampler": "loss_second_moment", "sampler_history": 2.5}, ("sampler_history",)),
    ({"timestep_sampler": "loss_second_moment", "sampler_uniform_prob": -0.1}, ("sampler_uniform_prob",)),
    ({"timestep_sampler": "loss_second_moment", "sampler_uniform_prob": 1.5}, ("sampler_uniform_prob",)),
    ({"sampler_history": 0}, ("sampler_history",)),  # validated whatever the sampler
    ({"loss_type": "vlb", "sampler_parameters": {"var_type": "learned", "mean_type": "xstart"}}, ("loss_target",)),
])
def test_refusals_name_the_argument(kw, names):
    with pytest.raises(ValueError) as e:
        GD(**kw)
    assert all(n in str(e.value) for n in names), str(e.value)


def test_loss_aware_draw_needs_a_device():
    gd = GD(timestep_sampler="loss_second_moment")
    with pytest.raises(ValueError, match="device"):
        gd.draw_timesteps(4)


def test_set_steps_onto_another_chain_resets_the_state():
    gd = GD(timestep_sampler="loss_second_moment", sampler_history=2)
    s = gd.timestep_sampler_state
    s.on("cpu")["counts"].fill_(2)
    gd.set_steps(1000)  # the same chain: the history stays
    assert s.n_steps == 1000 and int(s.tensors["counts"].sum()) == 2000
    gd.set_steps(8)
    assert gd.timestep_sampler_state is s and s.n_steps == 8 and not s.tensors
    t = s.on("cpu")
    assert t["history"].shape == (8, 2) and int(t["counts"].sum()) == 0 and torch.equal(t["p"], torch.full((8,), 0.125))
    assert torch.equal(t["imp"], torch.ones(8)) and torch.equal(t["cdf"], torch.arange(1, 9) / 8)


# ------------------------------------------------------------------------------------------------------------------ numpy resampler
def test_resampler_partly_filled_history_is_uniform():
    r = vt.Resampler(4, H=2, uniform_prob=0.1)
    r.update([0, 1, 1, 3], [1.0, 2.0, 3.0, 4.0])
    assert r.count.tolist() == [1, 2, 0, 1] and not r.warmed_up()
    assert r.hist.tolist() == [[1.0, 0.0], [2.0, 3.0], [0.0, 0.0], [4.0, 0.0]]
    p, imp, cdf = r.tables()
    assert p.tolist() == [0.25] * 4 and imp.tolist() == [1.0] * 4 and cdf.tolist() == [0.25, 0.5, 0.75, 1.0]


def test_resampler_warm_up_flips_when_the_last_count_reaches_h():
    r = vt.Resampler(2, H=2, uniform_prob=0.0)
    r.update([0, 0, 1], [3.0, 4.0, 1.0])
    assert not r.warmed_up() and r.tables()[0].tolist() == [0.5, 0.5]
    r.update([1], [1.0])  # the last count reaches H
    assert r.warmed_up()
    p, imp, cdf = r.tables()
    w0, w1 = np.sqrt((9.0 + 16.0) / 2), 1.0
    assert np.allclose(p, [w0 / (w0 + w1), w1 / (w0 + w1)], rtol=1e-15, atol=0)
    assert np.allclose(imp, 1.0 / (2 * p), rtol=1e-15, atol=0) and cdf[-1] == 1.0 and np.isclose(cdf[0], p[0], rtol=1e-15, atol=0)
    r2 = vt.Resampler(2, H=2, uniform_prob=0.5)
    r2.hist[:], r2.count[:] = r.hist, r.count
    assert np.allclose(r2.tables()[0], 0.5 * p + 0.25, rtol=1e-15, atol=0)


def test_resampler_shift_order_and_duplicates_within_a_batch():
    r = vt.Resampler(2, H=3)
    r.update([0, 0, 0, 1], [1.0, 2.0, 3.0, 9.0])
    assert r.hist[0].tolist() == [1.0, 2.0, 3.0] and r.count.tolist() == [3, 1]
    r.update([0, 1, 0], [4.0, 8.0, 5.0])  # two more of index 0: shifted in array order
    assert r.hist[0].tolist() == [3.0, 4.0, 5.0] and r.hist[1].tolist() == [9.0, 8.0, 0.0] and r.count.tolist() == [3, 2]
    assert vt.draw(np.array([0.25, 0.5, 1.0]), np.array([0.0, 0.2499, 0.25, 0.75, 0.9999])).tolist() == [0, 0, 1, 2, 2]


# ------------------------------------------------------------------------------------------------------------------ the derivative
@pytest.mark.parametrize("var_type", vt.LEARNED)
@pytest.mark.parametrize("name", gp.TARGETS)
def test_analytic_mean_derivative_against_autograd(name, var_type):
    """fp64, the 8-step chain, t = 0, 0, 1, T-2, T-1: both branches of the term; with a weight and an importance table, and upstream
    gradients other than 1"""
    T, t = vt.chain("t8")
    c = vt.bp.case(T, t, 192, name, var_type)
    weight = None if name == "xprev" else gp.min_snr(T.alphas_bar, name).float()
    imp = vt.imp_table(8)
    for loss_type, w in (("vlb", None), ("mse", weight)):
        pred = c["pred"].double().requires_grad_(True)
        out = vt.rows(c["tab"], pred, c["eps"], c["x0"], c["xt"], t, name, var_type, w, imp, loss_type, 0.3)
        vt.check_inputs(c, out)
        (0.7 * out["loss"][0] + 1.3 * out["loss"][1]).backward()
        hand = vt.rows_backward(c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], t, name, var_type, w, imp, loss_type, 0.7, 1.3)
        err = float((hand - pred.grad).abs().max())
        scale = float(pred.grad.abs().max())
        print(f"{name}/{var_type} {loss_type}: max|grad| {scale:.3e}  max|hand - autograd| {err:.3e}")
        assert err <= 1e-12 * scale
        first = (t == 0)
        mean_half = pred.grad[:, :192]
        bound_part = mean_half - vt.rows_backward(c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], t, name, var_type, w, imp, "mse", 0.7,
                                                  1.3)[:, :192]
        if loss_type == "vlb":  # the bound reaches the mean output, at t == 0 and at t > 0
            assert float(bound_part[first].abs().max()) > 0 and float(bound_part[~first].abs().max()) > 0
        else:
            assert float(bound_part.abs().max()) <= 1e-12 * scale


def test_restatement_rows_average_to_the_batch_scalars_of_gd_param_common():
    T, t = vt.chain("t8")
    c = vt.bp.case(T, t, 192, "v", "learned_range")
    out = vt.rows(c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], t, "v", "learned_range", None, None, "mse", 1.0)
    mse, vb = gp.loss(c["tab"], c["pred"], c["eps"], c["x0"], c["xt"], t, "v", "learned_range")
    assert abs(float(out["mse_row"].mean() - mse)) <= 1e-14 * float(mse) and abs(float(out["vb_row"].mean() - vb)) <= 1e-14 * float(vb)
    assert torch.allclose(out["loss"], torch.stack([mse, vb]), rtol=1e-14, atol=0)
    assert torch.allclose(out["total_row"], out["mse_row"] + out["vb_row"], rtol=1e-15, atol=0)


# ------------------------------------------------------------------------------------------------------------------ state
def test_state_dict_round_trip():
    from diffulab_amd.diffuse.modelizations.timestep_sampler import LossSecondMomentState

    s = LossSecondMomentState(6, history=3, uniform_prob=0.05)
    assert set(s.state_dict()) == {"n_steps", "history_per_term", "uniform_prob"}  # nothing allocated yet
    ten = s.on("cpu")
    g = torch.Generator().manual_seed(0)
    ten["history"].copy_(torch.rand(6, 3, generator=g))
    ten["counts"].copy_(torch.tensor([3, 3, 1, 0, 3, 2], dtype=torch.int32))
    ten["p"].copy_(torch.rand(6, generator=g))
    sd = s.state_dict()
    assert sd["history"] is not ten["history"] and sd["counts"].dtype == torch.int32
    s2 = LossSecondMomentState(6)
    s2.load_state_dict(sd)
    assert (s2.history_per_term, s2.uniform_prob) == (3, 0.05)
    for k in LossSecondMomentState.KEYS:
        assert torch.equal(s2.tensors[k], ten[k]) and s2.tensors[k].dtype == ten[k].dtype, k
    ten["history"].zero_()  # the loaded state is a copy
    assert float(s2.tensors["history"].abs().sum()) > 0
    with pytest.raises(ValueError, match="6-step"):
        LossSecondMomentState(8).load_state_dict(sd)
    with pytest.raises(ValueError, match="history"):
        LossSecondMomentState(6).load_state_dict({**sd, "history": torch.zeros(6, 4)})
    gd = GD(timestep_sampler="loss_second_moment", sampler_history=3)
    gd.set_steps(6)
    gd.timestep_sampler_state.load_state_dict(sd)
    assert torch.equal(gd.timestep_sampler_state.tensors["counts"], ten["counts"])


# ------------------------------------------------------------------------------------------------------------------ gather
def _gather_worker(rank: int, world: int, port: int, out):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from diffulab_amd.diffuse.modelizations.timestep_sampler import gather_pairs

    t = torch.tensor([rank * 10, rank * 10 + 1, 3], dtype=torch.int32)
    loss = torch.tensor([rank + 0.5, rank + 0.25, 7.0 + rank])
    ta, la = gather_pairs(t, loss)
    out[rank] = (ta.tolist(), la.tolist(), str(ta.dtype), str(la.dtype))
    dist.destroy_process_group()


def test_gather_pairs_two_gloo_ranks_in_rank_order():
    from diffulab_amd.diffuse.modelizations.timestep_sampler import gather_pairs

    t, loss = torch.tensor([1, 2], dtype=torch.int32), torch.tensor([0.5, 0.25])
    ta, la = gather_pairs(t, loss)  # no process group: the arguments themselves
    assert ta is t and la is loss
    mgr = mp.Manager()
    out = mgr.dict()
    port = 31500 + (os.getpid() % 2000)
    mp.spawn(_gather_worker, args=(2, port, out), nprocs=2, join=True)
    want = ([0, 1, 3, 10, 11, 3], [0.5, 0.25, 7.0, 1.5, 1.25, 8.0], "torch.int32", "torch.float32")
    assert out[0] == want and out[1] == want, dict(out)


# ------------------------------------------------------------------------------------------------------------------ config
def test_the_vlb_config_composes():
    from diffulab_amd.config import load_config

    cfg = load_config(os.path.join(ROOT, "configs"), "train_mnist_ddpm_vlb")
    ea = cfg.diffuser.extra_args
    assert ea.loss_type == "vlb" and ea.timestep_sampler == "loss_second_moment" and ea.sampler_parameters.var_type == "learned_range"
    assert cfg.model.out_channels == 2 and cfg.diffuser.model_type == "gaussian_diffusion"
    gd = GD(n_steps=cfg.diffuser.n_steps, sampling_method=cfg.diffuser.sampling_method,
            **{k: (dict(v) if hasattr(v, "items") else v) for k, v in ea.items()})
    assert gd.loss_type == "vlb" and gd.timestep_sampler_state.n_steps == cfg.diffuser.n_steps
