"""CPU tests of the host-side logic of the product package (no kernels are called): schedule tables, timestep draws,
respacing, module/state_dict contract, flat-arena layout, optimizer/arena plumbing.  Expected values are the committed
reference outputs (tests/golden/schedules.npz) -- bit-exact."""

import copy
import os

import numpy as np
import pytest
import torch

from diffulab_amd.diffuse.modelizations.flow import Flow
from diffulab_amd.diffuse.modelizations.gaussian_diffusion import GaussianDiffusion
from diffulab_amd.diffuse.modelizations.utils import space_timesteps
from diffulab_amd.engine import DiTDims, ParamLayout, rope_grid_tables
from diffulab_amd.networks.denoisers import MMDiT


def t2n(x):
    return x.detach().numpy()


def test_flow_grid_and_draws_match_reference(golden):
    g = golden("schedules")
    for n in (4, 50, 100):
        assert np.array_equal(np.array(Flow(n_steps=n).timesteps), g[f"flow_ts_n{n}"])
        for sh in (4.63, 6.93):
            f = Flow(n_steps=n, shift=sh)
            assert np.array_equal(np.array(f.timesteps), g[f"flow_ts_ctor_n{n}_shift{sh}"])  # ctor shift: draws only
            f.set_steps(n, shift=sh)
            assert np.array_equal(np.array(f.timesteps), g[f"flow_ts_n{n}_shift{sh}"])
    for seed in (0, 1, 2):
        for B in (4, 64):
            for tag, kw in (("uniform", {}), ("logit", {"logits_normal": True}),
                            ("logit_shift", {"logits_normal": True, "shift": 4.63}), ("xpred", {"prediction_type": "x"})):
                torch.manual_seed(seed)
                assert np.array_equal(t2n(Flow(n_steps=10, **kw).draw_timesteps(B)), g[f"draw_flow_{tag}_s{seed}_b{B}"])
            torch.manual_seed(seed)
            got = GaussianDiffusion(n_steps=1000).draw_timesteps(B)
            assert got.dtype == torch.int32 and np.array_equal(t2n(got), g[f"draw_ddpm_s{seed}_b{B}"])
    with pytest.raises(NotImplementedError):
        Flow(n_steps=4).set_steps(4, schedule="cosine")
    with pytest.raises(AssertionError):
        Flow(n_steps=4, prediction_type="eps")


def test_gaussian_tables_and_respacing_match_reference(golden, host_exact):
    from oracle import diffusion as od

    g = golden("schedules")
    for sched in ("linear", "cosine"):
        d = GaussianDiffusion(n_steps=1000, schedule=sched)
        # (tables behind a sqrt / log: the oracle -- the reference's formulas, test_oracle_golden.py -- on this host's math)
        T = od.GaussianTables(1000, schedule=sched)
        for nm in ("betas", "alphas_bar"):
            assert np.array_equal(t2n(getattr(d, nm)), g[f"gd_{sched}_{nm}"]), nm
        assert host_exact(d.sqrt_alphas_bar, g[f"gd_{sched}_sqrt_alphas_bar"], T.sqrt_alphas_bar)
        for nm in ("alphas_bar_prev", "posterior_variance"):
            assert np.array_equal(t2n(getattr(d.sampler, nm)), g[f"gd_{sched}_{nm}"]), nm
        for nm in ("posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"):
            assert host_exact(getattr(d.sampler, nm), g[f"gd_{sched}_{nm}"], getattr(T, nm)), nm
    for n in (50, 100, 250):
        d = GaussianDiffusion(n_steps=1000)
        d.set_steps(n)
        assert np.array_equal(np.array(d.timestep_map), g[f"respace_{n}_map"])
        assert np.array_equal(t2n(d.betas), g[f"respace_{n}_betas"])
        assert np.array_equal(t2n(d.sampler.posterior_variance), g[f"respace_{n}_postvar"])
    d = GaussianDiffusion(n_steps=1000)
    d.set_steps(30, section_counts="10,10,10")
    assert np.array_equal(np.array(d.timestep_map), g["respace_sections_map"])
    assert np.array_equal(np.array(sorted(space_timesteps(1000, 10))), g["space_1000_10"])
    with pytest.raises(ValueError):
        space_timesteps(1000, 10, ddim=True)
    with pytest.raises(ValueError):
        space_timesteps(10, "6,6")
    with pytest.raises(ValueError):
        GaussianDiffusion(n_steps=10, sampling_method="euler")
    with pytest.raises(NotImplementedError):
        GaussianDiffusion(n_steps=10, schedule="sigmoid")


def test_rope_tables_match_reference(golden):
    g = golden("prims")
    c, s = rope_grid_tables(16, 16, [32, 32], 10_000.0)
    assert np.array_equal(t2n(c), g["rope_cos_16x16"]) and np.array_equal(t2n(s), g["rope_sin_16x16"])
    c, s = rope_grid_tables(3, 5, [8, 24], 2000.0)
    assert np.array_equal(t2n(c), g["rope_cos_3x5"]) and np.array_equal(t2n(s), g["rope_sin_3x5"])


def test_module_contract_and_layout():
    kw = dict(simple_dit=True, input_channels=4, inner_dim=384, embedding_dim=384, num_heads=6, patch_size=2, depth=12,
              n_classes=1000, classifier_free=True)
    m = MMDiT(**kw)
    assert sum(p.numel() for p in m.parameters()) == 39_922_576  # SURVEY.md Appendix B (DiT-S/2 dims)
    lay = ParamLayout(m.dims)
    named = dict(m.named_parameters())
    assert set(named) == set(lay.entries)
    spans = sorted((off, off + int(np.prod(shape))) for off, shape in lay.entries.values())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "overlapping parameters in the arena"
    assert all(off % 4 == 0 for off, _ in lay.entries.values())
    # the adaLN matrices are one contiguous [L*6D+2D, E] block
    first = lay.entries["layers.0.modulation.lin.weight"][0]
    last_off, last_shape = lay.entries["last_layer.adaLN_modulation.1.weight"]
    assert last_off + int(np.prod(last_shape)) - first == lay.mod_rows * 384
    # reference init: zero adaLN, xavier elsewhere
    assert float(m.layers[3].modulation.lin.weight.detach().abs().sum()) == 0.0
    assert float(m.layers[3].attention.qkv.weight.detach().abs().sum()) > 0.0
    # deep copies (EMA) keep parameters, drop the engine
    m2 = copy.deepcopy(m)
    assert m2._engine is None and torch.equal(m2.conv_proj.weight, m.conv_proj.weight)
    # unsupported reference modes fail loudly, never silently fall back
    with pytest.raises(AssertionError):  # the reference's own assertion (mmdit.py:642): joint blocks need a context embedder
        MMDiT(simple_dit=False)
    from diffulab_amd.networks.embedders import PrecomputedEmbedder

    emb = PrecomputedEmbedder(torch.zeros(1, 16, 96), null_embedding_seq_len=3)
    assert emb.n_output == 1 and emb.output_size == (96,) and int(emb.null_embedding_mask.sum()) == 3
    # the per-(device, dtype) copy of the null embedding follows IN-PLACE updates of the attribute (the reference converts per call)
    ctx = {"embeddings": torch.ones(2, 16, 96), "attn_mask": torch.ones(2, 16, dtype=torch.bool)}
    assert float(emb.drop_conditions(ctx, 1.0)["embeddings"].abs().sum()) == 0.0
    emb.null_embedding.add_(2.0)
    assert bool((emb.drop_conditions(ctx, 1.0)["embeddings"] == 2.0).all())
    emb.null_embedding_mask[:] = True
    assert bool(emb.drop_conditions(ctx, 1.0)["attn_mask"].all())
    emb.null_embedding.zero_()
    jkw = dict(simple_dit=False, context_embedder=emb, input_channels=4, inner_dim=128, embedding_dim=64, num_heads=2, patch_size=2,
               depth=2, rope_axes_dim=[16, 24, 24])
    mj = MMDiT(**jkw)
    assert mj.context_embed.weight.shape == (128, 96) and hasattr(mj.layers[0], "modulation_context")
    ms = MMDiT(**{**jkw, "n_single_stream_blocks": 1})  # the last block of the stack becomes a single-stream block
    assert hasattr(ms.layers[0], "modulation_context") and hasattr(ms.layers[1], "mlp") and ms.layers[1].modulation[1].out_features == 384
    with pytest.raises(NotImplementedError):  # the reference's default 3-axis split (64 // 3 = 21, odd) is not a valid RoPE width
        MMDiT(**{**jkw, "rope_axes_dim": None})
    with pytest.raises(NotImplementedError):
        DiTDims(inner_dim=384, num_heads=4).validate()
    with pytest.raises(RuntimeError):
        m(x=torch.zeros(1, 4, 32, 32), timesteps=torch.zeros(1), y=torch.zeros(1, dtype=torch.long))  # CPU: no fallback


def _layout_cases():
    from diffulab_amd.networks.denoisers import DDT, SprintDiT
    from diffulab_amd.networks.embedders import PrecomputedEmbedder

    emb = PrecomputedEmbedder(torch.zeros(1, 16, 96), null_embedding_seq_len=3)
    small = dict(input_channels=4, inner_dim=128, num_heads=2, patch_size=2)
    joint = dict(simple_dit=False, context_embedder=emb, embedding_dim=64, rope_axes_dim=[16, 24, 24], **small)
    return {
        "dit": lambda: MMDiT(simple_dit=True, embedding_dim=64, depth=2, n_classes=10, classifier_free=True, **small),
        "sprint": lambda: SprintDiT(simple_dit=True, embedding_dim=64, encoder_depth=1, deep_layers_depth=2, decoder_depth=1,
                                    n_classes=10, classifier_free=True, **small),
        "ddt": lambda: DDT(simple_ddt=True, encoder_depth=2, decoder_depth=1, n_classes=10, classifier_free=True, **small),
        "mmdit_joint": lambda: MMDiT(depth=2, **joint),
        "mmdit_joint_stack": lambda: MMDiT(depth=3, n_single_stream_blocks=1, **joint),
        "sprint_joint": lambda: SprintDiT(encoder_depth=1, deep_layers_depth=2, n_single_stream_blocks=1, decoder_depth=1, **joint),
        "ddt_joint": lambda: DDT(encoder_depth=2, decoder_depth=1, context_embedder=emb, rope_axes_dim=[16, 24, 24], **small),
    }


@pytest.mark.parametrize("form", ["dit", "sprint", "ddt", "mmdit_joint", "mmdit_joint_stack", "sprint_joint", "ddt_joint"])
def test_every_bf16_layout_matches_its_module(form):
    """the arena layout of every bf16 engine names exactly the module's parameters, places them without overlap on 4-float
    boundaries, and keeps the stacked adaLN matrix (and DDT's per-token one) contiguous"""
    m = _layout_cases()[form]()
    lay = m._make_engine(torch.device("meta")).layout
    assert set(dict(m.named_parameters())) == set(lay.entries)
    for name, p in m.named_parameters():
        assert tuple(p.shape) == tuple(lay.entries[name][1]), name
    spans = sorted((off, off + int(np.prod(shape))) for off, shape in lay.entries.values())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "overlapping parameters in the arena"
    assert all(off % 4 == 0 for off, _ in lay.entries.values()) and spans[-1][1] <= lay.size and lay.size % 64 == 0
    E = m.dims.embedding_dim
    for w0, rows in ((lay.mod_w0, lay.mod_rows), (getattr(lay, "tmod_w0", None), getattr(lay, "tmod_rows", 0))):
        if w0 is None:
            continue
        first = lay.entries[w0][0]
        inside = sorted((off, int(np.prod(shape))) for off, shape in lay.entries.values() if first <= off < first + rows * E)
        assert sum(n for _, n in inside) == rows * E, "adaLN matrix rows are not one contiguous block"
        assert all(a[0] + a[1] == b[0] for a, b in zip(inside, inside[1:]))


def test_bench_launches_its_own_ranks_without_touching_a_gpu():
    """`python bench.py --gpus N` (no external launcher): the parent spawns N children with RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_* set on 127.0.0.1, never initialises the HIP runtime itself and returns the children's status."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "3", "--launch-check"], capture_output=True,
                         text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = sorted((json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")), key=lambda r: r["rank"])
    assert [r["rank"] for r in rows] == [0, 1, 2] and [r["local_rank"] for r in rows] == [0, 1, 2]
    assert all(r["world"] == 3 and r["master"] == "127.0.0.1" and not r["cuda_initialized"] for r in rows)
    assert len({r["port"] for r in rows}) == 1
    # a failing rank is the launcher's exit status
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--launch-check", "--steps", "x"],
                         capture_output=True, text=True, timeout=300, env=env)
    assert bad.returncode != 0


def test_bench_dump_outputs_is_a_fixed_float32_sample(tmp_path, monkeypatch):
    """`bench.py --dump-outputs DIR`: the last step's loss and the same seeded positions of its parameters, gradients and EMA copy
    (parameters concatenated in name order) as float32 .npy files, identical from call to call and under 64 MB at full size;
    `--steps` below 1 is refused before anything runs."""
    import subprocess
    import sys
    import types

    import bench

    assert 3 * bench.DUMP_SAMPLE * 4 + 4 <= 64 * 2**20
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.Linear(32, 8))
    m(torch.randn(4, 16)).square().mean().backward()
    ema = types.SimpleNamespace(ema_model=copy.deepcopy(m))
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    bench.dump_outputs(str(tmp_path / "a"), 0.25, m, ema)
    bench.dump_outputs(str(tmp_path / "b"), 0.25, m, ema)
    assert sorted(os.listdir(tmp_path / "a")) == ["ema_params.npy", "grads.npy", "loss.npy", "params.npy"]
    got = {}
    for name in os.listdir(tmp_path / "a"):
        a, b = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert a.dtype == np.float32 and np.array_equal(a, b), name
        got[name[:-4]] = a
    named = sorted(m.named_parameters())
    idx = torch.randperm(sum(p.numel() for _, p in named), generator=torch.Generator().manual_seed(0))[:100].sort().values
    assert np.array_equal(got["params"], torch.cat([p.detach().reshape(-1) for _, p in named])[idx].numpy())
    assert np.array_equal(got["grads"], torch.cat([p.grad.reshape(-1) for _, p in named])[idx].numpy())
    assert np.array_equal(got["ema_params"], got["params"]) and got["loss"].tolist() == [0.25]

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "0", "--launch-check"], capture_output=True,
                         text=True, timeout=300)
    assert bad.returncode == 2 and "--steps" in bad.stderr


def test_fused_adamw_flat_arena_detection_is_cached_and_revalidated():
    """FusedAdamW._flat (round 5): the arena scan is remembered per group and a hit is re-validated by pointer compares -- a gradient
    that was detached, re-pointed or newly attached is seen at the next call (host logic only: no kernel runs here)"""
    from diffulab_amd.training.optim import FusedAdamW

    flat, gflat = torch.zeros(64), torch.zeros(64)
    ps = []
    for i in range(4):
        p = torch.nn.Parameter(torch.empty(0))
        p.data = flat[16 * i : 16 * (i + 1)]
        p.grad = gflat[16 * i : 16 * (i + 1)]
        ps.append(p)
    extra = torch.nn.Parameter(torch.zeros(3))  # outside the arena (an auxiliary head in the same group), no gradient yet
    opt = FusedAdamW(ps + [extra], lr=1e-3)
    g = opt.param_groups[0]
    scans = []
    orig = opt._flat_scan
    opt._flat_scan = lambda group: (scans.append(1), orig(group))[1]
    pb, gb, rest = opt._flat(g)
    assert pb.data_ptr() == flat.data_ptr() and gb.data_ptr() == gflat.data_ptr() and rest == [extra] and len(scans) == 1
    assert opt._flat(g)[2] == [extra] and len(scans) == 1            # hit: no rescan
    extra.grad = torch.zeros(3)                                       # an outside tensor gains a gradient: rescan (it might be a view)
    assert opt._flat(g)[2] == [extra] and len(scans) == 2
    assert opt._flat(g) is not None and len(scans) == 2
    ps[2].grad = None                                                 # a detached gradient: the arena no longer holds the whole group
    r = opt._flat(g)
    assert len(scans) == 3 and (r is None or ps[2] in r[2])
    ps[2].grad = gflat[32:48]
    assert opt._flat(g)[2] == [extra] and len(scans) == 4
    ps[1].grad = torch.zeros(16)                                      # re-pointed outside the gradient arena
    assert opt._flat(g) is None and len(scans) == 5
