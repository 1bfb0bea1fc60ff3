"""CPU checks of the UNet's dropout: the Philox mask definition (tests/dropout_common.py) against known answers, the host-side
threshold / scale, what ``UNetModel(dropout=p)`` accepts and refuses, the site numbering against the reference fixture, the
data-parallel seed rule, and the refusals of ``dl_dropout`` (validated before any device call, so testable with no GPU)."""

import ctypes
import re

import numpy as np
import pytest
import torch

import dropout_common as dc

SMALL = dict(image_size=[16, 16], in_channels=1, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=[2],
             channel_mult="1, 2", num_heads=2, use_scale_shift_norm=True, resblock_updown=True, n_classes=10, classifier_free=True)


# ------------------------------------------------------------------ 1. the mask definition
@pytest.mark.parametrize("counter,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, out):
    assert " ".join("%08x" % int(w[0]) for w in dc.philox4x32_10(counter, key)) == out


def test_mask_known_answer_and_word_halves():
    keep = dc.keep_mask(2, 8, seed=1234, step=0, site=0, p=0.3).reshape(-1).astype(int).tolist()
    assert keep == [1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0]
    # lane j of group g reads word j >> 1: the low half for even j, the high half for odd
    w = dc.philox4x32_10((3, 0, 5, 7), (1234, 0))
    h = dc.halves(32, seed=1234, step=7, site=5)[24:32]
    assert [int(v) for v in h] == [int(w[j >> 1][0]) >> (16 * (j & 1)) & 0xFFFF for j in range(8)]
    # the element index is the LOGICAL one: the mask of [rows, cols] is the flat mask reshaped, whatever the pitch
    assert np.array_equal(dc.keep_mask(6, 16, 9, 2, 3, 0.5).reshape(-1), dc.keep_mask(1, 96, 9, 2, 3, 0.5).reshape(-1))


def test_keep_fraction_and_independence():
    n = 1 << 20
    for p in (0.1, 0.3, 0.5):
        q = 1.0 - dc.threshold(p) / 65536.0
        sigma = np.sqrt(q * (1.0 - q) / n)
        for step in range(3):
            for site in (0, 1, 7):
                f = dc.keep_mask(n // 8, 8, 1234, step, site, p).mean()
                assert abs(f - q) <= 1.9 * sigma, (p, step, site, f, q)
    a = dc.keep_mask(n // 8, 8, 1234, 0, 0, 0.3)
    for seed, step, site in ((1234, 1, 0), (1234, 0, 1), (1235, 0, 0), (1234 + (1 << 32), 0, 0), (1234, 1 << 32, 0)):
        agree = (a == dc.keep_mask(n // 8, 8, seed, step, site, 0.3)).mean()
        if step == 1 << 32:  # the counter carries the low word of the step only
            assert agree == 1.0
        else:  # independence: 0.7^2 + 0.3^2 = 0.58
            assert 0.5785 <= agree <= 0.5815, (seed, step, site, agree)


# ------------------------------------------------------------------ 2. threshold and scale
def test_threshold_and_scale():
    from diffulab_amd import ops

    for p, T in ((0.1, 6554), (0.3, 19661), (0.5, 32768)):
        assert ops.dropout_threshold(p) == T == dc.threshold(p)
        assert np.float32(ops.dropout_scale(p)) == np.float32(1.0 / (1.0 - p)) == dc.scale_of(p)
    assert ops.dropout_threshold(0.0) == 0  # nothing can be dropped: the engine launches nothing
    assert 0 < ops.dropout_threshold(0.999999) < 65536
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.dropout_threshold(bad)
        with pytest.raises(ValueError):
            ops.dropout_scale(bad)


# ------------------------------------------------------------------ 3. construction
def test_model_construction():
    from diffulab_amd.networks.denoisers import UNetModel
    from unet_context_common import C_CTX, CASES, ChannelFirstEmbedder

    m = UNetModel(dropout=0.1, **SMALL)
    assert m.dims.dropout == 0.1 and m.training and m.dropout_active
    drops = [mod for mod in m.modules() if isinstance(mod, torch.nn.Dropout)]
    assert drops and all(mod.p == 0.1 for mod in drops)
    assert not m.eval().dropout_active and m.train().dropout_active
    plain = UNetModel(**SMALL)
    assert not plain.dropout_active and plain.dims.dropout == 0.0
    assert list(m.state_dict()) == list(plain.state_dict())
    assert all(m.state_dict()[k].shape == v.shape for k, v in plain.state_dict().items())
    for bad in (-0.1, 1.0, 2):
        with pytest.raises(ValueError, match="dropout"):
            UNetModel(dropout=bad, **SMALL)
    with pytest.raises(NotImplementedError, match="dropout.*TransformerBlock"):
        UNetModel(context_embedder=ChannelFirstEmbedder(C_CTX), dropout=0.1, **CASES["d1"])
    assert UNetModel(context_embedder=ChannelFirstEmbedder(C_CTX), dropout=0.0, **CASES["d1"]).dims.dropout == 0.0
    # unconditional: built too
    assert UNetModel(dropout=0.2, **dict(SMALL, n_classes=None, classifier_free=False)).dropout_active


def test_seed_and_step_bookkeeping():
    from diffulab_amd.networks.denoisers import UNetModel

    m = UNetModel(dropout=0.3, **SMALL)
    assert m._dropout_seed is None and m._dropout_step == 0
    m.set_dropout_seed(1234)
    assert (m._dropout_seed, m._dropout_step) == (1234, 0)
    m.set_dropout_seed(7, step=5)
    assert (m._dropout_seed, m._dropout_step) == (7, 5)


# ------------------------------------------------------------------ 4. sites and seeds
def test_sites_match_the_plan_and_the_reference_fixture(golden):
    from diffulab_amd.networks.denoisers import UNetModel
    from diffulab_amd.unet_engine import build_plan, dropout_sites

    g = golden("unet_dropout")
    m = UNetModel(dropout=float(g["p"]), **SMALL)
    blocks = build_plan(m.dims).all_blocks()
    sites = dropout_sites(build_plan(m.dims))
    assert sites == {b.prefix: i for i, b in enumerate(blocks) if b.kind in ("res", "attn")}
    assert len(set(sites.values())) == len(sites) == sum(b.kind in ("res", "attn") for b in blocks)
    fixture = dict(zip(g["site_prefixes"].tolist(), g["site_ids"].tolist()))
    for prefix in sorted(set(sites) | set(fixture)):
        assert sites.get(prefix) == fixture.get(prefix), f"site of {prefix}: {sites.get(prefix)} here, {fixture.get(prefix)} in the fixture"
    # every site is a block that owns an nn.Dropout of the module tree
    mods = dict(m.named_modules())
    for prefix in sites:
        owner = mods[prefix[:-1]]
        assert sum(isinstance(c, torch.nn.Dropout) for c in owner.modules()) == 1, prefix
    assert (float(g["p"]), int(g["seed"]), int(g["step"])) == (dc.FIXTURE_P, dc.FIXTURE_SEED, dc.FIXTURE_STEP)


def test_rank_seeds_differ():
    from diffulab_amd.networks.denoisers.unet import dropout_rank_seed

    assert dropout_rank_seed(1234, 0) == 1234 and dropout_rank_seed(1234, 1) == 1235
    assert dropout_rank_seed((1 << 64) - 1, 1) == 0  # wraps inside the 64-bit key
    a = dc.keep_mask(4096, 8, dropout_rank_seed(1234, 0), 0, 3, 0.3)
    b = dc.keep_mask(4096, 8, dropout_rank_seed(1234, 1), 0, 3, 0.3)
    assert 0.56 < (a == b).mean() < 0.60


# ------------------------------------------------------------------ 5. the C entry point refuses what is out of contract
def test_dl_dropout_refuses_out_of_contract_arguments():
    from diffulab_amd import _lib

    L = _lib.lib()
    assert "dl_dropout" in L.protos
    fn = L._fns["dl_dropout"][0]
    c = L.cdll
    buf = ctypes.create_string_buffer(4096)
    base = (ctypes.addressof(buf) + 255) & ~255
    INVALID = int(re.search(r"\bDL_ERR_INVALID\s*=\s*(-?\d+)", open(_lib.HEADER_PATH).read()).group(1))

    def call(x=base, ldx=16, resid=base, ldr=16, out=base, ldo=16, rows=4, cols=16, dtype=0, rng=base, site=0, T=100, scale=1.5):
        return fn(x, ldx, resid, ldr, out, ldo, rows, cols, dtype, rng, site, T, scale, None)

    cases = {
        "cols = 12": dict(cols=12, ldx=16, ldo=16),
        "ldx below cols": dict(ldx=8),
        "ldo below cols": dict(ldo=8),
        "ldr below cols": dict(ldr=8),
        "ldx = 20": dict(ldx=20),
        "ldr = 20": dict(ldr=20),
        "ldo = 20": dict(ldo=20),
        "T = 65536": dict(T=65536),
        "T < 0": dict(T=-1),
        "unaligned x": dict(x=base + 8),
        "unaligned out": dict(out=base + 2),
        "unaligned resid": dict(resid=base + 4),
        "unknown dtype": dict(dtype=2),
        "null x": dict(x=None),
        "null state": dict(rng=None),
        "rows = 0": dict(rows=0),
        "rows * cols = 2^40": dict(rows=1 << 36, ldx=16),
    }
    for what, kw in cases.items():
        rc = call(**kw)
        msg = c.dl_last_error().decode()
        assert rc == INVALID, (what, rc, msg)
        assert "dl_dropout" in msg, (what, msg)


# ------------------------------------------------------------------ 6. the fixture is not vacuous
def test_fixture_differs_from_the_p0_fixture(golden):
    g, g0 = golden("unet_dropout"), golden("unet")
    a, b = g["un_pred"].astype(np.float64), g0["un_pred"].astype(np.float64)
    d = np.linalg.norm(a - b) / np.linalg.norm(b)
    print(f"relative L2 distance of the dropout fixture's prediction to the p = 0 fixture's: {d:.4f}")
    assert d > 0.1  # five times the 2e-2 bar of the bf16 whole-model test: a run that ignored the masks cannot pass
    assert g["un_grad_names"].tolist() == g0["un_grad_names"].tolist()
    held = {k for k in g0 if k.startswith("un_")}
    assert held == {k for k in (set(g) | set(golden("unet_dropout_wide"))) if k.startswith("un_")}
