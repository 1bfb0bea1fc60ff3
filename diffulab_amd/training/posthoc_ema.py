"""Post-hoc EMA (Karras et al. 2024, "Analyzing and Improving the Training Dynamics of Diffusion Models", sec. 3.2 and app. C).

During training ``PowerEMA`` (training/ema.py) tracks power-function EMA profiles and snapshots them now and then; afterwards the
EMA of ANY relative width at any snapshot time is the least-squares combination of the stored snapshots.  This project's own: the
reference tracks one classic EMA whose length is fixed before the run.

Profile of exponent gamma at time t:   p_{t,gamma}(tau) = (gamma + 1) tau^gamma / t^(gamma + 1)   on [0, t]
relative width (std of p / t):         sigma_rel = sqrt(gamma + 1) / ((gamma + 2) sqrt(gamma + 3))
running form:                          ema_t = beta_t ema_{t-1} + (1 - beta_t) theta_t,  beta_t = (1 - 1/t)^(gamma + 1)

The math below is fp64 numpy on the host; the only device work is in ``synthesize``: staging arenas filled from the snapshot files
and one ``dl_arena_lincomb`` launch per group of snapshots into the model's flat parameter arena.
"""

from __future__ import annotations

import json
import math
import os

import numpy as np

SIGMA_REL_MAX = 0.28  # sigma_rel -> 1 / sqrt(12) = 0.2887 as gamma -> 0 (the uniform average); wider profiles do not exist
INDEX_NAME = "phema_index.jsonl"


def snapshot_name(t: int, sigma_rel: float) -> str:
    return f"phema_{int(t):09d}_{float(sigma_rel):.3f}.pt"


# ---------------------------------------------------------------------------------------------------------------- profiles
def gamma_to_sigma_rel(gamma: float) -> float:
    g = float(gamma)
    return math.sqrt(g + 1.0) / ((g + 2.0) * math.sqrt(g + 3.0))


def sigma_rel_to_gamma(sigma_rel: float) -> float:
    """the largest real root of g^3 + 7 g^2 + (16 - s^-2) g + (12 - s^-2) (sigma_rel^2 (g + 2)^2 (g + 3) = g + 1, expanded), polished
    by Newton steps on the closed form so that the round trip holds to the last bits"""
    s = float(sigma_rel)
    if not 0.0 < s < SIGMA_REL_MAX:
        raise ValueError(f"sigma_rel must lie in (0, {SIGMA_REL_MAX}), got {sigma_rel!r}")
    t = s ** -2
    roots = np.roots([1.0, 7.0, 16.0 - t, 12.0 - t])
    g = float(max(r.real for r in roots if abs(r.imag) < 1e-9 * max(1.0, abs(r.real))))
    for _ in range(4):  # f(g) = sigma_rel(g) - s, decreasing in g on g > 0
        h = 1e-6 * max(1.0, abs(g))
        d = (gamma_to_sigma_rel(g + h) - gamma_to_sigma_rel(g - h)) / (2.0 * h)
        step = (gamma_to_sigma_rel(g) - s) / d
        g -= step
        if abs(step) <= 1e-15 * max(1.0, abs(g)):
            break
    return g


def ema_weight(t: int, gamma: float) -> float:
    """1 - beta_t = 1 - (1 - 1/t)^(gamma + 1) of update number t (counted from 1: the first update is a copy), formed in fp64 without
    the cancellation of `1 - beta` and rounded to f32 once -- the value `dl_ema_update_multi` takes"""
    t = int(t)
    if t < 1:
        raise ValueError(f"t counts updates from 1, got {t}")
    if t == 1:
        return 1.0
    return float(np.float32(-math.expm1((float(gamma) + 1.0) * math.log1p(-1.0 / t))))


def power_function_correlation(t_a, g_a, t_b, g_b):
    """integral over tau of p_{t_a,g_a}(tau) p_{t_b,g_b}(tau); broadcasts over numpy arrays.  With the shorter profile called a:
    (g_a + 1)(g_b + 1) (t_a / t_b)^g_b / ((g_a + g_b + 1) t_b)"""
    t_a, g_a, t_b, g_b = (np.asarray(v, dtype=np.float64) for v in (t_a, g_a, t_b, g_b))
    swap = t_a > t_b
    ts, gs = np.where(swap, t_b, t_a), np.where(swap, g_b, g_a)  # the shorter profile
    tl, gl = np.where(swap, t_a, t_b), np.where(swap, g_a, g_b)  # the longer one
    out = (gs + 1.0) * (gl + 1.0) * (ts / tl) ** gl / ((gs + gl + 1.0) * tl)
    return out if out.ndim else float(out)


def solve_posthoc_coefficients(in_t, in_sigma, out_t, out_sigma) -> np.ndarray:
    """X = solve(A, B): A the correlation of the stored snapshots (times in_t, widths in_sigma) with themselves, B their
    correlation with the targets.  -> [n_in] for a scalar target, [n_in, n_out] otherwise"""
    in_t = np.atleast_1d(np.asarray(in_t, dtype=np.float64))
    in_g = np.array([sigma_rel_to_gamma(s) for s in np.atleast_1d(in_sigma)], dtype=np.float64)
    if in_t.shape != in_g.shape or in_t.size == 0:
        raise ValueError(f"in_t and in_sigma must be equally long and not empty (got {in_t.size} and {in_g.size})")
    scalar = np.ndim(out_t) == 0 and np.ndim(out_sigma) == 0
    out_t_, out_s_ = np.broadcast_arrays(np.atleast_1d(np.asarray(out_t, dtype=np.float64)), np.atleast_1d(np.asarray(out_sigma, dtype=np.float64)))
    out_g = np.array([sigma_rel_to_gamma(s) for s in out_s_], dtype=np.float64)
    A = power_function_correlation(in_t[:, None], in_g[:, None], in_t[None, :], in_g[None, :])
    B = power_function_correlation(in_t[:, None], in_g[:, None], out_t_[None, :], out_g[None, :])
    X = np.linalg.solve(A, B)
    return X[:, 0] if scalar else X


# ---------------------------------------------------------------------------------------------------------------- synthesis
def read_index(snapshot_dir) -> list[dict]:
    path = os.path.join(os.fspath(snapshot_dir), INDEX_NAME)
    if not os.path.exists(path):
        raise ValueError(f"snapshot_dir: no {INDEX_NAME} in {os.fspath(snapshot_dir)!r}")
    with open(path) as f:
        rows = [json.loads(line) for line in f if line.strip()]
    seen = {}
    for r in rows:  # (a resumed run may have written a time twice: the later line wins)
        seen[(int(r["t"]), f"{float(r['sigma_rel']):.3f}")] = r
    return sorted(seen.values(), key=lambda r: (int(r["t"]), float(r["sigma_rel"])))


def select_snapshots(rows: list[dict], t: int | None) -> tuple[list[dict], int]:
    """the index rows a synthesis at time `t` (None: the last snapshot time) may use, and that time"""
    if not rows:
        raise ValueError("snapshot_dir: the snapshot index is empty")
    last = max(int(r["t"]) for r in rows)
    if t is None:
        t = last
    t = int(t)
    if t < 1:
        raise ValueError(f"t must be a positive update count, got {t}")
    if t > last:
        raise ValueError(f"t = {t} is later than the last snapshot (t = {last}): an EMA cannot be synthesised ahead of its snapshots")
    return [r for r in rows if int(r["t"]) <= t], t


def synthesize(model, snapshot_dir, sigma_rel: float, t: int | None = None, group: int = 8) -> np.ndarray:
    """Write the EMA of relative width `sigma_rel` at update `t` (None: the last snapshot) into `model`'s parameter arena as the
    least-squares combination of the snapshots under `snapshot_dir`; -> the fp64 coefficient vector, in the order of
    `select_snapshots(read_index(snapshot_dir), t)`.  Snapshots are staged on the device `group` at a time in the arena's layout and
    combined by one `dl_arena_lincomb` launch per group, each after the first continuing the chain of the one before, so the result
    does not depend on `group`.  Buffers that are not parameters come from the latest snapshot used."""
    import torch

    from .. import ops
    from ..engine import bump_param_epoch

    sigma_rel_to_gamma(sigma_rel)  # (range check first: names the argument)
    if int(group) < 1:
        raise ValueError(f"group must be >= 1, got {group}")
    group = min(int(group), ops.LINCOMB_MAX_SOURCES)
    rows, t = select_snapshots(read_index(snapshot_dir), t)
    coef = solve_posthoc_coefficients([r["t"] for r in rows], [r["sigma_rel"] for r in rows], t, sigma_rel)
    if not hasattr(model, "engine"):
        raise ValueError(f"model: {type(model).__name__} has no flat parameter arena to synthesise into")
    layout, flat = model.engine.layout, model._flat
    n = flat.numel()
    staging = torch.empty(min(group, len(rows)), n, device=flat.device, dtype=torch.float32)
    known = set(model.state_dict())
    latest = None
    with torch.no_grad():
        for g0 in range(0, len(rows), group):
            chunk = rows[g0:g0 + group]
            for slot, r in enumerate(chunk):
                sd = torch.load(os.path.join(os.fspath(snapshot_dir), r["file"]), weights_only=True, map_location="cpu")
                extra = sorted(k for k, v in sd.items() if torch.is_tensor(v) and k not in known)
                if extra:
                    raise ValueError(f"snapshot_dir: {r['file']} does not match the model: it holds {extra[0]!r} (and {len(extra) - 1} more), which the model lacks")
                stage = staging[slot].zero_()  # (alignment gaps of the layout stay 0 in every source, hence in the sum)
                for name in layout.entries:
                    view = layout.view(stage, name)
                    if name not in sd or tuple(sd[name].shape) != tuple(view.shape):
                        got = tuple(sd[name].shape) if name in sd else None
                        raise ValueError(f"snapshot_dir: {r['file']} does not match the model at {name!r}: shape {got}, the model has {tuple(view.shape)}")
                    view.copy_(sd[name])
                latest = sd
            ops.arena_lincomb(flat, [staging[s] for s in range(len(chunk))], coef[g0:g0 + len(chunk)], accumulate=g0 > 0)
        for name, buf in model.named_buffers():
            if latest is not None and name in latest:
                buf.copy_(latest[name])
    bump_param_epoch()
    return coef
