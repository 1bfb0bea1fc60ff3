"""Post-hoc EMA (Karras et al. 2024, sec. 3.2 / app. C) restated in fp64 numpy, independent of the package: what the host math, the two
kernels of csrc/ema.hip and the classes built on them are judged against.  Nothing here imports diffulab_amd."""

from __future__ import annotations

import numpy as np

U = 2.0 ** -24  # unit roundoff of f32


# ---------------------------------------------------------------------------------------------------------------- profiles
def sigma_rel_of(gamma: float) -> float:
    return np.sqrt(gamma + 1.0) / ((gamma + 2.0) * np.sqrt(gamma + 3.0))


def gamma_of(sigma_rel: float) -> float:
    """bisection on the closed form (sigma_rel falls monotonically from 1 / sqrt(12) at gamma = 0): no polynomial, no root finder"""
    lo, hi = 0.0, 1e6
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if sigma_rel_of(mid) > sigma_rel:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def profile(tau, t: float, gamma: float):
    """p_{t,gamma}(tau) on [0, t], zero beyond"""
    tau = np.asarray(tau, dtype=np.float64)
    return np.where(tau <= t, (gamma + 1.0) * tau ** gamma / t ** (gamma + 1.0), 0.0)


def correlation_quadrature(t_a, g_a, t_b, g_b, points: int = 200_001) -> float:
    """trapezoid rule for the integral of p_a p_b over [0, min(t_a, t_b)], where both are non-zero"""
    tau = np.linspace(0.0, min(t_a, t_b), points)
    f = profile(tau, t_a, g_a) * profile(tau, t_b, g_b)
    h = tau[1] - tau[0]
    return float(h * (f.sum() - 0.5 * (f[0] + f[-1])))


def correlation(t_a, g_a, t_b, g_b) -> float:
    if t_a > t_b:
        t_a, g_a, t_b, g_b = t_b, g_b, t_a, g_a
    return (g_a + 1.0) * (g_b + 1.0) * (t_a / t_b) ** g_b / ((g_a + g_b + 1.0) * t_b)


def weight64(t: int, gamma: float) -> float:
    """1 - (1 - 1/t)^(gamma + 1) in fp64 (not yet rounded to f32)"""
    return 1.0 if t == 1 else float(-np.expm1((gamma + 1.0) * np.log1p(-1.0 / t)))


def weight32(t: int, gamma: float) -> float:
    return float(np.float32(weight64(t, gamma)))


def coefficients(in_t, in_sigma, out_t, out_sigma) -> np.ndarray:
    in_g = [gamma_of(s) for s in in_sigma]
    n = len(in_t)
    A = np.array([[correlation(in_t[i], in_g[i], in_t[j], in_g[j]) for j in range(n)] for i in range(n)])
    B = np.array([correlation(in_t[i], in_g[i], out_t, gamma_of(out_sigma)) for i in range(n)])
    return np.linalg.solve(A, B), A


# ---------------------------------------------------------------------------------------------------------------- kernels
def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def ema_step_ref(ema, p, w: float):
    """ema' = ema + w (p - ema) on f32 operands held in fp64 -> (exact value, bound).  The expression as written rounds three times:
    the difference (relative U of |p - ema|, carried through the product: U |d|), the product (U |d|) and the sum (U |o|); a fused
    multiply-add drops the middle one, which the bound still admits.  (1 + U)^2 covers the second-order terms."""
    E, P = np.asarray(ema, dtype=np.float64), np.asarray(p, dtype=np.float64)
    d = float(w) * (P - E)
    o = E + d
    return o, U * (2.0 * np.abs(d) + np.abs(o)) * (1.0 + U) ** 2 + 2.0 ** -149


def lincomb_ref(srcs, weights, start=None):
    """out = [start +] sum_k w_k src_k -> (exact value, bound).  A length-K chain acc = fma(w_k, src_k, acc) is a recursive sum of K
    exact products with one rounding per step: every term passes through at most K roundings, so (Higham, Accuracy and Stability of
    Numerical Algorithms, sec. 4.2) |out - exact| <= gamma_K sum_k |w_k src_k|, gamma_K = K U / (1 - K U).  The test uses gamma_{K+1}:
    (K + 1) U sum / (1 - (K + 1) U), which also covers a chain that starts from a stored value."""
    K = len(srcs)
    acc = np.zeros_like(np.asarray(srcs[0], dtype=np.float64)) if start is None else np.asarray(start, dtype=np.float64).copy()
    mag = np.abs(acc)
    for w, s in zip(weights, srcs):
        term = float(np.float32(w)) * np.asarray(s, dtype=np.float64)
        acc = acc + term
        mag = mag + np.abs(term)
    g = (K + 1) * U
    return acc, g * mag / (1.0 - g) + 2.0 ** -149


def alternating_weights(K: int, total: float = 10.0) -> np.ndarray:
    """weights of alternating sign with sum |w| = total and unequal magnitudes: the conditioning a synthesis outside the tracked
    range of widths shows (tests/test_posthoc_ema_host.py prints it)"""
    mag = np.linspace(1.0, 2.0, K)
    w = mag * total / mag.sum() * np.where(np.arange(K) % 2 == 0, 1.0, -1.0)
    return w.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- reconstruction
def reconstruction_case():
    """the issue's case: a 512-dimensional random walk of 2048 steps, profiles 0.05 and 0.10 by the recursion, snapshots every 64
    updates, target 0.075 at t = 2048 tracked directly for comparison"""
    rng = np.random.default_rng(0)
    theta = np.cumsum(0.01 * rng.standard_normal((2048, 512)), 0) + rng.standard_normal(512)
    sig = (0.05, 0.10, 0.075)
    gam = [gamma_of(s) for s in sig]
    ema = [np.zeros(512) for _ in sig]
    snaps, in_t, in_s = [], [], []
    for t in range(1, 2049):
        for k, g in enumerate(gam):
            w = weight32(t, g)
            ema[k] = ema[k] + w * (theta[t - 1] - ema[k])
        if t % 64 == 0:
            for k in (0, 1):
                snaps.append(ema[k].copy())
                in_t.append(t)
                in_s.append(sig[k])
    return dict(theta=theta, direct=ema[2], tracked=(ema[0], ema[1]), snaps=np.stack(snaps), in_t=in_t, in_sigma=in_s)
