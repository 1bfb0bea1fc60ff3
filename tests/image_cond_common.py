"""Plain-torch restatement of image-to-image (SDEdit, Meng et al. 2022) and inpainting (RePaint, Lugmayr et al. 2022) sampling, as
`Flow.denoise` / `GaussianDiffusion.denoise` run it (imported by the test modules; not a conftest).  The reference has neither, so
this file states the semantics; the sampler step itself is the oracle's (oracle/diffusion.py) or tests/learned_variance_common.py's.

Every function takes a `dtype`: torch.float32 evaluates as the product does, torch.float64 evaluates the same formulas on the same
f32 inputs without rounding.  The loops take the run's noises as a list, in the order the product draws them:
    eps0 (the initial noise), then per repeat of a step: the sampler's own draw (Euler-Maruyama, DDPM, DDIM), the known region's draw
    (Gaussian diffusion, with a mask, t > 0), the re-noise draw (when another repeat of the step follows).
"""

from __future__ import annotations

import math

import torch
from torch import Tensor, nn

from oracle import diffusion as od

# (steps, strength) -> k = clamp(floor(strength * steps + 0.5), 1, steps)
STEP_TABLE = [((10, 0.3), 3), ((10, 0.7), 7), ((100, 0.29), 29), ((4, 0.5), 2), ((6, 0.01), 1), ((4, 0.125), 1), ((6, 1.0), 6),
              ((6, 0.5), 3), ((1, 1e-9), 1), ((1000, 1e-6), 1), ((50, 0.999), 50)]


def strength_steps(steps: int, strength: float) -> int:
    return max(1, min(steps, int(math.floor(strength * steps + 0.5))))


def n_model_calls(steps: int, strength: float, resample: int, cfg: bool) -> int:
    return (resample * (strength_steps(steps, strength) - 1) + 1) * (2 if cfg else 1)


def blend_ref(x: Tensor | None, ref: Tensor, noise: Tensor | None, mask: Tensor | None, a: float, b: float, dtype=torch.float64) -> Tensor:
    """known = a ref + b noise (noise is not read when b == 0); with a mask [B, 1 or C, *spatial]: x where m >= 1, known where m <= 0
    (both selects), m x + (1 - m) known between; without one: known"""
    known = a * ref.to(dtype)
    if b != 0:
        known = known + b * noise.to(dtype)
    if mask is None:
        return known
    m = mask.to(dtype).expand_as(known)
    x = x.to(dtype)
    return torch.where(m >= 1, x, torch.where(m <= 0, known, m * x + (1 - m) * known))


def flow_renoise_coefs(t_curr: float, t_prev: float) -> tuple[float, float]:
    """x_t = a x_prev + s randn takes the marginal (1 - t_prev) x0 + t_prev eps to (1 - t_curr) x0 + t_curr eps"""
    a = (1.0 - t_curr) / (1.0 - t_prev)
    return a, max(t_curr * t_curr - a * a * t_prev * t_prev, 0.0) ** 0.5


def gaussian_renoise_coefs(betas: Tensor, t: int) -> tuple[float, float]:
    """one forward step of the chain, q(x_t | x_{t-1})"""
    beta = float(betas[t])
    return (1.0 - beta) ** 0.5, beta**0.5


# ------------------------------------------------------------------------------------------------------------------ stub denoisers
class _Stub(nn.Module):
    """a denoiser with the interface the loops use: one dummy parameter (device / dtype probe), returns {"x": ...}, ignores `p`"""

    def __init__(self) -> None:
        super().__init__()
        self.dummy = nn.Parameter(torch.zeros(1))
        self.calls = 0

    def f(self, x: Tensor, t: Tensor) -> Tensor:
        raise NotImplementedError

    def forward(self, x: Tensor, timesteps: Tensor, p=None, **kw) -> dict[str, Tensor]:
        self.calls += 1
        t = timesteps.to(device=x.device, dtype=x.dtype).view(-1, *([1] * (x.dim() - 1)))
        return {"x": self.f(x, t)}


class PointMass(_Stub):
    """the flow model of a point mass at c: v = (x - c) / t, whose Euler samples end at c"""

    def __init__(self, c: float = 0.25) -> None:
        super().__init__()
        self.c = c

    def f(self, x, t):
        return (x - self.c) / t


class Mixer(_Stub):
    """a fixed model that couples neighbouring pixels, for both families: 0.5 x + 0.1 roll(x, 1, -1) - t, in x's dtype"""

    def f(self, x, t):
        return 0.5 * x + 0.1 * torch.roll(x, 1, -1) - t


def _predict(model: _Stub, x: Tensor, t_value, dtype, guidance: float) -> Tensor:
    t = torch.full((x.shape[0],), t_value, dtype=dtype)
    pred = model(x=x, timesteps=t, p=0)["x"]
    if guidance > 0:
        pred = od.cfg_combine(pred, model(x=x, timesteps=t, p=1)["x"], guidance)
    return pred


# ------------------------------------------------------------------------------------------------------------------ the two loops
def flow_loop(model: _Stub, timesteps: list[float], init: Tensor, noises: list[Tensor], mask: Tensor | None = None, strength: float = 1.0,
              resample: int = 1, sampler: str = "euler", eta: float = 0.7, guidance: float = 0.0, dtype=torch.float64) -> dict:
    """-> {"x": final sample, "xt": [starting x, x_prev after the blend of every step's last repeat]}"""
    draw = iter(noises)
    init = init.to(dtype)
    eps0 = next(draw).to(dtype)
    steps = len(timesteps) - 1
    k = strength_steps(steps, strength)
    i0 = steps - k
    t0 = timesteps[i0]
    x = (1 - t0) * init + t0 * eps0
    xt = [x]
    pairs = list(zip(timesteps[i0:-1], timesteps[i0 + 1:]))
    for j, (t_curr, t_prev) in enumerate(pairs):
        repeats = resample if j + 1 < k else 1
        for r in range(repeats):
            v = _predict(model, x, t_curr, dtype, guidance)
            if sampler == "euler":
                xp = od.euler_step(x, v, t_curr, t_prev)["x_prev"]
            else:
                xp = od.euler_maruyama_step(x, v, t_curr, t_prev, timesteps[1], eta, noise=next(draw).to(dtype))["x_prev"]
            if mask is not None:
                xp = blend_ref(xp, init, eps0, mask, 1.0 - t_prev, t_prev, dtype)
            x = xp
            if r + 1 < repeats:
                a, s = flow_renoise_coefs(t_curr, t_prev)
                x = a * xp + s * next(draw).to(dtype)
        xt.append(xp)
    return {"x": x, "xt": xt}


def gaussian_loop(model: _Stub, T: od.GaussianTables, init: Tensor, noises: list[Tensor], mask: Tensor | None = None, strength: float = 1.0,
                  resample: int = 1, sampler: str = "ddpm", eta: float = 0.0, guidance: float = 0.0, dtype=torch.float64) -> dict:
    """the chain of `T` (its own, possibly respaced, indices; the stub sees them unmapped).  Coefficients of the known region and of
    the re-noise: the fp64 tables cast to f32, as the product hands them to its kernel."""
    draw = iter(noises)
    init = init.to(dtype)
    eps0 = next(draw).to(dtype)
    B = init.shape[0]
    k = strength_steps(T.steps, strength)
    f32 = lambda v: float(torch.as_tensor(float(v), dtype=torch.float64).float())  # noqa: E731
    x = od.ddpm_add_noise(T, init, torch.full((B,), k - 1, dtype=torch.int32), eps0)
    xt = [x]
    for t in range(k - 1, -1, -1):
        repeats = resample if t > 0 else 1
        tt = torch.full((B,), t, dtype=torch.int32)
        for r in range(repeats):
            pred = _predict(model, x, t, dtype, guidance)
            nz = next(draw).to(dtype)
            if sampler == "ddpm":
                xp = od.ddpm_step(T, pred, tt, x, nz)["x_prev"]
            else:
                xp = od.ddim_step(T, pred, tt, x, nz, eta)["x_prev"]
            if mask is not None:
                if t > 0:
                    a, b = f32(T.sqrt_alphas_bar[t - 1]), f32((1.0 - T.alphas_bar[t - 1]).sqrt())
                    xp = blend_ref(xp, init, next(draw), mask, a, b, dtype)
                else:
                    xp = blend_ref(xp, init, None, mask, 1.0, 0.0, dtype)
            x = xp
            if r + 1 < repeats:
                a, s = (f32(c) for c in gaussian_renoise_coefs(T.betas, t))
                x = a * xp + s * next(draw).to(dtype)
        xt.append(xp)
    return {"x": x, "xt": xt}
