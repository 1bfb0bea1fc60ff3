"""Generate tests/golden/gd_targets.npz by IMPORTING THE REAL REFERENCE: what its ``GaussianDiffusion.add_noise`` and its ``DDPM``
sampler say the three parameterisations it knows are (``_get_mean_from_x_start``: the xprev target; ``_get_eps_from_xstart``; and
``DDPM(mean_type=mt).step`` fed the exact target of ``mt``), on the 1000-step linear chain and on a 50-step respaced one.

Runs only in the build container (the reference is not on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_gd_targets_golden.py

Like make_golden.py (whose import shims this script reuses by loading it), only OUTPUTS of the reference are stored.  The inputs are
named draws (``gdt.x0``, ``gdt.eps``) that tests/gd_param_common.py regenerates; the step's ``randn_like`` is pinned by a seed and only
the two outputs that do not depend on it are kept (``estimated_x0``, ``x_prev_mean``).
v-prediction has no counterpart in the reference: the tests check it by algebra.
"""

from __future__ import annotations

import importlib.util
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)  # installs the import shims and imports the reference

import torch  # noqa: E402

from oracle import synth  # noqa: E402

SHAPE = (5, 3, 8, 8)
CHAINS = {"full": (1000, (0, 0, 1, 500, 999)), "r50": (50, (0, 0, 1, 25, 49))}
SEED = 23


def main() -> None:
    o = {}
    x0 = synth.uniform("gdt.x0", SHAPE, lo=-1.0, hi=1.0)
    eps = synth.normal("gdt.eps", SHAPE)
    for chain, (steps, ts) in CHAINS.items():
        t = torch.tensor(ts, dtype=torch.int32)
        gd = mg.GaussianDiffusion(n_steps=1000)
        if steps != 1000:
            gd.set_steps(steps)
        betas = gd.betas
        assert betas.shape == (steps,)
        xt, _ = gd.add_noise(x0, t, eps)
        s = mg.DDPM()
        s.set_steps(betas)
        xprev = s._get_mean_from_x_start(xt, x0, t)
        o[f"{chain}_xt"] = xt
        o[f"{chain}_xprev_target"] = xprev
        o[f"{chain}_eps_from_xstart"] = s._get_eps_from_xstart(x0, xt, t)
        for mt, target in (("epsilon", eps), ("xstart", x0), ("xprev", xprev)):
            s = mg.DDPM(mean_type=mt)
            s.set_steps(betas)
            torch.manual_seed(SEED)
            r = s.step(target, t, xt)
            o[f"{chain}_{mt}_estimated_x0"] = r["estimated_x0"]
            o[f"{chain}_{mt}_x_prev_mean"] = r["x_prev_mean"]
    assert all(bool(torch.isfinite(v).all()) and v.dtype == torch.float32 for v in o.values())
    mg.save("gd_targets", **o)


if __name__ == "__main__":
    main()
