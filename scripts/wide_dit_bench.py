"""Wide-row timings (inner_dim above 1024).
    python scripts/wide_dit_bench.py [--iters N] [--no-step] [--batch B]

1. Row kernels: every row kernel a bf16 transformer engine reaches, at M = 65536 token rows (256 samples of 256 tokens) and
   D in {1024, 1536, 2048, 4096}.  D = 1024 runs the one-wave-per-row kernels (the baseline, same run); the wider rows run the
   *_rows_k kernels of csrc/norm.hip.  Bytes are the token-row tensors each call must read and write once (computed from the shapes:
   per-sample vectors and row statistics are left out), GB/s against the 6.3 TB/s measured HBM ceiling of an MI355X, and the ratio
   to the same kernel at D = 1024.
2. Training step: a bf16 flow-matching step (forward, backward, fused AdamW) of a class-conditional MMDiT on 256 tokens (32 x 32
   latents, patch 2) at 1152 wide / 18 heads / depth 28 and 1536 / 24 / 24.  Model FLOP = 3 x the forward's matmuls: per token and
   block 2 * (4 D^2 + 3 D F) for qkv, projection, SwiGLU up (2F x D) and down (D x F), plus 4 N D for QK^T and PV; TFLOP/s against
   the 2.5 PF/s dense bf16 peak."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffulab_amd import ops  # noqa: E402

DEV, BF, F32 = "cuda", torch.bfloat16, torch.float32
HBM = 6.3e12
PEAK = 2.5e15
M, RPM = 65536, 256
WIDTHS = [1024, 1536, 2048, 4096]


def timeit(fn, iters):
    """us per call between device events, after warm-up calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def row_cases(D):
    """(name, bytes, fn) for every row kernel at [M, D]"""
    g = torch.Generator(device=DEV).manual_seed(D)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV).to(BF)  # noqa: E731
    B = M // RPM
    x, t, d, dres = r(M, D), r(M, D), r(M, D), r(M, D)
    mod = r(B, 3 * D) * 0.1
    sc, sh, gate = mod[:, :D], mod[:, D:2 * D], mod[:, 2 * D:]
    w, b = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    out, xo, dx, dt = (torch.empty(M, D, device=DEV, dtype=BF) for _ in range(4))
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    dmod = torch.zeros(B, 3 * D, device=DEV)
    dwb = torch.zeros(B, 2, D, device=DEV)
    tmod = r(M, 3 * D) * 0.1
    dtok = torch.empty(M, 3 * D, device=DEV, dtype=BF)
    dwb_tok = torch.zeros(8, 2, D, device=DEV)
    H = D // 64
    qkv = r(M, 3 * D)
    q, k, v, dq, dk, dv = (torch.empty(B, H, RPM, 64, device=DEV, dtype=BF) for _ in range(6))
    for z in (dq, dk, dv):
        z.copy_(torch.randn(z.shape, generator=g, device=DEV))
    rr = torch.empty(M, 2, device=DEV)
    sq, sk = torch.ones(D, device=DEV), torch.ones(D, device=DEV)
    ang = torch.rand(RPM, 32, generator=g, device=DEV)
    cs, sn = ang.cos().contiguous(), ang.sin().contiguous()
    dqkv = torch.empty(M, 3 * D, device=DEV, dtype=BF)
    dsc = torch.zeros(2, D, device=DEV)
    ops.ln_modulate_fwd(x, None, None, sc, sh, RPM, 1e-6, out, mean, rstd)  # statistics for the backward calls
    ops.qk_norm_rope_fwd(qkv, sq, sk, cs, sn, q, k, v, rr, B, RPM, H, 64, 64)
    MD = M * D * 2
    return [
        ("ln_modulate_fwd", 2 * MD, lambda: ops.ln_modulate_fwd(x, None, None, sc, sh, RPM, 1e-6, out, mean, rstd)),
        ("ln_modulate_fwd +gate +affine", 4 * MD,
         lambda: ops.ln_modulate_fwd(x, w, b, sc, sh, RPM, 1e-6, out, mean, rstd, t=t, gate=gate, x_out=xo)),
        ("ln_modulate_bwd +dres", 4 * MD,
         lambda: ops.ln_modulate_bwd(d, x, None, None, sc, RPM, mean, rstd, dres, dx, dmod[:, :D], dmod[:, D:2 * D], None)),
        ("ln_modulate_bwd +gate +affine", 6 * MD,
         lambda: ops.ln_modulate_bwd(d, x, w, b, sc, RPM, mean, rstd, dres, dx, dmod[:, :D], dmod[:, D:2 * D], dwb, gate_t=t, gate=gate,
                                     dt=dt, dgate=dmod[:, 2 * D:])),
        ("ln_modulate_bwd_tok +gate +affine", 11 * MD,
         lambda: ops.ln_modulate_bwd_tok(d, x, w, b, tmod[:, :D], mean, rstd, dres, dx, dtok[:, :D], dtok[:, D:2 * D], dwb_tok,
                                         gate_t=t, gate=tmod[:, 2 * D:], dt=dt, dgate=dtok[:, 2 * D:])),
        ("gate_bwd", 3 * MD, lambda: ops.gate_bwd(d, t, gate, RPM, dt, dmod[:, 2 * D:])),
        ("qk_norm_rope_fwd", 6 * MD, lambda: ops.qk_norm_rope_fwd(qkv, sq, sk, cs, sn, q, k, v, rr, B, RPM, H, 64, 64)),
        ("qk_norm_rope_bwd", 8 * MD,
         lambda: ops.qk_norm_rope_bwd(dq, dk, dv, qkv, sq, sk, cs, sn, rr, dqkv, dsc, B, RPM, H, 64, 64)),
    ]


def row_table(iters):
    res = {}
    for D in WIDTHS:
        for name, nbytes, fn in row_cases(D):
            res[(name, D)] = (timeit(fn, iters), nbytes)
        torch.cuda.empty_cache()
    names = [n for n, _, _ in row_cases(1024)]
    print(f"row kernels at M = {M} rows ({M // RPM} samples x {RPM} tokens); GB/s vs {HBM / 1e12:.1f} TB/s; x D=1024 = GB/s / the same "
          "kernel's GB/s at D = 1024")
    print(f"{'kernel':34s} {'D':>5s} {'us':>9s} {'MB':>8s} {'GB/s':>7s} {'of HBM':>7s} {'x D=1024':>8s}")
    for n in names:
        base = res[(n, 1024)][1] / res[(n, 1024)][0] * 1e-3
        for D in WIDTHS:
            us, nb = res[(n, D)]
            gbs = nb / us * 1e-3
            print(f"{n:34s} {D:5d} {us:9.1f} {nb / 1e6:8.1f} {gbs:7.0f} {gbs * 1e9 / HBM:7.2f} {gbs / base:8.2f}")


def train_step(D, heads, depth, batch, steps, warmup):
    from diffulab_amd import Diffuser, MMDiT
    from diffulab_amd.training import FusedAdamW

    torch.manual_seed(0)
    kw = dict(input_channels=4, output_channels=4, inner_dim=D, embedding_dim=D, num_heads=heads, mlp_ratio=4, patch_size=2,
              depth=depth, n_classes=1000, classifier_free=True)
    m = MMDiT(simple_dit=True, **kw).to(DEV)
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=50)
    opt = FusedAdamW(list(m.parameters()), lr=1e-4, weight_decay=0.01)
    x0 = torch.randn(batch, 4, 32, 32, device=DEV)
    y = torch.randint(0, 1000, (batch,), device=DEV)

    def step():
        opt.zero_grad()
        t = d.draw_timesteps(batch).to(DEV, non_blocking=True)
        losses = d.compute_loss({"x": x0, "y": y, "p": 0.1}, timesteps=t)
        sum(losses.values()).backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    N, F = 256, 4 * D
    flop = 3 * depth * batch * N * (2 * (4 * D * D + 3 * D * F) + 4 * N * D)
    nparam = sum(p.numel() for p in m.parameters())
    del m, opt, d
    torch.cuda.empty_cache()
    return ms, flop, nparam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    row_table(a.iters)
    if a.no_step:
        return
    print(f"\nbf16 flow-matching training step, class-conditional MMDiT, 256 tokens, batch {a.batch}")
    print(f"{'D / heads / depth':20s} {'params':>8s} {'ms/step':>8s} {'img/s':>7s} {'TFLOP/s':>8s} {'of peak':>7s}")
    for D, heads, depth in ((1152, 18, 28), (1536, 24, 24)):
        ms, flop, n = train_step(D, heads, depth, a.batch, a.steps, 3)
        tf = flop / ms * 1e-9
        print(f"{f'{D} / {heads} / {depth}':20s} {n / 1e6:7.0f}M {ms:8.1f} {a.batch / ms * 1e3:7.0f} {tf:8.0f} {tf * 1e12 / PEAK:7.2f}")


if __name__ == "__main__":
    main()
