"""Long-sequence attention timings: forward and backward of dl_attn_fwd_ex / dl_attn_bwd_ex at (B, H, N), the tiled kernels at
(16, 10, 2048) as the yardstick, one masked joint text-image shape, and the same shapes through torch's
scaled_dot_product_attention where it has a flash backend on this device.
    python scripts/attn_long_bench.py [--iters N] [--no-sdpa] [--ddt-batch B] [--no-ddt]
TF/s counts 4*B*H*Nq*Nk*64 FLOP forward and 10*B*H*Nq*Nk*64 backward.  Last, one bf16 joint DDT training step (forward, backward,
AdamW) at the txt-to-img dims of configs/model/ddt_txt.yaml (640 wide, 10 heads, 128 input channels, patch 1, 8 encoder + 4 decoder
blocks) on 64x64 image tokens with a 300-token context of width 1024 (ragged key mask): 4396 attention tokens, padded to 4608."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from diffulab_amd import ops  # noqa: E402

DEV, BF, DH = "cuda", torch.bfloat16, 64
SCALE = DH**-0.5
# (label, B, H, Nq, Nk, masked joint: (context tokens, image tokens) or None)
SHAPES = [("2048 (tiled, yardstick)", 16, 10, 2048, 2048, None), ("2304", 16, 10, 2304, 2304, None), ("4096", 16, 10, 4096, 4096, None),
          ("8192", 4, 10, 8192, 8192, None), ("32768", 1, 10, 32768, 32768, None), ("joint 300+64x64", 4, 10, 4608, 4608, (300, 4096))]


def timeit(fn, iters):
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


def sdpa_backend():
    """(context manager factory, name) of a flash SDPA backend that runs here, or (None, reason)"""
    try:
        from torch.nn.attention import SDPBackend, sdpa_kernel

        q = torch.randn(1, 1, 256, DH, device=DEV, dtype=BF)
        with sdpa_kernel(SDPBackend.FLASH_ATTENTION):
            torch.nn.functional.scaled_dot_product_attention(q, q, q)
        torch.cuda.synchronize()
        return (lambda: sdpa_kernel(SDPBackend.FLASH_ATTENTION)), "flash"
    except Exception as e:  # noqa: BLE001
        return None, f"no flash backend ({type(e).__name__}: {str(e).splitlines()[0][:80]})"


def ddt_joint_step(batch, steps=10, warmup=3):
    """ms per bf16 joint DDT training step at the txt-to-img dims, 64x64 image tokens + 300 context tokens"""
    from diffulab_amd import DDT, Diffuser
    from diffulab_amd.networks.embedders import PrecomputedEmbedder
    from diffulab_amd.training import FusedAdamW

    kw = dict(input_channels=128, output_channels=128, inner_dim=640, num_heads=10, mlp_ratio=4, patch_size=1, encoder_depth=8,
              decoder_depth=4, classifier_free=True, rope_base=1000, rope_axes_dim=[20, 22, 22], n_classes=None)
    Lc, Cd = 300, 1024
    torch.manual_seed(0)
    m = DDT(simple_ddt=False, context_embedder=PrecomputedEmbedder(torch.randn(1, Lc, Cd), 7), **kw).to(DEV)
    d = Diffuser(m, sampling_method="euler", model_type="rectified_flow", n_steps=50, extra_args={"logits_normal": True})
    opt = FusedAdamW(list(m.parameters()), lr=1e-4, weight_decay=0.01)
    x0 = torch.randn(batch, 128, 64, 64, device=DEV)
    keep = torch.arange(Lc, device=DEV)[None, :] < torch.randint(8, Lc + 1, (batch, 1), device=DEV)
    ctx = {"embeddings": torch.randn(batch, Lc, Cd, device=DEV, dtype=BF), "attn_mask": keep}

    def step():
        opt.zero_grad()
        t = d.draw_timesteps(batch).to(DEV, non_blocking=True)
        losses = d.compute_loss({"x": x0, "initial_context": ctx, "p": 0.1}, timesteps=t)
        sum(losses.values()).backward()
        opt.step()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--no-sdpa", action="store_true")
    ap.add_argument("--ddt-batch", type=int, default=4)
    ap.add_argument("--no-ddt", action="store_true")
    a = ap.parse_args()
    ctx, sdpa_name = (None, "skipped") if a.no_sdpa else sdpa_backend()
    print(f"SDPA: {sdpa_name}")
    print(f"{'shape':26s} {'B':>3s} {'H':>3s} {'Nq':>6s} {'Nk':>6s} | {'fwd us':>9s} {'TF/s':>6s} | {'bwd us':>9s} {'TF/s':>6s}"
          + ("" if ctx is None else f" | {'sdpa fwd us':>11s} {'TF/s':>6s} | {'sdpa bwd us':>11s} {'TF/s':>6s}"))
    for label, B, H, Nq, Nk, joint in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(0)
        q, k, v = (torch.randn(B, H, n, DH, device=DEV, generator=g).to(BF) for n in (Nq, Nk, Nk))
        do = torch.randn(B, Nq, H * DH, device=DEV, generator=g).to(BF)
        out = torch.empty(B, Nq, H * DH, device=DEV, dtype=BF)
        lse = torch.empty(B, H, Nq, device=DEV)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        bias = None
        if joint is not None:  # ragged captions up to Lc, then the image tokens, then the pad to a multiple of 256
            Lc, Ni = joint
            keep = torch.zeros(B, Nk, dtype=torch.bool, device=DEV)
            for i in range(B):
                keep[i, : Lc - 37 * i] = True
                keep[i, Lc: Lc + Ni] = True
            bias = torch.zeros(B, Nk, device=DEV).masked_fill(~keep, float("-inf"))
        ffl, bfl = 4 * B * H * Nq * Nk * DH, 10 * B * H * Nq * Nk * DH
        uf = timeit(lambda: ops.attn_fwd_ex(q, k, v, out, lse, B, H, Nq, Nk, DH, SCALE, bias), a.iters)
        ub = timeit(lambda: ops.attn_bwd_ex(q, k, v, out, do, lse, dq, dk, dv, B, H, Nq, Nk, DH, SCALE, bias), a.iters)
        line = f"{label:26s} {B:3d} {H:3d} {Nq:6d} {Nk:6d} | {uf:9.1f} {ffl / uf / 1e6:6.1f} | {ub:9.1f} {bfl / ub / 1e6:6.1f}"
        if ctx is not None:
            qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
            mask = None if bias is None else bias.to(BF)[:, None, None, :]
            dos = do.view(B, Nq, H, DH).transpose(1, 2)
            try:
                with ctx():
                    o = torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, attn_mask=mask)
                    sf = timeit(lambda: torch.nn.functional.scaled_dot_product_attention(qs, ks, vs, attn_mask=mask), a.iters)
                    sb = timeit(lambda: torch.autograd.grad(o, (qs, ks, vs), dos, retain_graph=True), a.iters)
                line += f" | {sf:11.1f} {ffl / sf / 1e6:6.1f} | {sb:11.1f} {bfl / sb / 1e6:6.1f}"
            except Exception as e:  # noqa: BLE001  (e.g. flash takes no additive mask)
                line += f" | sdpa: {type(e).__name__}: {str(e).splitlines()[0][:60]}"
        print(line, flush=True)
        del q, k, v, do, out, lse, dq, dk, dv
        torch.cuda.empty_cache()
    if not a.no_ddt:
        ms = ddt_joint_step(a.ddt_batch)
        print(f"joint DDT train step (640/10h, 8+4 blocks, 128x64x64 latents + 300 context tokens), batch {a.ddt_batch}: {ms:.2f} ms "
              f"({a.ddt_batch / ms * 1e3:.1f} images/s)")


if __name__ == "__main__":
    main()
