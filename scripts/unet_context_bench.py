"""Timings of the text-conditioned UNet (context embedder -> TransformerBlocks) on one MI355X: the bf16 training step and the inference
forward at configs/model/unet.yaml dims without labels, C_ctx = 768, L = 77 (ragged masks), and the cross-attention core alone --
dl_attn_cross_* against the f32 fallback (f32 copies + batched dl_f32_gemm + dl_f32_softmax_keymask_fwd) -- at the two head widths of
that configuration (dh 256 at 8 x 8, 512 at 4 x 4).  Prints one JSON line."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from diffulab_amd import Diffuser, ops  # noqa: E402
from diffulab_amd.networks.denoisers import UNetModel  # noqa: E402
from diffulab_amd.training.optim import FusedAdamW  # noqa: E402
from unet_context_common import ChannelFirstEmbedder, mask_of  # noqa: E402


def timed(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def core(B: int, Nq: int, L: int, H: int, dh: int, steps: int, warmup: int) -> dict:
    c = H * dh
    g = torch.Generator(device="cuda").manual_seed(0)
    q = torch.randn(B * Nq, c, device="cuda", generator=g).bfloat16()
    kv = torch.randn(B * L, 2 * c, device="cuda", generator=g).bfloat16()
    dout = torch.randn(B * Nq, c, device="cuda", generator=g).bfloat16()
    keep = mask_of([L - (i % 40) for i in range(B)], L).cuda()
    bias = torch.zeros(B, L, device="cuda").masked_fill_(~keep, float("-inf"))
    out, probs, ds = torch.empty_like(q), torch.empty(B, H, Nq, L, device="cuda"), torch.empty(B, H, Nq, L, device="cuda")
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    qf, kvf, of = torch.empty(B * Nq, c, device="cuda"), torch.empty(B * L, 2 * c, device="cuda"), torch.empty(B * Nq, c, device="cuda")
    dqf, dkvf = torch.empty_like(qf), torch.empty_like(kvf)

    def hip():
        ops.attn_cross_fwd(q, kv[:, :c], kv[:, c:], bias, out, probs, B, Nq, L, H, dh)
        ops.attn_cross_bwd(q, kv[:, :c], kv[:, c:], bias, dout, probs, ds, dq, dkv[:, :c], dkv[:, c:], B, Nq, L, H, dh)

    def fallback():
        ops.cast_bf16_to_f32(q, qf)
        ops.cast_bf16_to_f32(kv, kvf)
        ops.f32_xattn_fwd(qf, kvf[:, :c], kvf[:, c:], bias, of, probs, B, Nq, L, H, dh)
        ops.cast_f32_to_bf16(of, out)
        ops.cast_bf16_to_f32(dout, of)
        ops.f32_xattn_bwd(qf, kvf[:, :c], kvf[:, c:], of, probs, ds, dqf, dkvf[:, :c], dkvf[:, c:], B, Nq, L, H, dh)
        ops.cast_f32_to_bf16(dqf, dq)
        ops.cast_f32_to_bf16(dkvf, dkv)

    return {"hip_ms": timed(hip, steps, warmup), "fallback_ms": timed(fallback, steps, warmup)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    B, L, cc = a.batch, 77, 768
    m = UNetModel(image_size=[32, 32], in_channels=1, model_channels=128, out_channels=1, num_res_blocks=2, attention_resolutions=[4, 8, 16],
                  num_heads=2, resblock_updown=True, use_scale_shift_norm=True, context_embedder=ChannelFirstEmbedder(cc)).cuda()
    gd = Diffuser(m, sampling_method="ddpm", model_type="gaussian_diffusion", n_steps=1000)
    opt = FusedAdamW(m.parameters(), lr=1e-4)
    g = torch.Generator(device="cuda").manual_seed(1)
    ctx = {"embeddings": torch.randn(B, cc, L, device="cuda", generator=g),
           "attn_mask": mask_of([L - (i % 60) for i in range(B)], L).cuda()}
    x0, noise = torch.randn(B, 1, 32, 32, device="cuda", generator=g), torch.randn(B, 1, 32, 32, device="cuda", generator=g)
    t = torch.randint(0, 1000, (B,), device="cuda", generator=g, dtype=torch.int32)

    def step():
        opt.zero_grad()
        gd.compute_loss({"x": x0, "context": ctx, "p": 0.0}, timesteps=t, noise=noise)["loss"].backward()
        opt.step()

    def infer():
        with torch.inference_mode():
            m(x=x0, timesteps=t, context=ctx)

    res = {"batch": B, "L": L, "C_ctx": cc, "train_step_ms": timed(step, a.steps, a.warmup), "inference_forward_ms": timed(infer, a.steps, a.warmup),
           "xattn_core_dh256": core(B, 64, L, 2, 256, a.steps, a.warmup), "xattn_core_dh512": core(B, 16, L, 2, 512, a.steps, a.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
