#!/usr/bin/env python3
"""A/B of one CeiT ``LeFFBlock`` (Dense -> BatchNorm + GELU -> k x k convolution -> BatchNorm + GELU ->
Dense -> BatchNorm + GELU around the class token), training forward + backward in bf16, on its two
routes inside ONE process: ``hip`` (forward(): ops.bn_gelu, the sae_bn_gelu_* kernels of
csrc/bn_rows.h, and ops.conv_tokens) and ``framework`` (_framework_forward(): slice, the BatchNorm as
elementwise / reduction passes, F.gelu, F.conv2d, torch.cat, autograd's replay of all of them).  The two
Dense layers (ops.dense) are the same on both.

    python tools/leff_ab.py [--rounds 7] [--iters 10] [--batch 128] > profiles/leff_ab.txt

Shapes: 14 x 14 patch tokens + the class token at E = 192, 384, 768 (ceit_t, ceit_s, ceit_b) with the
CeiT defaults expand_ratio = 4 and leff_kernel_size = 3 (models/ceit.py).  The routes alternate round
by round after a warm-up of every shape; a round is one event-timed window of ``iters`` forward +
backward calls; the figure is the median over the rounds, with min / max.  Two more rows time
ops.bn_gelu alone on the block's two widths, [B, 196, 4 E] behind the class row of [B, 197, 4 E]
(BatchNorm_0) and [B, 196, E] into [B, 197, E] (BatchNorm_2), and set them against the bytes the operation
needs: x read twice and y written by the forward, x and dy read twice and dx written by the backward --
8 tensors of B 196 C elements of 2 bytes."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTHS = [192, 384, 768]
S, K, RATIO = 14, 3, 4


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    import torch
    import sae_vision_amd.layers as layers
    import sae_vision_amd.ops as ops
    if not torch.cuda.is_available():
        sys.exit("leff_ab: needs a GPU")
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    B, L = a.batch, S * S
    print(f"# LeFFBlock forward + backward, bf16, batch {B}, {S}x{S} tokens + class token, k = {K}, expand_ratio "
          f"{RATIO}: median ms of {a.rounds} rounds x {a.iters} calls (routes alternated), [min .. max]")
    worst = 0.0
    for E in WIDTHS:
        torch.manual_seed(0)
        blk = layers.LeFFBlock(expand_ratio=RATIO, kernel_size=K, dtype=dt, in_ch=E, device=dev)
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(B, 1 + L, E, device=dev, generator=g).to(dt).requires_grad_(True)
        dy = torch.randn(B, 1 + L, E, device=dev, generator=g).to(dt)
        params = list(blk.parameters())
        routed = blk._hip_ok(x, True)

        def run(f, leaf, cot):
            def once():
                f().backward(cot)
                leaf.grad = None
                for p in params:
                    p.grad = None
            return once

        # ops.bn_gelu alone, in the layouts of BatchNorm_0 (x_lead) and BatchNorm_2 (y_lead)
        bn0, bn2 = blk.BatchNorm_0, blk.BatchNorm_2
        h0 = torch.randn(B, 1 + L, RATIO * E, device=dev, generator=g).to(dt).requires_grad_(True)
        d0 = torch.randn(B, L, RATIO * E, device=dev, generator=g).to(dt)
        h2 = torch.randn(B, L, E, device=dev, generator=g).to(dt).requires_grad_(True)
        variants = {
            "hip": run(lambda: blk(x, True), x, dy),
            "framework": run(lambda: blk._framework_forward(x, True), x, dy),
            "bn_gelu 4E": run(lambda: ops.bn_gelu(h0, bn0.scale, bn0.bias, bn0.mean, bn0.var, bn0.momentum, bn0.eps, True,
                                                  dt, x_lead=1), h0, d0),
            "bn_gelu E": run(lambda: ops.bn_gelu(h2, bn2.scale, bn2.bias, bn2.mean, bn2.var, bn2.momentum, bn2.eps, True,
                                                 dt, y_lead=1, lead=x.detach()[:, :1]), h2, dy),
        }
        for f in variants.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        res = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, f in variants.items():
                res[k].append(window(f, a.iters))
        med = {k: statistics.median(v) for k, v in res.items()}
        print(f"E = {E}, hidden {RATIO * E} (module routes to {'hip' if routed else 'framework'})")
        for k in variants:
            print(f"  {k:10s} {med[k]:8.3f} ms [{min(res[k]):7.3f} .. {max(res[k]):7.3f}]")
        ratio = med["hip"] / med["framework"]
        worst = max(worst, ratio if routed else 0.0)
        print(f"  hip / framework {ratio:.3f}")
        for k, C in (("bn_gelu 4E", RATIO * E), ("bn_gelu E", E)):
            nbytes = 8 * 2 * B * L * C
            print(f"  {k}: {nbytes / 1e6:.1f} MB algorithmic -> {nbytes / med[k] / 1e9:.3f} TB/s achieved", flush=True)
    print(f"# worst hip / framework over the routed shapes: {worst:.3f} ({'not slower' if worst <= 1.0 else 'SLOWER'})")


if __name__ == "__main__":
    main()
