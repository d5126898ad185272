#!/usr/bin/env python3
"""A/B of one CvT ``ConvProjectionBlock`` (depthwise 3x3 + BatchNorm + 1x1), training forward +
backward in bf16, on its two routes inside ONE process: ``hip`` (forward(): ops.dwconv_bn, the
sae_dwconv_bn_* kernels of csrc/dwconv.h) and ``framework`` (_framework_forward(): nine strided
multiply-adds, the BatchNorm as elementwise / reduction passes, autograd's replay of both).  The 1x1
convolution (ops.dense) is the same on both.

    python tools/conv_proj_ab.py [--rounds 7] [--iters 20] [--batch 128] > profiles/conv_proj_ab.txt

Shapes: the CvT-13 stages at 224^2 (56x56x64, 28x28x192, 15x15x368 -- the class-token stage after
zero_pad_and_reshape), each at stride 1 (q) and 2 (k, v).  The routes alternate round by round after
a warm-up of every shape; a round is one event-timed window of ``iters`` forward + backward calls;
the figure is the median over the rounds, with min / max.  A third row times ops.dwconv_bn alone
(no 1x1) and sets it against the bytes the operation needs: x read twice (forward, dw) and dx
written, t written and read, y written, dy read -- (3 |x| + 4 |y|) elements of 2 bytes."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(56, 56, 64), (28, 28, 192), (15, 15, 368)]


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    a = ap.parse_args()
    import torch
    import sae_vision_amd.ops as ops
    from sae_vision_amd.layers import cvt
    if not torch.cuda.is_available():
        sys.exit("conv_proj_ab: needs a GPU")
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    print(f"# ConvProjectionBlock forward + backward, bf16, batch {a.batch}: median ms of {a.rounds} rounds x "
          f"{a.iters} calls (routes alternated), [min .. max]")
    worst = 0.0
    for H, W, C in SHAPES:
        for s in (1, 2):
            torch.manual_seed(0)
            blk = cvt.ConvProjectionBlock(C, C, 3, s, False, 0.9, 1e-5, dt, dev)
            g = torch.Generator(device=dev).manual_seed(1)
            x = torch.randn(a.batch, H, W, C, device=dev, generator=g).to(dt).requires_grad_(True)
            Ho, Wo = -(-H // s), -(-W // s)
            dy = torch.randn(a.batch, Ho, Wo, C, device=dev, generator=g).to(dt)
            params = list(blk.parameters())
            bn = blk.BatchNorm_0
            routed = ops.dwconv_bn_ok(x, 3, s, dt)

            def run(f):
                def once():
                    f().backward(dy)
                    x.grad = None
                    for p in params:
                        p.grad = None
                return once

            variants = {
                "hip": run(lambda: blk(x, True)),
                "framework": run(lambda: blk._framework_forward(x, True)),
                "hip op": run(lambda: ops.dwconv_bn(x, blk.Conv_0.kernel, bn.scale, bn.bias, bn.mean, bn.var, s,
                                                    bn.momentum, bn.eps, True, dt)),
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
            nbytes = 2 * a.batch * C * (3 * H * W + 4 * Ho * Wo)
            print(f"{H}x{W}x{C} stride {s} (module routes to {'hip' if routed else 'framework'})")
            for k in variants:
                print(f"  {k:10s} {med[k]:8.3f} ms [{min(res[k]):7.3f} .. {max(res[k]):7.3f}]")
            ratio = med["hip"] / med["framework"]
            worst = max(worst, ratio if routed else 0.0)
            print(f"  hip / framework {ratio:.3f}; conv + BN alone {nbytes / 1e6:.1f} MB algorithmic -> "
                  f"{nbytes / med['hip op'] / 1e9:.3f} TB/s achieved", flush=True)
    print(f"# worst hip / framework over the routed shapes: {worst:.3f} ({'not slower' if worst <= 1.0 else 'SLOWER'})")


if __name__ == "__main__":
    main()
