#!/usr/bin/env python3
"""A/B of the CvT stem (``ConvTokenEmbedBlock``: k x k convolution, stride < k, SAME, + LayerNorm),
training forward + backward in bf16, on its two routes inside ONE process: ``hip`` (forward():
ops.conv_tokens -- sae_conv_window_gather, sae_gemm_nt, sae_gemm_dw, and for an input that takes a
gradient the dP product and sae_conv_window_scatter -- then ops.layer_norm) and ``framework``
(_framework_forward(): F.conv2d in fp32 on explicitly SAME-padded operands rounded to bf16, F.layer_norm,
autograd's replay).

    python tools/cvt_stem_ab.py [--rounds 7] [--iters 10] [--batch 128] > profiles/cvt_stem_ab.txt

Shapes: the three cvt-13 stems at 224^2 (224x224x3 -> 64 at 7/4, 56x56x64 -> 192 at 3/2,
28x28x192 -> 384 at 3/2).  The first stem's input is the image batch and takes no gradient; the other
two do.  The routes alternate round by round after a warm-up of every variant; a round is one
event-timed window of ``iters`` forward + backward calls; the figure is the median over the rounds,
with min / max.  A third row times the window-matrix kernels alone against the bytes they move (the
gather reads x and writes P; the scatter reads dP and writes dX).  Last: one cvt-13 training step
(TrainStep, HIP graph) in img/s, stems on either route, alternated the same way."""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (H, W, Cin, E, k, s, the input takes a gradient)
SHAPES = [(224, 224, 3, 64, 7, 4, False), (56, 56, 64, 192, 3, 2, True), (28, 28, 192, 384, 3, 2, True)]


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def alternate(variants, rounds, iters, warm=3):
    import torch
    for f in variants.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, f in variants.items():
            res[k].append(window(f, iters))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10, help="training steps per window (0: skip the step)")
    a = ap.parse_args()
    import torch
    import sae_vision_amd.ops as ops
    from sae_vision_amd import cvt, train
    if not torch.cuda.is_available():
        sys.exit("cvt_stem_ab: needs a GPU")
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    print(f"# ConvTokenEmbedBlock forward + backward, bf16, batch {a.batch}: median ms of {a.rounds} rounds x "
          f"{a.iters} calls (routes alternated), [min .. max]")
    worst = 0.0
    for H, W, C, E, k, s, xg in SHAPES:
        torch.manual_seed(0)
        blk = cvt.ConvTokenEmbedBlock(E, k, s, dt, in_ch=C, device=dev)
        g = torch.Generator(device=dev).manual_seed(1)
        # fp32 as in the model: the image batch, then the fp32 residual stream of the stage before
        x = torch.randn(a.batch, H, W, C, device=dev, generator=g).requires_grad_(xg)
        Ho, Wo = -(-H // s), -(-W // s)
        M, Kp = a.batch * Ho * Wo, ops.conv_window_cols(C, k)
        dy = torch.randn(a.batch, Ho * Wo, E, device=dev, generator=g).to(dt)
        dP = torch.randn(M, Kp, device=dev, generator=g).to(dt)
        params = list(blk.parameters())
        routed = ops.conv_tokens_ok(x, blk.Conv_0.kernel, k, s, dt)

        def run(f):
            def once():
                f().backward(dy)
                x.grad = None
                for p in params:
                    p.grad = None
            return once

        def kernels():
            ops.conv_window_matrix(x.detach(), k, s, dt)
            if xg:
                ops.conv_window_scatter(dP, x.shape, k, s)

        variants = {"hip": run(lambda: blk(x)), "framework": run(lambda: blk._framework_forward(x)), "gather/scatter": kernels}
        res = alternate(variants, a.rounds, a.iters)
        med = {n: statistics.median(v) for n, v in res.items()}
        xb = x.numel() * x.element_size()
        nbytes = xb + 2 * M * Kp + (2 * M * Kp + 2 * x.numel() if xg else 0)
        print(f"{H}x{W}x{C} -> {E}, {k}x{k} stride {s}: P {M} x {Kp} bf16 = {2 * M * Kp / 1e6:.1f} MB"
              f" (module routes to {'hip' if routed else 'framework'}; input gradient: {'yes' if xg else 'no'})")
        for n in variants:
            print(f"  {n:14s} {med[n]:8.3f} ms [{min(res[n]):7.3f} .. {max(res[n]):7.3f}]")
        ratio = med["hip"] / med["framework"]
        worst = max(worst, ratio if routed else 0.0)
        print(f"  hip / framework {ratio:.3f}; window kernels alone {nbytes / 1e6:.1f} MB -> "
              f"{nbytes / med['gather/scatter'] / 1e9:.3f} TB/s achieved", flush=True)
    print(f"# worst hip / framework over the routed shapes: {worst:.3f} ({'not slower' if worst <= 1.0 else 'SLOWER'})")
    if a.steps <= 0:
        return
    # one cvt-13 training step (forward, loss, backward, AdamW in one HIP graph), stems on either route
    torch.manual_seed(0)
    m_hip = cvt.create_cvt("cvt-13", 1000, dt, device=dev)
    m_fwk = copy.deepcopy(m_hip)
    for mod in m_fwk.modules():
        if isinstance(mod, cvt.ConvTokenEmbedBlock):
            mod.forward = mod._framework_forward
    g = torch.Generator(device=dev).manual_seed(2)
    images = torch.randn(a.batch, 224, 224, 3, device=dev, generator=g)
    labels = torch.randint(0, 1000, (a.batch,), device=dev, generator=g)
    steps = {n: train.TrainStep(m, global_batch=a.batch, device=dev, graph=True) for n, m in (("hip", m_hip), ("framework", m_fwk))}
    res = alternate({n: (lambda s=s: s(images, labels)) for n, s in steps.items()}, a.rounds, a.steps, warm=2)
    print(f"# cvt-13 training step, bf16, batch {a.batch}, 224 px, HIP graph: median of {a.rounds} rounds x {a.steps} steps")
    for n, v in res.items():
        ms = statistics.median(v)
        print(f"  stems {n:10s} {ms:8.3f} ms/step [{min(v):7.3f} .. {max(v):7.3f}]  {a.batch / ms * 1e3:9.1f} img/s"
              f"  (graph: {steps[n]._g is not None})")
    for s in steps.values():
        s.close()


if __name__ == "__main__":
    main()
