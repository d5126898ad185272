#!/usr/bin/env python3
"""Cost of the reference's optimizer chain (clip_grad + lr_schedule) on the DeiT-S training step.

    python tools/optim_ab.py [--blocks 9] [--steps 20] [--batch 128] [--legs off,on] [--tree DIR]

Kernels: the global-norm pass + prepare kernel (sae_adamw_prepare) over a flat buffer of the
DeiT-S size, and the one-thread tick they replace, each inside HIP graphs of 10 back-to-back calls
(HIP events around the replay, median over iterations, per-call time = replay time / 10).
Step: the captured training step of bench.py (same model, batch and feed); the legs' blocks of
``--steps`` replays alternate, median block per leg.  ``off``: TrainStep's defaults; ``on``:
clip_grad 1.0 and the reference's warm-up-cosine schedule.  ``--tree DIR`` imports the package from
another checkout (the parent commit's, with ``--legs off``: the leg with the feature absent).
One line per kernel / leg (profiles/optim_ab.txt).
"""
import argparse
import os
import statistics
import sys

REPS = 10


def graph_of(fn):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    return g


def kernels(dev, n, iters=30):
    import ctypes
    import math
    import torch
    from sae_vision_amd import _lib as L
    lib = L.load()
    g = torch.randn(n, device=dev)
    ws = torch.zeros(lib.sae_adamw_prepare_workspace_bytes(n) // 8, dtype=torch.float64, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    hyper = torch.zeros(4, device=dev)
    sched = L.LrSchedule(L.SAE_LR_WARMUP_COSINE, 0.0, 1e-3, 1e-5, 100, 1000)
    st = lambda: torch.cuda.current_stream(dev).cuda_stream
    calls = {
        "prepare (norm + clip + lr)": lambda: L.check(lib.sae_adamw_prepare(
            st(), n, g.data_ptr(), 1.0, ctypes.byref(sched), step.data_ptr(), ws.data_ptr(), hyper.data_ptr())),
        "prepare (lr only)": lambda: L.check(lib.sae_adamw_prepare(
            st(), 0, None, math.inf, ctypes.byref(sched), step.data_ptr(), None, hyper.data_ptr())),
        "tick (sae_adamw_step, 0 chunks)": lambda: L.check(lib.sae_adamw_step(
            st(), 0, None, step.data_ptr(), 1e-3, 0.9, 0.999, 1e-8, 1e-4)),
    }
    graphs = {k: graph_of(f) for k, f in calls.items()}
    times = {k: [] for k in calls}
    for _ in range(iters):
        for k, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / REPS)
    for k, t in times.items():
        us = statistics.median(t)
        extra = f" | {4 * n / us / 1e6:5.2f} TB/s of gradient read" if "norm" in k else ""
        print(f"{k:<32s} n={n:<10d} | {us:7.1f} us per call{extra}", flush=True)


def step(dev, legs, B, blocks, steps):
    import torch
    from sae_vision_amd import train, vit
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(B, 224, 224, 3, device=dev, generator=g).permute(1, 2, 3, 0).contiguous()
    labels = torch.randint(0, 1000, (B,), device=dev, generator=g)
    runs = []
    for leg in legs:
        torch.manual_seed(0)
        m = vit.create_model("deit_s_patch16", 1000, torch.bfloat16, device=dev)
        kw = {}
        if leg == "on":
            kw = dict(clip_grad=1.0, lr_schedule=train.reference_schedule(5e-4, B, 1281167 // B))
        s = train.TrainStep(m, global_batch=B, device=dev, graph=True, input_layout="HWCN", **kw)
        for _ in range(10):
            s(images, labels)
        runs.append((s, s.input_buffers() or (images, labels)))
    torch.cuda.synchronize()
    times = [[] for _ in runs]
    for _ in range(blocks):
        for i, (s, (im, lb)) in enumerate(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                s(im, lb)
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) / steps)
    for leg, t, (s, _) in zip(legs, times, runs):
        n = s._flat.numel()
        print(f"{'deit_s step, feature ' + leg:<32s} B={B} 224px graph, flat n={n} | median {statistics.median(t):7.3f} ms | "
              f"blocks min {min(t):.3f} max {max(t):.3f}", flush=True)
        s.close()
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    dev = torch.device("cuda:0")
    legs = args.legs.split(",")
    n = step(dev, legs, args.batch, args.blocks, args.steps)
    if not args.no_kernels and "on" in legs:
        kernels(dev, n)   # the step's flat gradient buffer: parameters + alignment padding


if __name__ == "__main__":
    main()
