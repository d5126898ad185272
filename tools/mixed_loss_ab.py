#!/usr/bin/env python3
"""A/B of the DeiT-S/16 graph training step with and without mixup / cutmix targets and in-step
metrics, inside ONE process (cdna_hip_programming.md §5.4 rule 24): the two variants interleaved
over several rounds, median ms/step each and the round-to-round spread of each.

    python tools/mixed_loss_ab.py [--rounds 6] [--steps 20] [--batch 128]
Variants of the one loss family (csrc/loss.h, sae_mixed_ce_fwd / _bwd): ``plain`` (TrainStep(graph=True):
no partner labels, no ranks -- the special case sae_smoothed_ce_* names; ce_fwd_kernel<T, false>) and
``mixed`` (TrainStep(graph=True, mix=True, metrics=True): partner labels, ratios and the top-1 / top-5
ranks; ce_fwd_kernel<T, true>).  Each variant trains its own copy of the model from the same start.
Output: profiles/mixed_loss_ab.txt.
"""
import argparse
import copy
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--model", default="deit_s_patch16")
    a = ap.parse_args()
    if a.rounds < 4:
        ap.error("--rounds must be at least 4 (the spread is read from them)")
    import torch
    from sae_vision_amd import train, vit
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m_plain = vit.create_model(a.model, 1000, torch.bfloat16, device=dev)
    m_mixed = copy.deepcopy(m_plain)
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(a.batch, 224, 224, 3, device=dev, generator=g)
    labels = torch.randint(0, 1000, (a.batch,), device=dev, generator=g)
    mix_labels = torch.randint(0, 1000, (a.batch,), device=dev, generator=g)
    ratio = torch.rand(a.batch, device=dev, generator=g)
    s_plain = train.TrainStep(m_plain, global_batch=a.batch, device=dev, graph=True)
    s_mixed = train.TrainStep(m_mixed, global_batch=a.batch, device=dev, graph=True, mix=True, metrics=True)
    variants = {"plain": lambda: s_plain(images, labels),
                "mixed": lambda: s_mixed(images, labels, mix_labels, ratio)}
    for run in variants.values():   # capture and warm both
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    res = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, run in variants.items():
            run()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                run()
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / a.steps * 1e3)
    print(f"# {a.model} batch {a.batch}, graph step, {a.rounds} rounds x {a.steps} steps, variants interleaved")
    for k in variants:
        med = statistics.median(res[k])
        print(f"{k:6s} ms/step median {med:7.3f} min {min(res[k]):7.3f} max {max(res[k]):7.3f} "
              f"spread {max(res[k]) - min(res[k]):6.3f} img/s {a.batch / med * 1e3:8.1f} | rounds "
              + " ".join(f"{t:.3f}" for t in res[k]), flush=True)
    d = statistics.median(res["mixed"]) - statistics.median(res["plain"])
    spread = max(res["plain"]) - min(res["plain"])
    print(f"mixed - plain {d:+.3f} ms/step; plain's round-to-round spread {spread:.3f} ms: "
          f"{'within' if abs(d) <= spread else 'OUTSIDE'} the spread")
    print(f"last mixed step: loss {float(s_mixed(images, labels, mix_labels, ratio)):.4f} "
          f"top1 {float(s_mixed.top1):.4f} top5 {float(s_mixed.top5):.4f}")
    s_plain.close()
    s_mixed.close()


if __name__ == "__main__":
    main()
