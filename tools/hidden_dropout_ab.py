#!/usr/bin/env python3
"""Cost of the hidden-state dropout (dropout_rate > 0): every kernel that has a dropout form, at the
DeiT-S training shape, dropout form against plain form, and the whole DeiT-S training step at
dropout_rate 0.1 against 0.

    python tools/hidden_dropout_ab.py [--iters 30] [--rate 0.1] [--batch 128] [--no-step]

Kernels: each call inside HIP graphs of 10 back-to-back launches (HIP events around the replay,
median over iterations, per-launch time = replay time / 10), the two forms' replays alternating.
Step: the captured training step of bench.py (same model, batch and feed), blocks of 20 replays of
the two models alternating, median block.  One line per kernel / step (profiles/hidden_dropout_ab.txt).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def ab(name, shape, plain, drop, iters, rate):
    """One line: per-launch time of both forms (their graph replays alternating) and the ratio."""
    import torch
    graphs = [graph_of(plain), graph_of(drop)]
    times = [[], []]
    for _ in range(iters):
        for i, g in enumerate(graphs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) * 1e3 / REPS)
    p, d = (statistics.median(t) for t in times)
    print(f"{name:<22s} {shape:<28s} | rate 0: {p:8.1f} us | rate {rate:g}: {d:8.1f} us | ratio {d / p:.3f}", flush=True)


def kernels(dev, iters, rate, B):
    import torch
    import sae_vision_amd.ops as ops
    N, C, Hd = 197, 384, 1536
    M = B * N
    gen = torch.Generator(device=dev).manual_seed(0)
    rng = ops.dropout_rng(dev)
    drop = (float(rate), rng.state, 0)
    x = torch.randn(M, C, device=dev, generator=gen)
    delta = torch.randn(M, C, device=dev, generator=gen).to(torch.bfloat16)
    gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    dy = torch.randn(M, C, device=dev, generator=gen).to(torch.bfloat16)
    xout, _, mean, rstd = ops._ln_fwd(x, delta, gamma, beta, ops.LN_EPS)
    shape = f"M={M} C={C}"
    ab("layernorm_fwd", shape, lambda: ops._ln_fwd(x, delta, gamma, beta, ops.LN_EPS),
       lambda: ops._ln_fwd(x, delta, gamma, beta, ops.LN_EPS, drop), iters, rate)
    ab("layernorm_bwd", shape, lambda: ops._ln_bwd(xout, mean, rstd, gamma, dy, x, True),
       lambda: ops._ln_bwd(xout, mean, rstd, gamma, dy, x, True, drop=drop), iters, rate)

    lib = ops.L.load()
    tok = torch.randn(B, N - 1, C, device=dev, generator=gen).to(torch.bfloat16)
    cls, pos = torch.randn(C, device=dev, generator=gen), torch.randn(N, C, device=dev, generator=gen)
    xt, dtok = torch.empty(B, N, C, device=dev), torch.empty_like(tok)
    dcls, dpos = torch.empty_like(cls), torch.empty_like(pos)
    st, p = ops._stream, ops._ptr
    shape = f"B={B} L={N - 1} E={C}"
    ab("tokens_fwd", shape,
       lambda: ops.L.check(lib.sae_tokens_fwd(st(tok), B, N - 1, C, p(tok), p(cls), p(pos), p(xt))),
       lambda: ops.L.check(lib.sae_tokens_fwd_dropout(st(tok), B, N - 1, C, p(tok), p(cls), p(pos), p(xt), drop[0],
                                                      p(drop[1]), drop[2])), iters, rate)
    ab("tokens_bwd", shape,
       lambda: ops.L.check(lib.sae_tokens_bwd(st(xt), B, N - 1, C, p(xt), p(dtok), p(dcls), p(dpos))),
       lambda: ops.L.check(lib.sae_tokens_bwd_dropout(st(xt), B, N - 1, C, p(xt), p(dtok), p(dcls), p(dpos), drop[0],
                                                      p(drop[1]), drop[2])), iters, rate)

    a = torch.randn(M, C, device=dev, generator=gen).to(torch.bfloat16)
    bt = (torch.randn(Hd, C, device=dev, generator=gen) / 20).to(torch.bfloat16)
    bias = torch.randn(Hd, device=dev, generator=gen)
    c = torch.empty(M, Hd, device=dev, dtype=torch.bfloat16)
    route = lib.sae_gemm_nt_route(M, Hd, C, ops.EPI_GELU_GRAD)
    ab("gemm_nt gelu_grad", f"M={M} K={C} N={Hd} route {route}",
       lambda: ops.gemm_nt(a, bt, bias, ops.EPI_GELU_GRAD, out=c),
       lambda: ops.gemm_nt(a, bt, bias, ops.EPI_GELU_GRAD, out=c, drop=drop), iters, rate)
    h = torch.randn(M, Hd, device=dev, generator=gen).to(torch.bfloat16)
    ab("dropout_rows bf16", f"M={M} C={Hd}", lambda: h.clone(), lambda: ops._dropout_rows_call(h, c, drop), iters, rate)


def step(dev, rate, B, blocks=9, steps=20):
    import torch
    from sae_vision_amd import train, vit
    g = torch.Generator(device=dev).manual_seed(1234)
    images = torch.randn(B, 224, 224, 3, device=dev, generator=g).permute(1, 2, 3, 0).contiguous()
    labels = torch.randint(0, 1000, (B,), device=dev, generator=g)
    runs = []
    for r in (0.0, rate):
        torch.manual_seed(0)
        m = vit.create_model("deit_s_patch16", 1000, torch.bfloat16, device=dev, dropout_rate=r)
        s = train.TrainStep(m, global_batch=B, device=dev, graph=True, input_layout="HWCN")
        for _ in range(10):
            s(images, labels)
        runs.append((s, s.input_buffers() or (images, labels)))
    torch.cuda.synchronize()
    times = [[], []]
    for _ in range(blocks):
        for i, (s, (im, lb)) in enumerate(runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                s(im, lb)
            e1.record()
            e1.synchronize()
            times[i].append(e0.elapsed_time(e1) / steps)
    p, d = (statistics.median(t) for t in times)
    spread = max(times[0]) - min(times[0])
    print(f"{'deit_s step':<22s} {'B=%d 224px graph' % B:<28s} | rate 0: {p:8.3f} ms | rate {rate:g}: {d:8.3f} ms | "
          f"ratio {d / p:.3f} (rate-0 blocks spread {spread:.3f} ms)", flush=True)
    for s, _ in runs:
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    import torch
    dev = torch.device("cuda:0")
    kernels(dev, args.iters, args.rate, args.batch)
    if not args.no_step:
        step(dev, args.rate, args.batch)


if __name__ == "__main__":
    main()
