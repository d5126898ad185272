"""The reference's optimizer chain on the GPU (csrc/adamw.h): the global-norm pass, the prepare
kernel (clip factor, warm-up-cosine schedule, step counter), the update kernels that read the
learning rate and the clip factor from device memory, and the training step built on them -- eager,
as a replayed HIP graph, and with the flag-gated one-rank RCCL collectives.  The float64 reference
is tests/_optim_ref.py."""
import copy
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _optim_ref as R

pytestmark = pytest.mark.gpu

TOL_NORM = 2.0 ** -21   # one exact-square fp64 sum, one fp32 rounding of the root (2^-24), ~5x margin
ADAMW_SHAPES = [(384, 1152), (7,), (1000,), (3, 2051), (384,)]        # test_fused_adamw_matches_torch
CAST_SHAPES = [(68, 100), (68, 36), (384, 1152), (7,), (256, 68)]     # test_fused_adamw_cast_copies
KW = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)


def _lib():
    from sae_vision_amd import _lib as L
    return L.load(), L


def _run_prepare(g, max_norm=math.inf, sched=None, step=None, hyper=None):
    """One sae_adamw_prepare over the fp32 tensor g (None: the schedule alone); returns
    (hyper as four Python floats, the partial sums, step, hyper)."""
    lib, L = _lib()
    dev = step.device if g is None else g.device
    sched = sched or L.LrSchedule(L.SAE_LR_CONSTANT, 0.0, 1e-3, 0.0, 0, 0)
    step = torch.zeros(1, dtype=torch.int32, device=dev) if step is None else step
    hyper = torch.full((4,), -7.0, device=dev) if hyper is None else hyper
    ws = None
    if g is not None:
        nbytes = lib.sae_adamw_prepare_workspace_bytes(g.numel())
        assert nbytes == 8 * -(-g.numel() // L.SAE_ADAMW_NORM_SPAN)
        ws = torch.full((nbytes // 8,), math.nan, dtype=torch.float64, device=dev)   # every partial must be written
    st = torch.cuda.current_stream(dev).cuda_stream
    L.check(lib.sae_adamw_prepare(st, 0 if g is None else g.numel(), None if g is None else g.data_ptr(), max_norm,
                                  ctypes.byref(sched), step.data_ptr(), None if ws is None else ws.data_ptr(),
                                  hyper.data_ptr()))
    return hyper.tolist(), ws, step, hyper


def _norm_cases(dev):
    """(name, tensor handed to the kernel, arrays the reference sums).  Sizes: the smallest, around
    one AdamW chunk, one workgroup's span +-1, three partials more than one pass of the prepare
    kernel adds (with a ragged tail), a base off the 16-byte grid, and a padded flat layout."""
    from sae_vision_amd import train
    _, L = _lib()
    span, per_pass = L.SAE_ADAMW_NORM_SPAN, L.SAE_ADAMW_PREPARE_PASS
    g = torch.Generator(device=dev).manual_seed(17)
    cases = []
    for n in (1, 7, 2047, 2048, 2049, span - 1, span, span + 1, (per_pass + 2) * span + 5):
        x = torch.randn(n, device=dev, generator=g)
        cases.append((f"n{n}", x, [x]))
    for n in (7, 2049, span + 1):       # base pointer offset by one float: the scalar path
        buf = torch.randn(n + 1, device=dev, generator=g)
        x = buf[1:]
        assert x.data_ptr() % 16 == 4
        cases.append((f"n{n}+1f", x, [x]))
    ps = [torch.empty(s, device=dev) for s in ((7,), (1000,), (3, 2051))]
    offs, total = train.flat_layout(ps)
    assert total > sum(p.numel() for p in ps)                      # this one contains padding
    flat = torch.zeros(total, device=dev)
    views = [flat[o:o + p.numel()] for p, o in zip(ps, offs)]
    for v in views:
        v.copy_(torch.randn(v.numel(), device=dev, generator=g))
    cases.append(("flat_layout", flat, views))
    return cases


@pytest.mark.parametrize("kind", ["randn", "one_1e4", "one_1e-20"])
def test_global_norm_matches_float64(dev, kind):
    """sqrt(sum g^2) over every size and layout: |norm - ref| / ref <= 2^-21 against the float64
    reference (the kernel squares and sums in fp64: the squares are exact, the sums are exact to
    ~1e-16 at these sizes, the one fp32 rounding is that of the result), and two runs give the same
    bits, partial sums included."""
    for name, x, parts in _norm_cases(dev):
        if kind == "one_1e4":
            parts[-1].view(-1)[parts[-1].numel() // 2] = 1e4
        elif kind == "one_1e-20":       # its fp32 square is 0: no NaN, no change of the norm
            parts[0].view(-1)[0] = 1e-20
        ref = float(R.global_norm([p.cpu().numpy() for p in parts]))
        h1, ws1, step, _ = _run_prepare(x)
        h2, ws2, _, _ = _run_prepare(x)
        torch.cuda.synchronize()
        norm = h1[2]
        print(f"{kind} {name}: norm {norm!r} ref {ref!r} rel {abs(norm - ref) / ref if ref else 0.0:.3e}")
        assert math.isfinite(norm), (name, norm)
        if ref == 0.0:
            assert norm == 0.0, name
        else:
            assert abs(norm - ref) / ref <= TOL_NORM, (name, norm, ref)
        assert h1[1] == 1.0 and int(step.item()) == 1, (name, h1)        # max_norm = +inf: monitor only
        assert h1 == h2 and torch.equal(ws1, ws2), name
        assert bool(torch.isfinite(ws1).all()), name


def test_prepare_schedule_counter_and_clip(dev):
    """Counts 0..12 of warm-up 3 / decay 10 / peak 3e-3 / end 1e-5: |lr_t - ref| <= 1e-6 peak (the
    fp32 argument of cos is off by at most pi 2^-23, the cosine term by 2e-7 peak: 5x margin);
    *step advances by one per call; clip_scale is exactly 1.0 below max_norm and max / norm to 2^-21
    above it; zero gradients give norm 0 and scale 1; without a gradient buffer only the schedule runs."""
    _, L = _lib()
    peak, sch = 3e-3, (0.0, 3e-3, 3, 10, 1e-5)
    sched = L.LrSchedule(L.SAE_LR_WARMUP_COSINE, sch[0], sch[1], sch[4], sch[2], sch[3])
    x = torch.randn(5000, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    ref_norm = float(R.global_norm([x.cpu().numpy()]))
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    hyper = torch.zeros(4, device=dev)
    for count in range(13):
        above = count % 2 == 1                       # max_norm below the norm on odd counts
        max_norm = 0.37 * ref_norm if above else 1.5 * ref_norm
        h, _, _, _ = _run_prepare(x, max_norm, sched, step, hyper)
        ref_lr = float(R.warmup_cosine(count, *sch))
        print(f"count {count}: lr {h[0]!r} ref {ref_lr!r} clip {h[1]!r} norm {h[2]!r}")
        assert abs(h[0] - ref_lr) <= 1e-6 * peak, (count, h[0], ref_lr)
        assert int(step.item()) == count + 1
        assert abs(h[2] - ref_norm) / ref_norm <= TOL_NORM
        if above:
            want = float(R.clip_scale(ref_norm, max_norm))
            assert abs(h[1] - want) / want <= TOL_NORM, (h[1], want)
        else:
            assert h[1] == 1.0
    # the norm itself as max_norm: not below it, so max / norm, which is exactly 1
    h, _, _, _ = _run_prepare(x, h[2], sched, step, hyper)
    assert h[1] == 1.0
    h, _, _, _ = _run_prepare(torch.zeros(777, device=dev), 1.0, sched, step, hyper)
    assert h[1] == 1.0 and h[2] == 0.0
    # the schedule alone (n = 0, no buffers): constant kind, counter still ticks
    before = int(step.item())
    h, _, _, _ = _run_prepare(None, step=step, hyper=hyper)
    assert h[:3] == [float(np.float32(1e-3)), 1.0, 0.0] and int(step.item()) == before + 1


def test_non_finite_norm_propagates(dev):
    """No silent skip: a NaN gradient gives a NaN norm and a NaN clip factor, an infinite one an
    infinite norm and factor 0 (optax: g / inf * max_norm)."""
    x = torch.randn(3000, device=dev)
    x[1234] = math.nan
    h, _, _, _ = _run_prepare(x, 1.0)
    assert math.isnan(h[2]) and math.isnan(h[1])
    x[1234] = math.inf
    h, _, _, _ = _run_prepare(x, 1.0)
    assert h[2] == math.inf and h[1] == 0.0


def _make(dev, base):
    from sae_vision_amd import train
    ps = [t.clone().requires_grad_(True) for t in base]
    offs, n = train.flat_layout(ps)
    flat = torch.zeros(n, device=dev)
    for p, o in zip(ps, offs):
        p.grad = flat[o:o + p.numel()].view_as(p)
    return ps, flat


def test_dev_update_bit_identical_at_defaults(dev):
    """Constant schedule, max_norm = +inf, five steps: the chunk form of sae_adamw_step_dev gives the
    bits of sae_adamw_step, the tile form those of sae_adamw_step_cast -- parameters, moments, the
    bf16 copies and their transposes, partial 64 x 64 edge tiles (K 68, N 100) included."""
    from sae_vision_amd import train
    g = torch.Generator(device=dev).manual_seed(11)
    for shapes, groups in ((ADAMW_SHAPES, None), (CAST_SHAPES, [[0, 1], [2], [4]])):
        base = [torch.randn(s, device=dev, generator=g) for s in shapes]
        a, fa = _make(dev, base)
        b, fb = _make(dev, base)
        pick = lambda ps: None if groups is None else [[ps[i] for i in grp] for grp in groups]
        opt_a = train.FusedAdamW(a, fa, cast_groups=pick(a), **KW)
        opt_b = train.FusedAdamW(b, fb, cast_groups=pick(b), monitor_norm=True, **KW)
        try:
            assert opt_a.hyper is None and opt_b.hyper is not None
            assert (opt_b.n_tiles > 0) == (groups is not None) and opt_a.n_tiles == opt_b.n_tiles
            for _ in range(5):
                for p, q in zip(a, b):
                    gr = torch.randn(p.shape, device=dev, generator=g)
                    p.grad.copy_(gr)
                    q.grad.copy_(gr)
                opt_a.step()
                opt_b.step()
                assert float(opt_b.lr_now) == float(np.float32(KW["lr"]))
                assert abs(float(opt_b.grad_norm) - float(fb.double().norm())) <= TOL_NORM * float(fb.double().norm())
            assert int(opt_a.step_count.item()) == int(opt_b.step_count.item()) == 5
            for p, q in zip(a, b):
                assert torch.equal(p, q)
            assert torch.equal(opt_a.m, opt_b.m) and torch.equal(opt_a.v, opt_b.v)
            for (w16a, wt16a), (w16b, wt16b) in zip(opt_a.copies, opt_b.copies):
                assert torch.equal(w16a, w16b) and torch.equal(wt16a, wt16b)
            for ws, (w16, wt16) in zip(opt_b.cast_groups, opt_b.copies):
                ref = torch.cat([w.detach() for w in ws], dim=1).to(torch.bfloat16)
                assert torch.equal(w16, ref) and torch.equal(wt16, ref.t().contiguous())
        finally:
            opt_a.close()
            opt_b.close()


def test_dev_update_matches_float64(dev):
    """Five steps with the clip triggering on steps 3 and 5 only and a 2-step warm-up crossing into
    the cosine, against the float64 helper: max |p - ref| / max |ref| <= 2e-6 per tensor, the measure
    and bound of test_fused_adamw_matches_torch.  The helper's own fp32 execution against float64 is
    printed beside the kernel's figure (measured on an MI355X: 2.6e-7 for both at the worst tensor,
    the same figure tensor by tensor, so the clip's extra rounding needs no wider bound).  The tile form with the
    bf16 copies gives the same parameter bits as the chunk form under the clip as well."""
    from sae_vision_amd import train
    g = torch.Generator(device=dev).manual_seed(11)
    base = [torch.randn(s, device=dev, generator=g) for s in ADAMW_SHAPES]
    mine, flat = _make(dev, base)
    cast, flat_c = _make(dev, base)
    numel = sum(t.numel() for t in base)
    clip = 1.05 * math.sqrt(numel)                     # a randn gradient's norm is ~ sqrt(numel)
    amps = [1.0, 0.5, 2.0, 0.25, 1.5]
    sch = (0.0, 3e-3, 2, 8, 1e-5)
    kw = dict(KW, clip_grad=clip, lr_schedule=train.WarmupCosine(*sch))
    opt = train.FusedAdamW(mine, flat, **kw)
    opt_c = train.FusedAdamW(cast, flat_c, cast_groups=[[cast[0]]], **kw)
    r64 = [[t.cpu().numpy().astype(np.float64), np.zeros(t.shape), np.zeros(t.shape)] for t in base]
    r32 = [[t.cpu().numpy().copy(), np.zeros(t.shape, np.float32), np.zeros(t.shape, np.float32)] for t in base]
    clipped = []
    try:
        assert opt_c.n_tiles > 0 and opt.n_tiles == 0
        for k, amp in enumerate(amps):
            grads = [torch.randn(p.shape, device=dev, generator=g) * amp for p in mine]
            for p, q, gr in zip(mine, cast, grads):
                p.grad.copy_(gr)
                q.grad.copy_(gr)
            opt.step()
            opt_c.step()
            gn = [gr.cpu().numpy() for gr in grads]
            norm = R.global_norm(gn)
            scale, lr = R.clip_scale(norm, clip), R.warmup_cosine(k, *sch)
            clipped.append(bool(norm >= clip))
            assert abs(float(opt.grad_norm) - norm) <= TOL_NORM * norm
            assert abs(float(opt.lr_now) - lr) <= 1e-6 * sch[1]
            for (p, m, v), (p3, m3, v3), gr in zip(r64, r32, gn):
                R.adamw_step(p, gr, m, v, k + 1, lr, scale, *KW["betas"], KW["eps"], KW["weight_decay"])
                R.adamw_step(p3, gr, m3, v3, k + 1, np.float32(lr), np.float32(scale), *KW["betas"], KW["eps"],
                             KW["weight_decay"])
        assert clipped == [False, False, True, False, True], clipped
        assert int(opt.step_count.item()) == 5
        worst = 0.0
        for t, q, (p, _, _), (p3, _, _) in zip(mine, cast, r64, r32):
            err = float(np.abs(t.detach().cpu().numpy() - p).max() / np.abs(p).max())
            own = float(np.abs(p3 - p).max() / np.abs(p).max())
            print(f"{tuple(t.shape)}: kernel vs float64 {err:.3e}; the helper in fp32 vs float64 {own:.3e}")
            worst = max(worst, err)
            assert torch.equal(t, q), tuple(t.shape)
        assert worst <= 2e-6, worst
        w16, wt16 = opt_c.copies[0]
        ref16 = cast[0].detach().to(torch.bfloat16)
        assert torch.equal(w16, ref16) and torch.equal(wt16, ref16.t().contiguous())
    finally:
        opt.close()
        opt_c.close()


def _first_step_norm(model, dev, x, y):
    """The global gradient norm of one forward + backward of a copy of ``model`` (float64)."""
    from sae_vision_amd import train
    s = train.TrainStep(copy.deepcopy(model), global_batch=x.shape[0], device=dev)
    s._fwd_bwd(x, y)
    norm = float(s._flat.double().norm())
    s.close()
    return norm


def test_graph_replay_with_clip_and_schedule(dev):
    """deit_ti_patch16, batch 8, 7 steps: the replayed graph step with clip_grad and a WarmupCosine
    gives the losses and parameters of the eager step bit for bit; after every replay opt.lr_now is
    the schedule at that count (it could not be if the rate were captured by value) and
    opt.grad_norm the norm of that step's flat gradient to 2^-21.  clip_grad is the first step's
    norm, so later steps fall on both sides of it."""
    from sae_vision_amd import train, vit
    torch.manual_seed(0)
    m_e = vit.create_model("deit_ti_patch16", 1000, torch.bfloat16, device=dev)
    m_g = copy.deepcopy(m_e)
    g = torch.Generator(device=dev).manual_seed(3)
    data = [(torch.randn(8, 224, 224, 3, device=dev, generator=g),
             torch.randint(0, 1000, (8,), device=dev, generator=g)) for _ in range(7)]
    clip = _first_step_norm(m_e, dev, *data[0])
    sch = (0.0, 1e-3, 3, 8, 1e-5)
    kw = dict(global_batch=8, device=dev, clip_grad=clip, lr_schedule=train.WarmupCosine(*sch))
    s_e = train.TrainStep(m_e, **kw)
    s_g = train.TrainStep(m_g, graph=True, **kw)
    try:
        assert isinstance(s_e.opt, train.FusedAdamW) and isinstance(s_g.opt, train.FusedAdamW)
        le, lg, scales = [], [], []
        for count, (x, y) in enumerate(data):
            le.append(float(s_e(x, y)))
            lg.append(float(s_g(x, y)))
            assert s_g._g is not None and s_g.graph
            ref_lr = float(R.warmup_cosine(count, *sch))
            ref_norm = float(s_g._flat.double().norm())
            lr, norm, scale = float(s_g.lr_now), float(s_g.grad_norm), float(s_g.opt.hyper[1])
            print(f"step {count}: lr {lr!r} ref {ref_lr!r}; norm {norm!r} ref {ref_norm!r} clip {clip!r} scale {scale!r}")
            assert abs(lr - ref_lr) <= 1e-6 * sch[1], (count, lr, ref_lr)
            assert abs(norm - ref_norm) <= TOL_NORM * ref_norm, (count, norm, ref_norm)
            assert float(s_e.lr_now) == lr and float(s_e.grad_norm) == norm
            assert int(s_g.opt.step_count.item()) == count + 1
            assert scale == (1.0 if norm < float(np.float32(clip)) else float(np.float32(clip) / np.float32(norm)))
            scales.append(scale)
        assert le == lg, (le, lg)
        assert any(sc < 1.0 for sc in scales) and sum(sc == 1.0 for sc in scales) >= 2, scales   # both sides
        for (n, pe), pg in zip(m_e.named_parameters(), m_g.parameters()):
            assert torch.equal(pe, pg), n
    finally:
        s_g.close()
        s_e.close()


def test_world1_rccl_flagged_step_with_clip_and_schedule(dev):
    """tests/world1_rccl_optim_case.py in a child process (it owns the RCCL communicator and the
    graphs that captured its collectives): the one-rank flag-gated step with clip and schedule is
    bit-equal, losses and parameters, to the no-collective graph step with the same arguments."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "world1_rccl_optim_case.py")
    env = {k: v for k, v in os.environ.items() if k != "SAE_FLAGGED"}      # the default: flagged
    r = subprocess.run([sys.executable, "-u", script, "deit_ti_patch16"], capture_output=True, text=True, timeout=110,
                       env=env)
    assert r.returncode == 0 and "WORLD1_OPTIM_OK" in r.stdout, \
        f"rc {r.returncode}\nstdout:\n{r.stdout[-2000:]}\nstderr:\n{r.stderr[-4000:]}"


def test_graph_refused_with_the_torch_optimizer(dev):
    """clip_grad / lr_schedule with graph=True need FusedAdamW: a step whose parameters take
    torch.optim.AdamW (here: no flat gradient buffer) raises instead of ignoring them; without
    graph=True the same step applies them eagerly."""
    from sae_vision_amd import train, vit
    torch.manual_seed(0)
    m = vit.create_model("deit_ti_patch16", 1000, torch.bfloat16, device=dev)
    with pytest.raises(ValueError, match="FusedAdamW"):
        train.TrainStep(m, global_batch=8, device=dev, graph=True, flat_grads=False, clip_grad=1.0)
    with pytest.raises(ValueError, match="FusedAdamW"):
        train.TrainStep(m, global_batch=8, device=dev, graph=True, flat_grads=False,
                        lr_schedule=train.WarmupCosine(0.0, 1e-3, 1, 4))
    s = train.TrainStep(m, global_batch=8, device=dev, flat_grads=False, clip_grad=1.0,
                        lr_schedule=train.WarmupCosine(0.0, 1e-3, 1, 4))
    assert not isinstance(s.opt, train.FusedAdamW)
    x = torch.randn(8, 224, 224, 3, device=dev)
    y = torch.randint(0, 1000, (8,), device=dev)
    s(x, y)
    s(x, y)
    assert s.lr_now == pytest.approx(1e-3) and float(s.grad_norm) > 0.0
    assert s.opt.param_groups[0]["lr"] == pytest.approx(1e-3)
