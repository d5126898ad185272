"""CPU side of the mixup / cutmix loss, top-k and the evaluation step: the torch branches of
train.mixed_cross_entropy / train.topk_correct against a numpy restatement of the reference
(train.py:83-90, utils.topk_correct with a stable argsort), the host-side validation of the new
C-ABI entry points (no GPU touched), and TrainStep(mix=True) / EvalStep over gloo at world size 2
against one process on the whole batch."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _reference_loss(x, y0, y1, rho, alpha):
    """train.py:83-90 in float64: one-hot, mix, optax.smooth_labels, mean softmax cross entropy."""
    x = x.astype(np.float64)
    K = x.shape[1]
    t = np.eye(K)[y0]
    if y1 is not None:
        t = rho[:, None] * t + (1.0 - rho[:, None]) * np.eye(K)[y1]
    t = (1.0 - alpha) * t + alpha / K
    logp = x - x.max(1, keepdims=True)
    logp = logp - np.log(np.exp(logp).sum(1, keepdims=True))
    return float(-(t * logp).sum(1).mean())


@pytest.mark.parametrize("alpha", [0.1, 0.0])
def test_cpu_mixed_loss_is_the_reference_formula(alpha):
    from sae_vision_amd import train
    g = torch.Generator().manual_seed(2)
    x = 3 * torch.randn(33, 17, generator=g)
    y0, y1 = torch.randint(0, 17, (33,), generator=g), torch.randint(0, 17, (33,), generator=g)
    rho = torch.rand(33, generator=g)
    rho[0::5], rho[1::5] = 0.0, 1.0
    y1[2::5] = y0[2::5]
    want = _reference_loss(x.numpy(), y0.numpy(), y1.numpy(), rho.double().numpy(), alpha)
    got = train.mixed_cross_entropy(x, y0, y1, rho, alpha)
    assert abs(float(got) - want) <= 1e-6 * abs(want)
    plain = train.mixed_cross_entropy(x, y0, smoothing=alpha)
    assert abs(float(plain) - _reference_loss(x.numpy(), y0.numpy(), None, None, alpha)) <= 1e-6 * abs(float(plain))
    torch.testing.assert_close(plain, train.smoothed_cross_entropy(x, y0, alpha))
    # the gradient flows through the CPU branch (the gloo step below relies on it)
    xa = x.clone().requires_grad_(True)
    train.mixed_cross_entropy(xa, y0, y1, rho, alpha).backward()
    assert xa.grad is not None and torch.isfinite(xa.grad).all()
    with pytest.raises(ValueError, match="go together"):
        train.mixed_cross_entropy(x, y0, ratio=rho)
    # the HIP loss gives a label outside the classes no target term; the CPU branch refuses it
    with pytest.raises(ValueError, match="outside"):
        train.mixed_cross_entropy(x, torch.full_like(y0, 17), y1, rho, alpha)
    with pytest.raises(ValueError, match="mix_labels outside"):
        train.mixed_cross_entropy(x, y0, torch.full_like(y1, -1), rho, alpha)


@pytest.mark.parametrize("K", [3, 5, 6, 37])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_cpu_topk_is_the_stable_argsort(K, dt):
    from sae_vision_amd import train
    g = torch.Generator().manual_seed(K)
    R = 200
    x = torch.randint(-3, 4, (R, K), generator=g).float()
    u = torch.rand(R, K, generator=g)
    x[u < 0.02] = float("nan")
    x[(u >= 0.02) & (u < 0.07)] = -0.0
    x = x.to(dt)
    y = torch.randint(0, K, (R,), generator=g)
    order = np.argsort(x.float().numpy(), axis=1, kind="stable")
    rank = train.label_ranks(x, y).numpy()
    pos = (order == y.numpy()[:, None]).argmax(1)
    assert np.array_equal(rank, K - 1 - pos)
    top1, top5 = train.topk_correct(x, y)
    for k, got in ((1, top1), (5, top5)):
        want = (order[:, -k:] == y.numpy()[:, None]).any(1)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy() > 0, want)
    (top3,) = train.topk_correct(x, y, topk=(3,))
    assert np.array_equal(top3.numpy() > 0, (order[:, -3:] == y.numpy()[:, None]).any(1))
    loss, m1, m5 = train.mixed_cross_entropy(x.float().nan_to_num(), y, metrics=True)
    assert m1.dim() == 0 and 0.0 <= float(m1) <= float(m5) <= 1.0
    # a label outside the classes ranks K: in no top-k with k <= K
    bad = torch.full((R,), K)
    assert bool((train.label_ranks(x, bad) == K).all())
    assert float(train.topk_correct(x, bad, topk=(min(K, 5),))[0].sum()) == 0.0


def test_cpu_topk_tie_at_the_fifth_place():
    """bf16 3 randn at K = 1000: the label at the 6th place of the stable order in rows whose 5th and
    6th largest logits are equal is not top-5, though only four logits are strictly greater."""
    from sae_vision_amd import train
    g = torch.Generator().manual_seed(5)
    x = (3 * torch.randn(1024, 1000, generator=g)).to(torch.bfloat16)
    xn = x.float().numpy()
    order = np.argsort(xn, axis=1, kind="stable")
    rows = np.arange(xn.shape[0])
    tied = np.nonzero(xn[rows, order[:, -5]] == xn[rows, order[:, -6]])[0]
    assert len(tied) >= 16
    y = torch.from_numpy(order[tied, -6])
    xs = x[torch.from_numpy(tied)]
    assert int((xs.float() > xs.float().gather(1, y[:, None])).sum(1).max()) == 4
    assert int((train.label_ranks(xs, y) == 5).sum()) == len(tied)
    assert float(train.topk_correct(xs, y)[1].sum()) == 0.0


def test_new_entry_points_validate_on_the_host():
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    d = ctypes.c_void_p(256)
    err = lambda: lib.sae_last_error().decode()
    fwd = lambda rows=8, K=10, ld=10, dt=L.SAE_DTYPE_BF16, mix=None, ratio=None, rank=None, top=None, lse=d: \
        lib.sae_mixed_ce_fwd(None, rows, K, d, ld, dt, d, mix, ratio, 0.1, lse, d, rank, d, top)
    assert fwd(rows=0) == L.SAE_EINVAL and "rows 0" in err()
    assert fwd(dt=7) == L.SAE_EINVAL and "bad dtype 7" in err()
    assert fwd(ld=9) == L.SAE_EINVAL and "ld 9" in err()
    assert fwd(ratio=d) == L.SAE_EINVAL and "mix_labels and ratio" in err()
    assert fwd(mix=d) == L.SAE_EINVAL and "mix_labels and ratio" in err()
    assert fwd(rank=d) == L.SAE_EINVAL and "rank and top" in err()
    assert fwd(lse=None) == L.SAE_EINVAL and "NULL lse" in err()
    bwd = lambda rows=8, K=10, dt=L.SAE_DTYPE_F32, mix=None, ratio=None, ldd=10: \
        lib.sae_mixed_ce_bwd(None, rows, K, d, 10, dt, d, mix, ratio, 0.1, d, d, d, ldd)
    assert bwd(rows=0) == L.SAE_EINVAL and "rows 0" in err()
    assert bwd(dt=5) == L.SAE_EINVAL and "bad dtype 5" in err()
    assert bwd(ratio=d) == L.SAE_EINVAL and "mix_labels and ratio" in err()
    assert bwd(ldd=9) == L.SAE_EINVAL and "ldd < classes" in err()
    assert lib.sae_ce_accumulate(None, 0, d, d, d) == L.SAE_EINVAL and "rows 0" in err()
    assert lib.sae_ce_accumulate(None, 8, d, None, d) == L.SAE_EINVAL and "NULL" in err()
    assert lib.sae_ce_accumulate(None, 8, d, d, ctypes.c_void_p(260)) == L.SAE_EINVAL and "8-byte" in err()
    assert L.SAE_CE_ACCUM_BYTES == 32


def test_a_refusal_names_the_entry_point_called():
    """sae_smoothed_ce_* forwards to the host path of sae_mixed_ce_*; each refusal still names the
    function the caller called (no GPU touched: the refusals return before any HIP call)."""
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    lib = sae_vision_amd.load_library()
    d = ctypes.c_void_p(256)
    err = lambda: lib.sae_last_error().decode()
    assert lib.sae_smoothed_ce_fwd(None, 0, 10, d, 10, L.SAE_DTYPE_BF16, d, 0.1, d, d, d) == L.SAE_EINVAL
    assert err().startswith("smoothed_ce_fwd:") and "rows 0" in err()
    assert lib.sae_mixed_ce_fwd(None, 0, 10, d, 10, L.SAE_DTYPE_BF16, d, None, None, 0.1, d, d, None, d, None) == L.SAE_EINVAL
    assert err().startswith("mixed_ce_fwd:") and "rows 0" in err()
    assert lib.sae_smoothed_ce_bwd(None, 8, 10, d, 10, L.SAE_DTYPE_F32, d, 0.1, d, d, d, 9) == L.SAE_EINVAL
    assert err().startswith("smoothed_ce_bwd:") and "ldd < classes" in err()
    assert lib.sae_mixed_ce_bwd(None, 8, 10, d, 10, 7, d, None, None, 0.1, d, d, d, 10) == L.SAE_EINVAL
    assert err().startswith("mixed_ce_bwd:") and "bad dtype 7" in err()
    assert lib.sae_smoothed_ce_fwd(None, 8, 10, d, 10, L.SAE_DTYPE_BF16, d, 0.1, None, d, d) == L.SAE_EINVAL
    assert err().startswith("smoothed_ce_fwd:") and "NULL lse" in err()


def test_step_refuses_mismatched_mix_arguments():
    from sae_vision_amd import train
    from test_dp_gloo import TinyNet, _data
    x, y = _data()
    with pytest.raises(ValueError, match="need mix=True"):
        train.TrainStep(TinyNet(), global_batch=8)(x, y, y, torch.ones(8))
    with pytest.raises(ValueError, match="every call needs"):
        train.TrainStep(TinyNet(), global_batch=8, mix=True)(x, y)


# ---- gloo, world size 2
def _mix_data():
    from test_dp_gloo import _data
    x, y = _data()
    g = torch.Generator().manual_seed(4)
    return x, y, torch.randint(0, 5, (8,), generator=g), torch.rand(8, generator=g)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    from sae_vision_amd import train
    from test_dp_gloo import TinyNet
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, y, y1, rho = _mix_data()
    per = x.shape[0] // world
    sl = slice(rank * per, (rank + 1) * per)
    step = train.TrainStep(TinyNet(seed=rank), global_batch=x.shape[0], bucket_cap_mb=0.0001, mix=True, metrics=True)
    for _ in range(3):
        step(x[sl], y[sl], y1[sl], rho[sl])
    top = (float(step.top1), float(step.top5))
    flat = torch.cat([p.detach().flatten() for p in step.model.parameters()])
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    ev = train.EvalStep(TinyNet(seed=3))   # the same weights on every rank, as after a broadcast
    for _ in range(2):   # two passes: the accumulator keeps adding
        ev(x[sl], y[sl])
    res = ev.result()
    ev.reset()
    empty = ev.result()
    tops = [None] * world
    dist.all_gather_object(tops, top)
    if rank == 0:
        torch.save({"params": torch.stack(gathered), "eval": res, "empty": empty, "tops": tops}, out)
    step.close()
    dist.barrier()   # no rank tears its group down while a peer is still in a collective
    dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_gloo_mix_step_and_eval_match_single_process(tmp_path):
    from sae_vision_amd import train
    from test_dp_gloo import TinyNet
    out = str(tmp_path / "mix.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out, weights_only=False)
    assert torch.equal(got["params"][0], got["params"][1]), "ranks diverged"
    x, y, y1, rho = _mix_data()
    ref = train.TrainStep(TinyNet(), global_batch=x.shape[0], mix=True, metrics=True)
    plain = train.TrainStep(TinyNet(), global_batch=x.shape[0])
    for _ in range(3):
        # the third step's metrics see the parameters after two updates, on every rank's own half
        with torch.no_grad():
            logits = ref.model(x, False)
        ref(x, y, y1, rho)
        plain(x, y)
    flat = torch.cat([p.detach().flatten() for p in ref.model.parameters()])
    torch.testing.assert_close(got["params"][0], flat, rtol=1e-5, atol=1e-6)
    # ... and the partner labels were felt
    assert not torch.allclose(flat, torch.cat([p.detach().flatten() for p in plain.model.parameters()]), atol=1e-5)
    for r, (t1, t5) in enumerate(got["tops"]):
        h1, h5 = train.topk_correct(logits[4 * r:4 * r + 4], y[4 * r:4 * r + 4])
        assert (t1, t5) == (float(h1.mean()), float(h5.mean()))
    net = TinyNet(seed=3)
    before = [p.detach().clone() for p in net.parameters()]
    ev = train.EvalStep(net)
    for _ in range(2):
        loss = ev(x, y)
    assert loss.dim() == 0 and all(p.grad is None for p in net.parameters())
    assert all(torch.equal(p, b) for p, b in zip(net.parameters(), before))
    want = ev.result()
    res = got["eval"]
    assert res["samples"] == want["samples"] == 16
    assert (res["top_1_acc"], res["top_5_acc"]) == (want["top_1_acc"], want["top_5_acc"])
    assert abs(res["loss"] - want["loss"]) <= 1e-6 * abs(want["loss"])
    ce = torch.nn.functional.cross_entropy(net(x, False).detach().double(), y)
    assert abs(want["loss"] - float(ce)) <= 1e-6 * float(ce)
    assert got["empty"] == {"loss": 0.0, "top_1_acc": 0.0, "top_5_acc": 0.0, "samples": 0}
