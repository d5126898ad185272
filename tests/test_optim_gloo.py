"""World-2 gloo (CPU): the global-norm clip sees the all-reduced gradient.

Same harness as tests/test_dp_gloo.py (its TinyNet, data and comparison).  Each rank's local
gradient has its own norm; clipping it before the SUM all-reduce would give parameters that
differ from a single process stepping on the concatenated batch.  With the clip triggering, the
two-rank parameters must equal the single-process ones: the clip runs after the all-reduce."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dp_gloo import TinyNet, _data, _free_port

CLIP = 0.05
SCHED = (0.0, 2e-3, 2, 6, 1e-5)


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from sae_vision_amd import train
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, y = _data()
    per = x.shape[0] // world
    step = train.TrainStep(TinyNet(seed=rank), global_batch=x.shape[0], bucket_cap_mb=0.0001, clip_grad=CLIP,
                           lr_schedule=train.WarmupCosine(*SCHED))
    assert step.collective == "overlap" and not isinstance(step.opt, train.FusedAdamW)
    norms = []
    for _ in range(3):
        step(x[rank * per:(rank + 1) * per], y[rank * per:(rank + 1) * per])
        norms.append(float(step.grad_norm))
    flat = torch.cat([p.detach().flatten() for p in step.model.parameters()])
    gathered = [torch.zeros_like(flat) for _ in range(world)]
    dist.all_gather(gathered, flat)
    allnorms = [None] * world
    dist.all_gather_object(allnorms, norms)
    if rank == 0:
        torch.save({"params": torch.stack(gathered), "norms": torch.tensor(allnorms)}, out)
    dist.destroy_process_group()


def test_clip_runs_after_the_all_reduce(tmp_path):
    from sae_vision_amd import train
    out = str(tmp_path / "clip.pt")
    mp.spawn(_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    got = torch.load(out, weights_only=True)
    assert torch.equal(got["params"][0], got["params"][1]), "ranks diverged"
    assert torch.equal(got["norms"][0], got["norms"][1]), "ranks saw different norms"
    x, y = _data()
    ref = train.TrainStep(TinyNet(), global_batch=x.shape[0], clip_grad=CLIP, lr_schedule=train.WarmupCosine(*SCHED))
    norms = []
    for _ in range(3):
        ref(x, y)
        norms.append(float(ref.grad_norm))
    assert min(norms) > CLIP, norms                      # the clip triggered on every step
    torch.testing.assert_close(got["norms"][0], torch.tensor(norms), rtol=1e-5, atol=0)
    flat = torch.cat([p.detach().flatten() for p in ref.model.parameters()])
    torch.testing.assert_close(got["params"][0], flat, rtol=1e-5, atol=1e-6)
