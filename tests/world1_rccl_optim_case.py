"""Child process of tests/test_gpu_optim.py::test_world1_rccl_flagged_step_with_clip_and_schedule (GPU).

    python tests/world1_rccl_optim_case.py <deit_ti_patch16>

The collective path of the multi-rank step on one GPU (as tests/world1_rccl_case.py: a one-rank
RCCL group, the bucket all-reduces on the communication stream behind device flags the captured
backward bumps, the optimizer in a graph of its own behind the join) with the reference's clip and
schedule: the global-norm pass is captured with the update, so it runs after the all-reduces have
been joined.  A one-rank SUM is the identity, so losses, parameters, learning rates and norms must
equal those of the no-collective graph step with the same arguments bit for bit.  Prints
WORLD1_OPTIM_OK on success.
"""
import copy
import os
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(model):
    import torch
    import torch.distributed as dist
    from sae_vision_amd import train, vit
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m_a = vit.create_model(model, 1000, torch.bfloat16, device=dev)
    m_b = copy.deepcopy(m_a)
    g = torch.Generator(device=dev).manual_seed(3)
    data = [(torch.randn(8, 224, 224, 3, device=dev, generator=g),
             torch.randint(0, 1000, (8,), device=dev, generator=g)) for _ in range(4)]
    # clip_grad: just under the first step's norm, so that step is clipped for certain
    probe = train.TrainStep(copy.deepcopy(m_a), global_batch=8, device=dev)
    probe._fwd_bwd(*data[0])
    clip = 0.97 * float(probe._flat.double().norm())
    probe.close()
    kw = dict(global_batch=8, device=dev, graph=True, clip_grad=clip,
              lr_schedule=train.WarmupCosine(0.0, 1e-3, 2, 6, 1e-5))
    s_a = train.TrainStep(m_a, **kw)
    assert s_a.collective == "none"
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)   # as train.init_distributed
    s_b = None
    try:
        s_b = train.TrainStep(m_b, bucket_cap_mb=4.0, **kw)
        assert s_b.collective == "overlap" and len(s_b.reducer.buckets) > 1
        la, lb, ha, hb = [], [], [], []
        for x, y in data:
            la.append(float(s_a(x, y)))
            ha.append(s_a.opt.hyper.tolist())
        for x, y in data:
            lb.append(float(s_b(x, y)))
            hb.append(s_b.opt.hyper.tolist())
        assert s_b._flagged and s_b._g is not None and s_b._g_opt is not None and s_b.graph
        assert sorted(s_b.reducer.flag_order) == list(range(len(s_b.reducer.buckets)))
        assert la == lb, (la, lb)
        assert ha == hb, (ha, hb)                        # lr_t, clip_scale, grad_norm of every step
        assert all(abs(h[0] - want) <= 1e-9 for h, want in zip(hb, (0.0, 5e-4, 1e-3))), hb
        assert all(h[2] > 0.0 for h in hb) and any(h[1] < 1.0 for h in hb)
        for (n, pa), pb in zip(m_a.named_parameters(), m_b.parameters()):
            assert torch.equal(pa, pb), n
    finally:
        # the captured graph holds RCCL collectives: it goes before the communicator
        if s_b is not None:
            s_b.close()
        s_a.close()
        dist.destroy_process_group()
    print("WORLD1_OPTIM_OK", flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
