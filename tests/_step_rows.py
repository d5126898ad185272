"""The structure of a training step (train.step_plan) restated, and one pinned plan per structure that
bench.py and the tests reach.  Shared by tests/test_step_plan_cpu.py.

``constructor_structure`` is read off the branch cascade of ``TrainStep.__init__`` that ``step_plan``
replaced, statement by statement in that constructor's order, not off the plan:
  * ``graph = bool(graph) and torch.cuda.is_available()``;
  * ``flat = (pg or on_gpu) if flat_grads is None else bool(flat_grads)``; the one-launch optimizer iff
    flat, on the GPU, every parameter fp32 contiguous; clip / schedule with graph and without it: refused;
  * no process group: "none"; GPU parameters on a gloo group: "host"; a truthy ``two_graphs``: "between";
    else "overlap"; a collective without the flat buffer: refused;
  * the RCCL gradient group for "overlap" / "between" on the GPU; the gloo agreement group at world > 1
    with graph; flagged = "overlap", graph, GPU, SAE_FLAGGED != "0"; two graphs for "between", "host",
    "none" with a truthy ``two_graphs``, or flagged;
  * inside ``if flat:`` the hooks for "overlap", and inside the arming a communication stream if the flat
    buffer is on the GPU;
  * the weight-gradient stream if asked, flat, grad_sinks, GPU; the sinks if flat and grad_sinks, with the
    listener for "overlap"; ``capturable`` for the torch optimizer under graph; capture mode
    "thread_local" with a process group, else "global".
"""
import sae_vision_amd.train as train

REFUSE_CLIP = ("TrainStep: clip_grad / lr_schedule with graph=True need the one-launch FusedAdamW "
               "(fp32 contiguous GPU parameters, flat gradients); torch.optim.AdamW applies them "
               "eagerly from the host")
REFUSE_FLAT = "TrainStep: the collective path needs the flat gradient buffer"


def constructor_structure(f):
    """The StepPlan fields as a dict; raises what the constructor raised."""
    s = {}
    s["graph"] = bool(f.graph) and f.cuda
    s["flat"] = (f.pg or f.on_gpu) if f.flat_grads is None else bool(f.flat_grads)
    s["fused"] = s["flat"] and f.on_gpu and f.fp32_contiguous
    if s["graph"] and not s["fused"] and f.clip_or_schedule:
        raise ValueError(REFUSE_CLIP)
    if not f.pg:
        s["collective"] = "none"
    elif f.on_gpu and f.backend == "gloo":
        s["collective"] = "host"
    elif f.two_graphs:
        s["collective"] = "between"
    else:
        s["collective"] = "overlap"
    if s["collective"] != "none" and not s["flat"]:
        raise ValueError(REFUSE_FLAT)
    s["grad_group"] = s["collective"] in ("overlap", "between") and f.on_gpu
    s["agree_group"] = f.world > 1 and s["graph"]
    s["flagged"] = s["collective"] == "overlap" and s["graph"] and f.on_gpu and f.flagged_on
    s["two_graphs"] = (s["collective"] in ("between", "host") or (s["collective"] == "none" and bool(f.two_graphs))
                       or s["flagged"])
    s["hooks"] = s["comm_stream"] = False
    if s["flat"]:
        if s["collective"] == "overlap":
            s["hooks"] = True
            if f.on_gpu:
                s["comm_stream"] = True
    s["wgrad_stream"] = bool(f.wgrad_stream and s["flat"] and f.grad_sinks and f.on_gpu)
    s["sinks"] = bool(s["flat"] and f.grad_sinks)
    s["sink_listener"] = s["sinks"] and s["collective"] == "overlap"
    s["capturable"] = s["graph"]
    s["capture_mode"] = "thread_local" if f.pg else "global"
    return s


# bench.py's default step on one GPU, and the default RCCL step on eight
_ONE = train.StepPlan(graph=True, flat=True, fused=True, collective="none", flagged=False, two_graphs=False,
                      grad_group=False, agree_group=False, hooks=False, comm_stream=False, sinks=True,
                      sink_listener=False, wgrad_stream=False, capturable=True, capture_mode="global")
_EIGHT = train.StepPlan(graph=True, flat=True, fused=True, collective="overlap", flagged=True, two_graphs=True,
                        grad_group=True, agree_group=True, hooks=True, comm_stream=True, sinks=True,
                        sink_listener=True, wgrad_stream=False, capturable=True, capture_mode="thread_local")
_RCCL8 = dict(pg=True, backend="nccl", world=8)

# (id, step_facts_of_values arguments, the plan)
PINS = [
    ("bench_n1", dict(), _ONE),
    ("bench_n1_two_graphs", dict(two_graphs=True), _ONE._replace(two_graphs=True)),
    ("bench_n1_eager", dict(graph=False), _ONE._replace(graph=False, capturable=False)),
    ("bench_n1_no_flat_grads", dict(flat_grads=False),
     _ONE._replace(flat=False, fused=False, sinks=False)),   # torch.optim.AdamW, per-parameter gradients
    ("rccl_n8", _RCCL8, _EIGHT),
    ("rccl_n8_unflagged", dict(_RCCL8, flagged_on=False), _EIGHT._replace(flagged=False, two_graphs=False)),
    ("rccl_n8_two_graphs", dict(_RCCL8, two_graphs=True),
     _EIGHT._replace(collective="between", flagged=False, hooks=False, comm_stream=False, sink_listener=False)),
    ("gloo_rehearsal_gpu", dict(pg=True, backend="gloo", world=2),
     _EIGHT._replace(collective="host", flagged=False, grad_group=False, hooks=False, comm_stream=False,
                     sink_listener=False)),
    ("world1_rccl", dict(pg=True, backend="nccl", world=1), _EIGHT._replace(agree_group=False)),
    ("world1_rccl_unflagged", dict(pg=True, backend="nccl", world=1, flagged_on=False),
     _EIGHT._replace(agree_group=False, flagged=False, two_graphs=False)),
    # tests/test_dp_gloo.py: CPU parameters, gloo, world 2, graph=False
    ("cpu_gloo_world2", dict(pg=True, backend="gloo", world=2, on_gpu=False, cuda=False, graph=False),
     _EIGHT._replace(graph=False, fused=False, flagged=False, two_graphs=False, grad_group=False,
                     agree_group=False, comm_stream=False, capturable=False)),
]
