"""The training step's structure (train.step_plan): a pure function of a step's facts, so no device and
no process group is needed.  tests/_step_rows.py restates the decisions of the constructor the plan
replaced and pins one plan per structure that bench.py and the tests reach."""
import itertools

import pytest
import torch

import _step_rows as R
import sae_vision_amd.train as train
from sae_vision_amd.sinks import GradSinks

TF = (False, True)


def _all_facts():
    """Every combination of the facts' values: 2 ** 11 * 3 * 3 = 18432."""
    for pg, backend, world, on_gpu, f32, cuda, graph, flat, sinks, two, wg, flagged_on, clip in itertools.product(
            TF, ("gloo", "nccl"), (1, 2), TF, TF, TF, TF, (None, True, False), TF, (None, True, False), TF, TF, TF):
        yield train.StepFacts(pg, backend, world, on_gpu, f32, cuda, graph, flat, sinks, two, wg, clip, flagged_on)


def _outcome(fn, f):
    try:
        return fn(f)
    except Exception as e:   # noqa: BLE001 (the refusal is the outcome)
        return type(e), str(e)


def test_plan_equals_the_constructor_restatement_everywhere():
    n, refusals = 0, set()
    for f in _all_facts():
        want, got = _outcome(R.constructor_structure, f), _outcome(train.step_plan, f)
        if isinstance(want, tuple):
            assert got == want, f
            refusals.add(want)
        else:
            assert isinstance(got, train.StepPlan) and set(want) == set(got._fields), f
            for k in got._fields:
                assert getattr(got, k) == want[k] and type(getattr(got, k)) is type(want[k]), (k, f)
        n += 1
    assert n == 18432
    assert refusals == {(ValueError, R.REFUSE_CLIP), (ValueError, R.REFUSE_FLAT)}


def test_plan_invariants():
    for f in _all_facts():
        p = _outcome(train.step_plan, f)
        if not isinstance(p, train.StepPlan):
            continue
        if p.flagged:
            assert p.collective == "overlap" and p.graph and p.two_graphs and p.grad_group, f
        assert p.collective == "none" or p.flat, f
        assert p.sinks or not p.sink_listener, f
        assert p.hooks or not p.comm_stream, f
        assert p.flat or not p.fused, f


@pytest.mark.parametrize("kw,plan", [r[1:] for r in R.PINS], ids=[r[0] for r in R.PINS])
def test_pinned_structure(kw, plan):
    assert train.step_plan(train.step_facts_of_values(**kw)) == plan


def test_every_structure_is_pinned():
    assert {p.collective for *_, p in R.PINS} == {"none", "host", "between", "overlap"}
    assert {p.flagged for *_, p in R.PINS} == {True, False}
    assert {p.two_graphs for *_, p in R.PINS} == {True, False} == {p.graph for *_, p in R.PINS}
    assert {p.fused for *_, p in R.PINS} == {True, False}


def test_facts_read_the_environment_when_built(monkeypatch):
    ps = [torch.nn.Parameter(torch.zeros(3))]
    for var in ("SAE_FLAGGED", "SAE_WG_STREAM"):
        monkeypatch.delenv(var, raising=False)
    f = train.step_facts(ps, True, None, True, None, None, False)
    assert f == train.step_facts_of_values(on_gpu=False, cuda=torch.cuda.is_available())
    monkeypatch.setenv("SAE_FLAGGED", "0")
    monkeypatch.setenv("SAE_WG_STREAM", "1")
    f = train.step_facts(ps, True, None, True, None, None, False)
    assert (f.flagged_on, f.wgrad_stream) == (False, True)
    assert not train.step_facts(ps, True, None, True, None, False, False).wgrad_stream   # the argument wins
    assert not train.step_facts([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))], True, None, True, None,
                                None, False).fp32_contiguous


class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.l1 = torch.nn.Linear(12, 16)
        self.l2 = torch.nn.Linear(16, 5)

    def forward(self, x, is_training: bool):
        return self.l2(torch.nn.functional.gelu(self.l1(x.flatten(1))))


@pytest.mark.parametrize("flat_grads", [None, True])
def test_cpu_step_shows_what_its_plan_names(flat_grads):
    step = train.TrainStep(TinyNet(), global_batch=8, flat_grads=flat_grads)
    want = train.step_plan(train.step_facts_of_values(on_gpu=False, cuda=torch.cuda.is_available(), graph=False,
                                                      flat_grads=flat_grads))
    assert step.plan == want and not want.fused and want.collective == "none" and not want.graph
    assert (step.graph, step.flat, step.collective, step.two_graphs, step._flagged) == (
        False, bool(flat_grads), "none", False, False)
    assert step.pg is False and step.world == 1
    assert step.reducer is None and step._flag_pg is None and step._wg is None
    assert isinstance(step.opt, torch.optim.AdamW)
    if flat_grads:
        assert isinstance(step._sinks, GradSinks) and step._sinks.listener is None
        lo, hi = step._flat.data_ptr(), step._flat.data_ptr() + 4 * step._flat.numel()
        assert all(p.grad is not None and lo <= p.grad.data_ptr() < hi and p.grad.data_ptr() % 16 == 0
                   for p in step._params)
    else:
        assert step._sinks is None and not hasattr(step, "_flat") and all(p.grad is None for p in step._params)
    g = torch.Generator().manual_seed(1)
    loss = step(torch.randn(8, 3, 4, generator=g), torch.randint(0, 5, (8,), generator=g))
    assert torch.isfinite(loss)
    step.close()


@pytest.mark.parametrize("kw,msg", [(dict(pg=True, backend="nccl", world=2, flat_grads=False), R.REFUSE_FLAT),
                                    (dict(world=2, flat_grads=False, clip_or_schedule=True), R.REFUSE_CLIP)])
def test_a_refused_configuration_raises_before_the_parameter_broadcast(monkeypatch, kw, msg):
    calls = []
    monkeypatch.setattr(train, "step_facts", lambda *a: train.step_facts_of_values(**kw))
    monkeypatch.setattr(train.TrainStep, "_broadcast_from_rank0", staticmethod(calls.append))
    with pytest.raises(ValueError) as e:
        train.TrainStep(TinyNet(), global_batch=8)
    assert str(e.value) == msg and calls == []
