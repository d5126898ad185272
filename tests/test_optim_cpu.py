"""CPU tests of the reference's optimizer chain around AdamW (global-norm clip, warm-up-cosine
schedule): the float64 helper the GPU tests compare against (tests/_optim_ref.py) on hand-computed
values, the new C ABI entry points (declared, exported, refusing bad arguments on the host) and
the torch-op form TrainStep runs when the optimizer is torch.optim.AdamW."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["sae_adamw_prepare_workspace_bytes", "sae_adamw_prepare", "sae_adamw_step_dev"]


def test_reference_schedule_values():
    """0 at count 0, peak at warmup_steps, end from decay_steps on; the midpoints by hand."""
    a = (0.0, 3e-3, 3, 10, 1e-5)
    assert R.warmup_cosine(0, *a) == 0.0
    assert R.warmup_cosine(3, *a) == 3e-3
    for c in (10, 11, 1000):
        assert R.warmup_cosine(c, *a) == pytest.approx(1e-5, rel=1e-12)
    assert R.warmup_cosine(1, *a) == pytest.approx(1e-3, rel=1e-12)
    assert R.warmup_cosine(2, 1e-3, 3e-3, 4, 8, 0.0) == pytest.approx(2e-3, rel=1e-12)   # init > 0
    # halfway down the cosine (c = D / 2: cos = 0): the mean of peak and end
    assert R.warmup_cosine(6, 0.0, 3e-3, 2, 10, 1e-5) == pytest.approx(0.5 * (3e-3 + 1e-5), rel=1e-12)
    # a quarter of the way: cos(pi / 4)
    want = 3e-3 * ((1 - 1e-5 / 3e-3) * 0.5 * (1 + math.sqrt(0.5)) + 1e-5 / 3e-3)
    assert R.warmup_cosine(4, 0.0, 3e-3, 2, 10, 1e-5) == pytest.approx(want, rel=1e-12)
    assert R.warmup_cosine(0, 0.0, 3e-3, 0, 10, 1e-5) == 3e-3                             # no warm-up


def test_reference_clip_values():
    g = [np.array([3.0, 0.0], np.float32), np.array([[4.0]], np.float32)]
    assert R.global_norm(g) == 5.0
    assert R.clip_scale(5.0, 6.0) == 1.0            # below max_norm: untouched
    assert R.clip_scale(5.0, 5.0) == 1.0            # at max_norm: max / norm, which is exactly 1
    assert R.clip_scale(5.0, 2.0) == 0.4
    assert R.global_norm([np.zeros(7, np.float32)]) == 0.0 and R.clip_scale(0.0, 1.0) == 1.0


def test_package_schedule_matches_reference_helper():
    from sae_vision_amd import train
    s = train.WarmupCosine(0.0, 3e-3, 3, 10, 1e-5)
    for c in range(14):
        assert s.value(c) == pytest.approx(R.warmup_cosine(c, 0.0, 3e-3, 3, 10, 1e-5), rel=1e-14, abs=0)
    ref = train.reference_schedule(5e-4, 1024, 1251)
    assert (ref.init_value, ref.peak_value, ref.warmup_steps, ref.decay_steps, ref.end_value) == \
        (0.0, 1e-3, 5 * 1251, 30 * 1251, 1e-5)
    for bad in ((0.0, 0.0, 1, 2, 0.0), (0.0, 1e-3, -1, 2, 0.0), (0.0, 1e-3, 2, 2, 0.0), (0.0, math.nan, 1, 2, 0.0)):
        with pytest.raises(ValueError):
            train.WarmupCosine(*bad)


def test_header_declares_and_library_exports():
    import sae_vision_amd
    from sae_vision_amd import _lib as L
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sae_attn.h")).read(), flags=re.S)
    lib = sae_vision_amd.load_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert re.search(r" T %s\b" % name, nm), name
        assert hasattr(lib, name) and name in L.EXPORTED_SYMBOLS
    assert "sae_lr_schedule" in src
    for macro, val in (("SAE_ADAMW_NORM_SPAN", L.SAE_ADAMW_NORM_SPAN), ("SAE_ADAMW_PREPARE_PASS", L.SAE_ADAMW_PREPARE_PASS),
                       ("SAE_LR_CONSTANT", L.SAE_LR_CONSTANT), ("SAE_LR_WARMUP_COSINE", L.SAE_LR_WARMUP_COSINE)):
        assert re.search(r"#define %s %d\b" % (macro, val), src), macro
    assert ctypes.sizeof(L.LrSchedule) == 24
    span = L.SAE_ADAMW_NORM_SPAN
    ws = lib.sae_adamw_prepare_workspace_bytes
    assert [ws(n) for n in (-1, 0, 1, span, span + 1, 10 * span)] == [0, 0, 8, 8, 16, 80]


def _prepare(lib, L, n=64, g=16, max_norm=1.0, sched="default", step=16, ws=16, hyper=16):
    if sched == "default":
        sched = L.LrSchedule(L.SAE_LR_WARMUP_COSINE, 0.0, 1e-3, 1e-5, 2, 10)
    return lib.sae_adamw_prepare(None, n, g, max_norm, None if sched is None else ctypes.byref(sched), step, ws, hyper)


@pytest.mark.parametrize("kw,msg", [
    (dict(sched=None), "NULL"),
    (dict(step=None), "NULL"),
    (dict(hyper=None), "NULL"),
    (dict(g=None), "norm pass"),
    (dict(ws=None), "norm pass"),
    (dict(n=0), "norm pass"),
    (dict(n=-5), "norm pass"),
    (dict(max_norm=0.0), "max_norm"),
    (dict(max_norm=-1.0), "max_norm"),
    (dict(max_norm=math.nan), "max_norm"),
    (dict(sched=(1, 0.0, 1e-3, 1e-5, -1, 10)), "warmup_steps"),
    (dict(sched=(1, 0.0, 1e-3, 1e-5, 10, 10)), "decay_steps"),
    (dict(sched=(1, 0.0, 1e-3, 1e-5, 10, 4)), "decay_steps"),
    (dict(sched=(1, 0.0, 0.0, 1e-5, 2, 10)), "peak"),
    (dict(sched=(1, 0.0, -1e-3, 1e-5, 2, 10)), "peak"),
    (dict(sched=(0, 0.0, 0.0, 0.0, 0, 0)), "peak"),
    (dict(sched=(1, 0.0, math.nan, 1e-5, 2, 10)), "peak"),
    (dict(sched=(7, 0.0, 1e-3, 1e-5, 2, 10)), "kind"),
])
def test_prepare_refusals(kw, msg):
    """Every refusal happens on the host (no GPU here): SAE_EINVAL and a message naming the argument."""
    from sae_vision_amd import _lib as L
    lib = L.load()
    if isinstance(kw.get("sched"), tuple):
        kw = dict(kw, sched=L.LrSchedule(*kw["sched"]))
    assert _prepare(lib, L, **kw) == L.SAE_EINVAL
    assert msg in lib.sae_last_error().decode(), lib.sae_last_error()


def test_step_dev_refusals():
    from sae_vision_amd import _lib as L
    lib = L.load()
    ok = dict(n_chunks=1, chunks=16, n_tiles=0, tiles=None, step=16, hyper=16)
    for bad in (dict(chunks=None), dict(step=None), dict(hyper=None), dict(n_chunks=-1), dict(n_tiles=2),
                dict(n_tiles=-1)):
        a = dict(ok, **bad)
        rc = lib.sae_adamw_step_dev(None, a["n_chunks"], a["chunks"], a["n_tiles"], a["tiles"], a["step"], a["hyper"],
                                    0.9, 0.999, 1e-8, 1e-4)
        assert rc == L.SAE_EINVAL and "adamw_step_dev" in lib.sae_last_error().decode(), bad
    # nothing to update: accepted without a launch
    assert lib.sae_adamw_step_dev(None, 0, None, 0, None, 16, 16, 0.9, 0.999, 1e-8, 1e-4) == L.SAE_OK


def test_torch_optimizer_step_applies_clip_and_schedule():
    """TrainStep with torch.optim.AdamW (CPU, fp32), 4 steps, a clip that triggers and a 2-step
    warm-up: parameters equal to a loop written here -- the helper's clip factor on the gradients,
    the helper's schedule value as the rate, torch.optim.AdamW -- within the tolerance of the CPU
    step tests (tests/test_dp_gloo.py)."""
    from sae_vision_amd import train
    from test_dp_gloo import TinyNet, _data
    x, y = _data()
    clip, sched = 0.05, (0.0, 2e-3, 2, 6, 1e-5)
    step = train.TrainStep(TinyNet(), global_batch=x.shape[0], clip_grad=clip, lr_schedule=train.WarmupCosine(*sched))
    assert not isinstance(step.opt, train.FusedAdamW) and step.lr_now is None
    ref = TinyNet()
    opt = torch.optim.AdamW(ref.parameters(), lr=1.0, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    clipped = []
    for k in range(4):
        step(x, y)
        opt.zero_grad()
        torch.nn.functional.cross_entropy(ref(x, True).float(), y, label_smoothing=0.1).backward()
        norm = R.global_norm([p.grad.numpy() for p in ref.parameters()])
        scale = R.clip_scale(norm, clip)
        clipped.append(bool(norm > clip))
        for p in ref.parameters():
            p.grad.mul_(float(scale))
        lr = float(R.warmup_cosine(k, *sched))
        for gr in opt.param_groups:
            gr["lr"] = lr
        opt.step()
        assert step.lr_now == pytest.approx(lr, rel=1e-12, abs=0)
        assert float(step.grad_norm) == pytest.approx(norm, rel=1e-5)
    assert any(clipped), "the clip never triggered: the case checks nothing"
    for (n, a), b in zip(step.model.named_parameters(), ref.parameters()):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-6, msg=n)
    # and the arguments are not ignored: the plain step ends elsewhere
    plain = train.TrainStep(TinyNet(), global_batch=x.shape[0])
    for _ in range(4):
        plain(x, y)
    assert any(not torch.allclose(a, b, rtol=1e-3, atol=1e-5)
               for a, b in zip(plain.model.parameters(), step.model.parameters()))


def test_bad_arguments_are_refused():
    from sae_vision_amd import train
    from test_dp_gloo import TinyNet
    for clip in (0.0, -1.0, math.nan):
        with pytest.raises(ValueError, match="clip_grad"):
            train.TrainStep(TinyNet(), global_batch=8, clip_grad=clip)
    with pytest.raises(TypeError, match="WarmupCosine"):
        train.TrainStep(TinyNet(), global_batch=8, lr_schedule=lambda c: 1e-3)
