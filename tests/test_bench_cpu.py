"""bench.py's host-side pieces that need no GPU: the --dump-outputs writer and the argument surface."""
import types

import numpy as np
import pytest
import torch

import bench


def _fake_step(n_big, flat=True):
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(3, 5, generator=g), torch.randn(n_big, generator=g), torch.randn(7, generator=g)]
    step = types.SimpleNamespace(_params=params, flat=flat)
    if flat:
        step._flat = torch.randn(n_big + 24, generator=g)
    else:
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
    return step


def test_dump_outputs_small_arrays_are_written_whole(tmp_path):
    step = _fake_step(100)
    loss = torch.tensor(6.25)
    bench.dump_outputs(str(tmp_path), step, loss)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["grads.npy", "loss.npy", "params.npy"]
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("loss", "params", "grads")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got["loss"].tolist() == [6.25]
    np.testing.assert_array_equal(got["params"], torch.cat([p.reshape(-1) for p in step._params]).numpy())
    np.testing.assert_array_equal(got["grads"], step._flat.numpy())


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    step = _fake_step(5000, flat=False)
    bench.dump_outputs(str(tmp_path / "a"), step, torch.tensor(1.0))
    bench.dump_outputs(str(tmp_path / "b"), step, torch.tensor(1.0))
    full = torch.cat([p.reshape(-1) for p in step._params]).numpy()
    grads = torch.cat([p.grad.reshape(-1) for p in step._params]).numpy()
    idx = np.sort(np.random.default_rng(0).choice(full.size, 1000, replace=False))
    for name, ref in (("params", full), ("grads", grads)):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.shape == (1000,)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, ref[idx])


def test_dump_budget_is_under_64_mb():
    # loss + params + grads, each cut to DUMP_MAX_ELEMS float32 values
    assert 4 * (1 + 2 * bench.DUMP_MAX_ELEMS) <= 64 * 10 ** 6


def test_steps_must_be_positive(monkeypatch, capsys):
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as e:
        bench.main()
    assert e.value.code == 2
    assert "--steps" in capsys.readouterr().err
