"""bench.py's command line without a GPU: a plain run leaves the extra measurements to --full, --steps is checked, and --dump-outputs
writes float32 / float64 arrays within its 64 MB budget, the same rows on every run."""
import sys

import numpy as np
import pytest

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_leaves_the_extras_to_full(monkeypatch):
    assert not _parse(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2").extras
    assert _parse(monkeypatch, "--full").extras
    assert not _parse(monkeypatch, "--full", "--no-extras").extras
    a = _parse(monkeypatch, "--steps", "7", "--dump-outputs", "out")
    assert a.steps == 7 and a.dump_outputs == "out"


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--steps", "0")


def test_dump_outputs_dtypes(tmp_path):
    bench.dump_outputs(str(tmp_path / "d"), {"poses": np.arange(6, dtype=np.float64).reshape(2, 3),
                                             "points": np.ones((10, 4), np.float32), "ids": np.arange(5, dtype=np.int32)})
    got = {p.stem: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert sorted(got) == ["ids", "points", "poses"]
    assert got["poses"].dtype == np.float64 and np.array_equal(got["poses"], np.arange(6.0).reshape(2, 3))
    assert got["points"].dtype == np.float32 and got["points"].shape == (10, 4)
    assert got["ids"].dtype == np.float32 and np.array_equal(got["ids"], np.arange(5))


def test_dump_outputs_samples_large_arrays_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 << 20)
    rng = np.random.default_rng(5)
    big = rng.standard_normal((400_000, 4)).astype(np.float32)  # 6.4 MB
    big[:, 0] = np.arange(big.shape[0])  # a row number in column 0
    small = rng.standard_normal((6, 3))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a_big, b_big = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    total = sum(p.stat().st_size for p in (tmp_path / "a").iterdir())
    assert total <= (3 << 20) + 1024  # + the two .npy headers
    assert 0 < a_big.shape[0] < big.shape[0] and a_big.shape[1] == 4
    assert np.array_equal(a_big, b_big)  # the same rows on every run
    # every sampled row is a row of the original, in the original order
    idx = a_big[:, 0].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(big[idx], a_big)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)  # small arrays are kept whole
