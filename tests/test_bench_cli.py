"""bench.py command line: a plain run prints the headline result line only,
`--full` adds the Rank-1 validation, `--dump-outputs DIR` writes the last
timed round's outputs — the same arrays from run to run on the same
arguments.  Exercised on the CPU path at a tiny size."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = ["--cpu", "--gpus", "1", "--steps", "2", "--warmup", "1",
        "--model", "resnet18", "--img", "32x16", "--batch", "8", "--ids", "4",
        "--imgs-per-id", "2", "--num-classes", "64", "--lambda-k", "8"]


def _bench(cwd, *extra):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), *TINY, *extra],
        capture_output=True, text=True, timeout=300, cwd=str(cwd))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


def _load_dir(path):
    return {f: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


@pytest.mark.timeout(600)
def test_plain_and_dump_outputs(tmp_path):
    a, b, cwd = tmp_path / "a", tmp_path / "b", tmp_path / "cwd"
    cwd.mkdir()
    result = _bench(cwd, "--dump-outputs", str(a))
    _bench(cwd, "--dump-outputs", str(b))
    # the current directory need not be writable: nothing is left in it
    assert os.listdir(cwd) == []

    # a plain run: headline fields, the steps it was asked for, no Rank-1
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in result
    assert result["steps"] == 2 and result["warmup"] == 1
    assert result["ms_per_step"] > 0
    assert result["value"] == pytest.approx(
        4 * 2 / (result["ms_per_step"] / 1000.0), rel=0.02)
    assert "rank1" not in result

    first, second = _load_dir(a), _load_dir(b)
    assert first and set(first) == set(second)
    assert all(f.endswith(".npy") for f in first)
    assert any(f.startswith("upload.client-0.incremental_sw.") for f in first)
    assert "train.client-0.task-0-0.tr_loss.npy" in first
    total = 0
    for name, arr in first.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert np.isfinite(arr).all(), name
        # same arguments -> same inputs; the CPU path is deterministic, so
        # the outputs match bit for bit
        np.testing.assert_array_equal(arr, second[name], err_msg=name)
        total += arr.nbytes
    assert total <= 64 * 2 ** 20


@pytest.mark.timeout(600)
def test_full_reports_rank1(tmp_path):
    result = _bench(tmp_path, "--full")
    assert 0.0 <= result["rank1"] <= 1.0


@pytest.fixture()
def bench_module(monkeypatch, tmp_path):
    """bench.py imported in-process; the benchmark-mode environment defaults
    it sets on import are undone afterwards so later tests do not see them.
    With MIOPEN_USER_DB_PATH set the import copies no find-db files."""
    import importlib

    saved = dict(os.environ)
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(tmp_path))
    monkeypatch.syspath_prepend(REPO)
    try:
        yield importlib.import_module("bench")
    finally:
        os.environ.clear()
        os.environ.update(saved)
        sys.modules.pop("bench", None)


def test_dump_outputs_samples_large_arrays(tmp_path, monkeypatch, bench_module):
    """An array above its share of the budget is cut to a fixed seeded sample
    of its flattened elements; small ones are written whole."""
    import torch

    bench = bench_module
    monkeypatch.setattr(bench, "DUMP_BUDGET_ELEMS", 300)

    class _Server:
        clients = {"client-0": {
            "train_cnt": 7, "task_token": None,
            "incremental_sw": {"w": torch.arange(1000.).reshape(10, 100),
                               "b": torch.arange(6, dtype=torch.bfloat16)}}}

    class _Log:
        records = {"data": {"client-0": {"3": {"t": {"tr_loss": 1.5,
                                                     "tr_acc": 0.25}}}}}

    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), _Server(), ["client-0"], _Log(), 3)
    got, again = _load_dir(tmp_path / "a"), _load_dir(tmp_path / "b")
    assert set(got) == {"upload.client-0.train_cnt.npy",
                        "upload.client-0.incremental_sw.w.npy",
                        "upload.client-0.incremental_sw.b.npy",
                        "train.client-0.t.tr_loss.npy",
                        "train.client-0.t.tr_acc.npy"}
    w = got["upload.client-0.incremental_sw.w.npy"]
    assert w.shape == (60,) and w.dtype == np.float32     # 300 // 5 arrays
    assert len(set(w.tolist())) == 60 and (np.diff(w) > 0).all()
    np.testing.assert_array_equal(w, again["upload.client-0.incremental_sw.w.npy"])
    b = got["upload.client-0.incremental_sw.b.npy"]
    assert b.dtype == np.float32 and b.tolist() == [0, 1, 2, 3, 4, 5]
    assert got["upload.client-0.train_cnt.npy"] == 7.0
    assert got["train.client-0.t.tr_loss.npy"] == 1.5
