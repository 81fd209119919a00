"""CPU: bench.py's command line (a plain run against --full), --dump-outputs' files, and the MIOpen
find-db working copy that keeps the tracked tools/miopen_db files unmodified."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert _parse(monkeypatch, "--full").full
    assert _parse(monkeypatch, "--kernel-only").full   # only --full fields are left to measure
    assert _parse(monkeypatch, "--dump-outputs", "somewhere").dump_outputs == "somewhere"


@pytest.mark.parametrize("argv", [("--steps", "0"), ("--warmup", "-1"), ("--kernel-only", "--dump-outputs", "d")])
def test_arguments_that_cannot_be_timed_are_refused(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_headline_fields(monkeypatch):
    a = _parse(monkeypatch, "--steps", "5", "--warmup", "1")
    out = bench.headline(a, 1, 4, 3, 192, 512, 640, 660.0, 6.06)
    assert out["value"] == 660.0 and out["ms_per_step"] == 6.06 and out["steps"] == 5 and out["warmup"] == 1
    assert out["unit"] == "depth maps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["metric"].startswith("depth maps/sec") and out["full"] is False
    assert out["config"]["feature_hw"] == [128, 160]


def test_dump_outputs_writes_float32_arrays(tmp_path):
    g = torch.Generator().manual_seed(0)
    initial = torch.rand(2, 1, 5, 7, generator=g, dtype=torch.float64)
    refined = torch.rand(2, 1, 5, 7, generator=g)
    bench.dump_outputs(str(tmp_path / "sub" / "dir"), (initial, refined))
    got = {n: np.load(str(tmp_path / "sub" / "dir" / n)) for n in sorted(os.listdir(str(tmp_path / "sub" / "dir")))}
    assert sorted(got) == ["initial_depth.npy", "refined_depth.npy"]
    assert all(v.dtype == np.float32 and v.shape == (2, 1, 5, 7) for v in got.values())
    assert np.array_equal(got["initial_depth.npy"], initial.to(torch.float32).numpy())
    assert np.array_equal(got["refined_depth.npy"], refined.numpy())


def test_miopen_reads_a_working_copy_of_the_shipped_find_db(tmp_path, monkeypatch):
    import miopen_db
    monkeypatch.delenv("MIOPEN_USER_DB_PATH", raising=False)
    monkeypatch.setattr(miopen_db.tempfile, "tempdir", str(tmp_path))
    work = miopen_db.use()
    assert work == os.environ["MIOPEN_USER_DB_PATH"] and os.path.dirname(work) == str(tmp_path)
    shipped = sorted(n for n in os.listdir(miopen_db.SHIPPED) if not n.startswith("."))
    assert shipped and sorted(os.listdir(work)) == shipped
    for n in shipped:
        assert open(os.path.join(miopen_db.SHIPPED, n), "rb").read() == open(os.path.join(work, n), "rb").read()
    # the path in the environment (this process's copy, a parent's, or the caller's own) wins
    assert miopen_db.use() == work
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", "elsewhere")
    assert miopen_db.use() == "elsewhere"
    miopen_db._remove(work, os.getpid() + 1)   # a forked child leaves the parent's copy alone
    assert os.path.isdir(work)
    miopen_db._remove(work, os.getpid())
    assert not os.path.exists(work)
