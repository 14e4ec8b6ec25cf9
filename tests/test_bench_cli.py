"""bench.py command line: a plain run does only the headline measurement,
``--full`` adds the secondary logloss fit, ``--dump-outputs`` writes the
timed fit's model as float .npy arrays that repeat run to run."""

import importlib.util
import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--cpu", "--rows", "3000", "--features", "8",
         "--max-depth", "3", "--steps", "3", "--warmup", "1"]


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location(
        "sea_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _run(bench, monkeypatch, capsys, extra):
    from spark_ensemble_amd.parallel import set_comm

    monkeypatch.setattr(sys, "argv", ["bench.py"] + SMALL + extra)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    try:
        bench.main()
    finally:
        set_comm(None)
    lines = [ln for ln in capsys.readouterr().out.splitlines()
             if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_lean_and_full_adds_logloss(bench, monkeypatch, capsys):
    out = _run(bench, monkeypatch, capsys, [])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in out
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(
        3000 / (out["ms_per_step"] / 1000.0), rel=1e-9)
    assert out["config"]["logloss_secondary"] is None

    full = _run(bench, monkeypatch, capsys, ["--full"])
    ll = full["config"]["logloss_secondary"]
    assert ll["loss"] == "logloss" and ll["rounds"] == 1 and ll["trees"] == 2
    assert ll["ms_per_round"] > 0


def test_dump_outputs_repeatable(bench, monkeypatch, capsys, tmp_path):
    dirs = [str(tmp_path / "a"), str(tmp_path / "b")]
    for d in dirs:
        out = _run(bench, monkeypatch, capsys, ["--dump-outputs", d])
        assert out["steps"] == 3
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"stage_weights.npy", "tree_offsets.npy", "tree_feature.npy",
            "tree_threshold.npy", "tree_left_child.npy",
            "tree_leaf_value.npy", "sample_rows.npy", "sample_raw.npy",
            "sample_probability.npy"} <= set(names)
    total = 0
    for name in names:
        a = np.load(os.path.join(dirs[0], name))
        b = np.load(os.path.join(dirs[1], name))
        assert a.dtype in (np.float32, np.float64), name
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 * 2**20
    # one tree per timed step (bernoulli, dim 1): --steps sets the work
    assert np.load(os.path.join(dirs[0], "stage_weights.npy")).shape == (3, 1)
    offs = np.load(os.path.join(dirs[0], "tree_offsets.npy"))
    assert offs.shape == (4,) and (np.diff(offs) > 0).all()
    assert offs[-1] == np.load(
        os.path.join(dirs[0], "tree_feature.npy")).shape[0]
    p = np.load(os.path.join(dirs[0], "sample_probability.npy"))
    assert p.shape == (3000, 2)
    assert np.allclose(p.sum(axis=1), 1.0, atol=1e-6)
