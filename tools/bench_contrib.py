"""Throughput of per-row feature contributions on one GPU.

Fits a binary GBMClassifier (default 100 trees of depth 8 on F=256 synthetic
features) and prints one JSON line per step:

  fit        the fit itself (on --fit-rows rows) and the forest's path count
  contrib    rows/s of predictContrib (the gfx950 kernel) on --rows rows
  reference  rows/s of the torch reference op on the GPU, same model and the
             first --ref-rows of the same rows
  predict    rows/s of predictRaw on the same rows

Every step is a fresh child process under its own time limit
(--step-timeout seconds); the fitted model travels between them through a
temporary directory.  A step that fails or runs out of time ends the run.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("fit", "contrib", "reference", "predict")


def _rows(n, f, seed, dev):
    import torch

    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, f, generator=g, device=dev)


def _timed(fn, reps):
    import torch

    fn()  # warm: packs the forest, loads the kernels
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return sorted(ts)[len(ts) // 2], ts


def run_step(a):
    import torch

    import spark_ensemble_amd as sea
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.models import DecisionTreeRegressor
    from spark_ensemble_amd.ops import dispatch, reference

    dev = "cuda:0"
    path = os.path.join(a.workdir, "model")
    if a.step == "fit":
        x = _rows(a.fit_rows, a.features, 1, dev)
        # every 8th feature carries signal; deep trees still split on noise
        logit = x[:, ::8].sum(dim=1) + (x[:, 0] * x[:, 8])
        y = (logit + torch.randn_like(logit) > 0).float()
        est = (
            sea.GBMClassifier()
            .setLoss("bernoulli")
            .setBaseLearner(DecisionTreeRegressor().setMaxDepth(a.depth))
            .setNumBaseLearners(a.trees)
        )
        t0 = time.perf_counter()
        model = est.fit(TensorFrame(features=x, label=y))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        model.save(path, overwrite=True)
        leaves = sum(int((m._tree["feature"] < 0).sum())
                     for ms in model._models for m in ms)
        print(json.dumps({"step": "fit", "seconds": round(dt, 3),
                          "trees": model.numModels, "paths": leaves,
                          "fit_rows": a.fit_rows, "features": a.features}),
              flush=True)
        return
    model = sea.GBMClassificationModel.load(path)
    if a.step == "reference":
        x = _rows(a.rows, a.features, 2, dev)[: a.ref_rows].contiguous()
        trees, weights = [], []
        for ms, ws in zip(model._models, model._weights):
            trees.append(ms[0]._tree)
            weights.append(ws[0])
        tables = reference.contrib_paths(trees, weights, None, 1)
        med, ts = _timed(lambda: reference.forest_contrib(
            x, trees, weights, None, 1, tables=tables), 1)
        n = a.ref_rows
    else:
        x = _rows(a.rows, a.features, 2, dev)
        n = a.rows
        if a.step == "contrib":
            med, ts = _timed(lambda: model.predictContrib(x), a.reps)
            assert dispatch.last_forest_contrib_info["path"] == "native"
        else:
            med, ts = _timed(lambda: model.predictRaw(x), a.reps)
    print(json.dumps({
        "step": a.step, "rows": n, "rows_per_s": round(n / med, 1),
        "median_s": round(med, 5), "all_s": [round(t, 5) for t in ts],
    }), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--trees", type=int, default=100)
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--features", type=int, default=256)
    p.add_argument("--rows", type=int, default=1_000_000)
    p.add_argument("--fit-rows", type=int, default=200_000)
    p.add_argument("--ref-rows", type=int, default=1024)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--step-timeout", type=float, default=240.0)
    p.add_argument("--step", choices=STEPS, help=argparse.SUPPRESS)
    p.add_argument("--workdir", help=argparse.SUPPRESS)
    a = p.parse_args()
    if a.step:
        run_step(a)
        return 0
    with tempfile.TemporaryDirectory(prefix="bench_contrib_") as wd:
        for step in STEPS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", step,
                   "--workdir", wd]
            for k in ("trees", "depth", "features", "rows", "fit_rows",
                      "ref_rows", "reps"):
                cmd += ["--" + k.replace("_", "-"), str(getattr(a, k))]
            try:
                rc = subprocess.run(cmd, timeout=a.step_timeout).returncode
            except subprocess.TimeoutExpired:
                print(json.dumps({"step": step, "error": "time limit"}),
                      flush=True)
                return 1
            if rc != 0:
                print(json.dumps({"step": step, "error": f"exit {rc}"}),
                      flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
