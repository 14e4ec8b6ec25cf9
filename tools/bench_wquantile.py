"""Time of median-voting BoostingRegressionModel.predict on one GPU.

For every member count in --members the model is --members complete depth
--depth regression trees over --features columns with thresholds drawn from
the distribution of the rows (standard normal), random leaves and stage
weights drawn like log(1 / beta) of a boosting run (one of them negative).
It prints one JSON line with, per version, the median / min / max seconds
over --reps rounds and the peak extra device memory of one call:

  fused    model.predict as it stands: one forest_wquantile launch (rank
           transform of the rows, the gfx950 kernel)
  stacked  the route it replaces: one predict per member, torch.stack, and
           ensemble.utils.weighted_median over [N, M]

and the share of rows on which the two disagree (the stacked route decides
"cumulative weight >= half" with an f32 cumsum).  Every timing is
device-synchronised and warmed once, and the versions alternate inside each
round of one process.  A GPU is required: there is no CPU fallback for
timings.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_oob import complete_tree  # noqa: E402


def bench_members(a, M, x, dev):
    import torch

    from spark_ensemble_amd.ensemble.utils import weighted_median
    from spark_ensemble_amd.models.tree import DecisionTreeRegressionModel
    from spark_ensemble_amd.ops import dispatch
    from spark_ensemble_amd.regression.boosting import BoostingRegressionModel

    gen = torch.Generator().manual_seed(a.seed + M)
    model = BoostingRegressionModel()
    model._models = []
    for _ in range(M):
        t = DecisionTreeRegressionModel()
        t._set_tree(complete_tree(a.depth, a.features, 1, gen, dev),
                    a.features)
        model._models.append(t)
    wts = (torch.rand(M, generator=gen) * 3.0 + 0.05).tolist()
    wts[-1] = -0.01  # the stage that tripped est_err >= 0.5
    model._weights = wts
    model._num_features = a.features
    model.set("votingStrategy", "median")

    def fused():
        return model.predict(x)

    def stacked():
        preds = torch.stack([m.predict(x) for m in model._models], dim=1)
        w = torch.tensor(wts, dtype=torch.float32, device=dev)
        return weighted_median(preds, w.unsqueeze(0).expand_as(preds))

    versions = {"fused": fused, "stacked": stacked}
    results, peak = {}, {}
    for k, fn in versions.items():  # warm: packs, code load; peak memory
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        results[k] = fn()
        torch.cuda.synchronize()
        peak[k] = torch.cuda.max_memory_allocated() - before
    info = dict(dispatch.last_forest_wquantile_info)
    assert info["path"] == "native", info
    times = {k: [] for k in versions}
    for _ in range(a.reps):
        for k, fn in versions.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)

    differ = float((results["fused"] != results["stacked"]).float().mean())
    rec = {"members": M, "rows": a.rows, "features": a.features,
           "depth": a.depth, "mode": info["mode"],
           "rows_per_block": info["rows_per_block"],
           "groups": info["groups"], "rows_that_differ": differ}
    for k, ts in times.items():
        ts = sorted(ts)
        rec[k] = {"median_s": round(ts[len(ts) // 2], 6),
                  "min_s": round(ts[0], 6), "max_s": round(ts[-1], 6),
                  "n": len(ts), "peak_extra_bytes": int(peak[k])}
    rec["speedup"] = round(
        rec["stacked"]["median_s"] / rec["fused"]["median_s"], 2)
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--members", type=int, nargs="+", default=[10, 50, 200])
    p.add_argument("--depth", type=int, default=6)
    p.add_argument("--features", type=int, default=64)
    p.add_argument("--rows", type=int, default=2_000_000)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_wquantile needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(a.seed)
    x = torch.randn(a.rows, a.features, generator=g, device=dev)
    for M in a.members:
        bench_members(a, M, x, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
