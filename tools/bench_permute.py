"""Time of permutation loss sums over a packed forest on one GPU.

The forest is --trees complete depth --depth trees over --features columns
with thresholds drawn from the distribution of the rows (standard normal);
rows, labels and donors come from a seed.  For every walk mode in --modes
(SEA_PERMUTE_MODE / SEA_SERVE_MODE) it prints one JSON line with, per
version, the median / min / max seconds over --reps rounds and the
rows * features * repeats per second at the median:

  fused   ops.forest_permute_loss as the models call it (rank transform of
          the rows, donor upload, the gfx950 kernel and its reduce)
  loop    the column-swap loop it replaces: features * repeats times a
          column overwrite, ops.forest_predict of all rows and a squared
          loss sum, on the same frame with the same donors

and the largest relative difference between the two results.  A forest
with more than 255 thresholds on one feature (a narrow frame under many
trees) has no u8 rank form: the binned line then says so.  Every timing
is device-synchronised and warmed once, and the versions alternate inside
each round of one process.  A GPU is required: there is no CPU fallback for
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


def bench_mode(a, mode, dev):
    import torch

    from spark_ensemble_amd.boosting.losses import SquaredLoss
    from spark_ensemble_amd.inspection import draw_donors
    from spark_ensemble_amd.ops import dispatch

    os.environ["SEA_PERMUTE_MODE"] = mode
    os.environ["SEA_SERVE_MODE"] = mode
    gen = torch.Generator().manual_seed(a.seed)
    trees = [complete_tree(a.depth, a.features, 1, gen, dev)
             for _ in range(a.trees)]
    weights = [0.1] * a.trees
    g = torch.Generator(device=dev).manual_seed(a.seed)
    x = torch.randn(a.rows, a.features, generator=g, device=dev)
    label = torch.randn(a.rows, generator=g, device=dev)
    init = torch.zeros(a.rows, device=dev)
    w = torch.ones(a.rows, device=dev)
    donor = draw_donors(a.rows, a.repeats, a.seed).to(dev, torch.int32)
    loss = SquaredLoss()
    wt = torch.tensor(weights)
    cache, pcache = {}, {}

    def fused():
        return dispatch.forest_permute_loss(
            x, trees, weights, init, label, w, loss, donor, cache=cache)

    def loop():
        def loss_sum(xx):
            p = dispatch.forest_predict(xx, trees, wt, cache=pcache)[:, 0]
            return (0.5 * (label - p) ** 2).double().sum()

        base = loss_sum(x)
        perm = torch.empty(a.repeats, a.features, dtype=torch.float64,
                           device=dev)
        xp = x.clone()
        for r in range(a.repeats):
            dr = donor[r].long()
            for f in range(a.features):
                xp[:, f] = x[dr, f]
                perm[r, f] = loss_sum(xp)
                xp[:, f] = x[:, f]
        return base, perm

    versions = {"fused": fused, "loop": loop}
    results = {}
    try:
        for k, fn in versions.items():  # warm: packs, code load
            results[k] = fn()
            torch.cuda.synchronize()
    except ValueError as e:
        if mode != "binned" or "no u8 rank form" not in str(e):
            raise
        # more than 255 thresholds on one feature: only f32 rows apply
        print(json.dumps({"mode": mode, "rows": a.rows,
                          "features": a.features, "unavailable": str(e)}),
              flush=True)
        return
    info = dict(dispatch.last_forest_permute_info)
    assert info["path"] == "native", info
    assert info["mode"] == mode, info
    times = {k: [] for k in versions}
    for r in range(a.reps):
        for k, fn in versions.items():
            if k == "loop" and r >= a.loop_reps:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)

    fb, fp = results["fused"]
    lb, lp = results["loop"]
    rel = float(((fp - lp).abs() / lp.abs().clamp_min(1e-30)).max())
    rel = max(rel, abs(float(fb) - float(lb)) / max(abs(float(lb)), 1e-30))
    work = a.rows * a.features * a.repeats
    geo = dispatch.forest_permute_geometry()
    rec = {"mode": mode, "rows": a.rows, "features": a.features,
           "repeats": a.repeats, "trees": a.trees, "depth": a.depth,
           "threads": geo[0], "feature_chunk": info["feature_chunk"],
           "groups": info["groups"], "max_rel_diff": rel}
    for k, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        rec[k] = {"median_s": round(med, 6), "min_s": round(ts[0], 6),
                  "max_s": round(ts[-1], 6), "n": len(ts),
                  "row_feature_repeats_per_s": round(work / med, 1)}
    rec["speedup"] = round(
        rec["loop"]["median_s"] / rec["fused"]["median_s"], 2)
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--trees", type=int, default=100)
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--features", type=int, default=256)
    p.add_argument("--rows", type=int, default=262_144)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--modes", nargs="+", default=["binned", "raw"],
                   choices=["binned", "raw"])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--loop-reps", type=int, default=2)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_permute needs a GPU", file=sys.stderr)
        return 2
    for mode in a.modes:
        bench_mode(a, mode, torch.device("cuda", 0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
