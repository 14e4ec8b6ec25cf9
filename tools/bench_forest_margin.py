"""Seconds per ``predictRaw`` of a multiclass GBM on one GPU: the one-launch
forest_margin route against the per-class forest_predict route.

The model is built by hand, not fitted: --stages x --classes complete depth
--depth regression trees whose thresholds come from a table of 255 cut points
per feature (what trees trained on 256 bins share, so the union pack keeps
its u8 rank form), random leaves, weights 0.1, a constant init.  The rows
come from a seed.  It prints JSON lines with the median / min / max seconds
over --reps rounds:

  predict_raw   GBMClassificationModel.predictRaw, warm, packs cached:
                "fused" (one forest_margin launch) and "old"
                (SEA_MARGIN_FUSED=0: a forest_predict call per class),
                alternating inside each round; the results are compared
                bit for bit before anything is timed
  row_form      ops.forest_margin under SEA_MARGIN_MODE=raw and =binned
  stores        ops.forest_margin over the SAME trees cut into 2 planes and
                into --classes planes: same node hops, 13x the plane flushes

--root names the tree to import the package from (default: this one).  A
tree without ops.forest_margin (an earlier commit) times "old" alone.
Every timing is device-synchronised.  A GPU is required: there is no CPU
fallback for timings.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_model(a, dev):
    import torch

    from spark_ensemble_amd.classification.gbm import GBMClassificationModel
    from spark_ensemble_amd.models.dummy import DummyClassificationModel
    from spark_ensemble_amd.models.tree import DecisionTreeRegressionModel

    gen = torch.Generator().manual_seed(a.seed)
    F, K = a.features, a.classes
    cuts = torch.randn(F, 255, generator=gen).sort(dim=1).values
    n = 2 ** (a.depth + 1) - 1
    k = (n - 1) // 2
    left = torch.full((n,), -1, dtype=torch.int32)
    left[:k] = 2 * torch.arange(k, dtype=torch.int32) + 1

    def tree():
        feature = torch.full((n,), -1, dtype=torch.int32)
        feature[:k] = torch.randint(0, F, (k,), generator=gen).int()
        thr = torch.zeros(n)
        thr[:k] = cuts[feature[:k].long(),
                       torch.randint(0, 255, (k,), generator=gen)]
        leaf = torch.randn(n, 1, generator=gen)
        leaf[:k] = 0.0
        m = DecisionTreeRegressionModel()
        m._set_tree({"feature": feature.to(dev), "threshold": thr.to(dev),
                     "left_child": left.to(dev), "leaf_value": leaf.to(dev)},
                    F)
        return m

    model = GBMClassificationModel()
    model._init = DummyClassificationModel.from_raw(torch.zeros(K), K, F)
    model._models = [[tree() for _ in range(K)] for _ in range(a.stages)]
    model._weights = [[0.1] * K for _ in range(a.stages)]
    model._subspaces = [torch.arange(F) for _ in range(a.stages)]
    model._num_classes, model._dim, model._num_features = K, K, F
    model.set("loss", "logloss")
    return model


def timed(fn, env):
    import torch

    for k, v in env.items():
        os.environ[k] = v
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    finally:
        for k in env:
            del os.environ[k]


def race(name, versions, envs, reps, extra):
    """Warm every version once (packs, code load, the old route's probe),
    compare the results, then time them alternating inside each round."""
    import torch

    outs = {v: timed(fn, envs[v])[1] for v, fn in versions.items()}
    first = next(iter(outs.values()))
    rec = dict(extra, case=name, bitwise_equal=all(
        torch.equal(o, first) for o in outs.values()))
    del outs, first
    times = {v: [] for v in versions}
    for _ in range(reps):
        for v, fn in versions.items():
            times[v].append(timed(fn, envs[v])[0])
    for v, ts in times.items():
        ts = sorted(ts)
        rec[v] = {"median_s": round(ts[len(ts) // 2], 6),
                  "min_s": round(ts[0], 6), "max_s": round(ts[-1], 6),
                  "n": len(ts)}
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--root", default=ROOT)
    p.add_argument("--classes", type=int, default=26)
    p.add_argument("--stages", type=int, default=100)
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--features", type=int, default=256)
    p.add_argument("--rows", type=int, default=2_000_000)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))

    import torch

    if not torch.cuda.is_available():
        print("bench_forest_margin needs a GPU", file=sys.stderr)
        return 2
    from spark_ensemble_amd.ops import dispatch

    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(a.seed)
    x = torch.randn(a.rows, a.features, generator=g, device=dev)
    model = build_model(a, dev)
    shape = {"rows": a.rows, "features": a.features, "classes": a.classes,
             "stages": a.stages, "depth": a.depth}

    fused = hasattr(dispatch, "forest_margin")
    versions = {"old": lambda: model.predictRaw(x)}
    # "1" lifts the model's feature-count rule: the kernel is timed at any F
    envs = {"old": {"SEA_MARGIN_FUSED": "0"}, "fused": {"SEA_MARGIN_FUSED": "1"}}
    if fused:
        versions = {"fused": lambda: model.predictRaw(x), **versions}
    race("predict_raw", versions, envs, a.reps, shape)
    if not fused:
        return 0

    K = a.classes
    trees = [m._tree for ms in model._models for m in ms]
    w = [0.1] * len(trees)
    planes = [t % K for t in range(len(trees))]
    caches = {"raw": {}, "binned": {}, "planes_2": {}, f"planes_{K}": {}}

    def op(key, pl, P):
        return lambda: dispatch.forest_margin(x, trees, w, pl, P,
                                              cache=caches[key])

    race("row_form", {"raw": op("raw", planes, K),
                      "binned": op("binned", planes, K)},
         {"raw": {"SEA_MARGIN_MODE": "raw"},
          "binned": {"SEA_MARGIN_MODE": "binned"}}, a.reps, shape)
    # the same trees dealt to two planes: the results differ by construction
    # (bitwise_equal is false), only the times are of interest
    two =[t % 2 for t in range(len(trees))]
    race("stores", {"planes_2": op("planes_2", two, 2),
                    f"planes_{K}": op(f"planes_{K}", planes, K)},
         {"planes_2": {}, f"planes_{K}": {}}, a.reps, shape)
    return 0


if __name__ == "__main__":
    sys.exit(main())
