"""Wide-multiclass (K = 26) gini-tree micro-benchmarks on one GPU.

No arguments; seeded; reads only data/letter and synthetic data.  Prints one
JSON line per measurement (times in milliseconds, every repetition listed
so the spread is visible):

  (a) hist      label-indexed hist_build_class (transposed and row-major
                bins source) vs the chunked generic hist_build, N=2M, F=64,
                B=256, K=26, at the root and at a 256-node level
  (b) split     wide split_argmax kernel vs the eager torch chain, n=256,
                F=64, B=256, C=28
  (c) fit       DecisionTreeClassifier depth 8 and an 8-member
                BaggingClassifier on the synthetic set and on letter

The old and new implementations of (a)/(b) alternate inside each timing
loop.  The script also runs on a checkout that predates the class-mode ops:
it then reports only the old halves of (a)/(b), and (c) times whatever path
that checkout's estimators take — run both checkouts alternately to compare
fits.
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import spark_ensemble_amd as sea  # noqa: E402
from spark_ensemble_amd.frame import TensorFrame  # noqa: E402
from spark_ensemble_amd.models import DecisionTreeClassifier  # noqa: E402
from spark_ensemble_amd.ops import dispatch, reference  # noqa: E402
from spark_ensemble_amd.utils.io import (  # noqa: E402
    load_libsvm, synthetic_classification,
)

DEV = "cuda:0"
HAS_CLASS = hasattr(dispatch, "hist_build_class")
TREE = "class-mode" if HAS_CLASS else "before"


def timed_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def alternate(impls, reps, warm=2):
    """impls: {name: fn}; warm each, then time them round-robin."""
    for fn in impls.values():
        for _ in range(warm):
            fn()
    times = {k: [] for k in impls}
    for _ in range(reps):
        for name, fn in impls.items():
            times[name].append(timed_ms(fn)[1])
    return times


def report(bench, times, **extra):
    for impl, ts in times.items():
        s = sorted(ts)
        print(json.dumps({
            "bench": bench, "impl": impl, "checkout": TREE,
            "median_ms": round(s[len(s) // 2], 3),
            "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3),
            "all_ms": [round(t, 3) for t in ts], **extra,
        }), flush=True)


def bench_hist():
    n, f, b, k, nn = 2_000_000, 64, 256, 26, 2
    g = torch.Generator(device=DEV).manual_seed(1)
    bins = torch.randint(0, b, (n, f), generator=g, device=DEV,
                         dtype=torch.uint8)
    label = torch.randint(0, k, (n,), generator=g, device=DEV).to(torch.uint8)
    w = torch.poisson(torch.ones(n, 1, device=DEV), generator=g)
    w_max = float(w.max())
    onehot = torch.zeros(n, k, device=DEV)
    onehot.scatter_(1, label.long().unsqueeze(1), 1.0)
    gh = torch.cat([onehot * w, w, torch.ones(n, 1, device=DEV)], 1)
    gh = gh.contiguous()
    del onehot
    gh_max = torch.tensor([w_max] * (k + 1) + [1.0])
    # level shapes: the root, and 256 nodes whose rows are ascending inside
    # each node (what the stable partition leaves behind)
    node_of = torch.randint(0, 256, (n,), generator=g, device=DEV)
    order = torch.argsort(node_of, stable=True).to(torch.int32)
    counts = torch.bincount(node_of, minlength=256).cpu()
    levels = {
        "root": (torch.arange(n, dtype=torch.int32, device=DEV),
                 torch.tensor([0, n], dtype=torch.int64)),
        "256-node level": (order, torch.cat(
            [torch.zeros(1, dtype=torch.int64), counts.cumsum(0)])),
    }
    for name, (rows, offs) in levels.items():
        n_nodes = offs.numel() - 1
        col0 = torch.zeros(n_nodes, dtype=torch.int32)
        impls = {
            "hist_build chunked": lambda: dispatch.hist_build(
                bins, gh, rows, offs, b, k, gh_max),
        }
        if HAS_CLASS:
            impls["hist_build_class transposed"] = (
                lambda: dispatch.hist_build_class(
                    bins, label, w, rows, offs, col0, b, k, nn, w_max,
                    transposed=True))
            impls["hist_build_class row-major"] = (
                lambda: dispatch.hist_build_class(
                    bins, label, w, rows, offs, col0, b, k, nn, w_max,
                    transposed=False))
            old = impls["hist_build chunked"]()
            for key in list(impls)[1:]:
                diff = float((impls[key]() - old).abs().max())
                print(json.dumps({"bench": f"hist {name}", "impl": key,
                                  "max_abs_diff_vs_chunked": diff}))
            del old
        report(f"hist {name}", alternate(impls, reps=10),
               shape=dict(N=n, F=f, B=b, K=k, nodes=n_nodes))


def bench_split():
    n, f, b, c, d = 256, 64, 256, 28, 26
    g = torch.Generator(device=DEV).manual_seed(2)
    # a histogram-like tensor: integer class counts, hess = their sum
    cls = torch.randint(0, 6, (n, f, b, d), generator=g, device=DEV).float()
    # every feature of a node must carry the same totals: permute bins of
    # feature 0 per feature instead of drawing independent counts
    base = cls[:, 0]
    for j in range(1, f):
        cls[:, j] = base[:, torch.randperm(b, generator=g, device=DEV)]
    hess = cls.sum(-1, keepdim=True)
    hist = torch.cat([cls, hess, hess], dim=-1).contiguous()
    del cls, hess, base
    args = (1e-6, 0.0, 1.0, 0.0)
    impls = {"eager chain": lambda: reference.split_search(
        hist, *args, d_dims=d)}
    if HAS_CLASS:
        impls["split_argmax wide"] = lambda: dispatch.split_search(
            hist, *args, d_dims=d)
        a = impls["eager chain"]()[0]
        k = impls["split_argmax wide"]()[0]
        print(json.dumps({"bench": "split", "max_rel_gain_diff": float(
            ((a - k).abs() / a.abs().clamp_min(1e-6)).max())}))
    report("split", alternate(impls, reps=10),
           shape=dict(n=n, F=f, B=b, C=c))


def _letter():
    df = load_libsvm(os.path.join(ROOT, "data", "letter", "letter.svm"))
    return TensorFrame({
        "features": df["features"].to(DEV),
        "label": (df["label"] - 1.0).to(DEV),
    })


def bench_fits():
    sets = {
        "synthetic 2M x 64, K=26, 256 bins": (
            synthetic_classification(2_000_000, 64, k=26, seed=5, device=DEV),
            256, 3),
        "letter 15k x 16, K=26, 32 bins": (_letter(), 32, 5),
    }
    for name, (df, max_bins, reps) in sets.items():
        tree = DecisionTreeClassifier().setMaxDepth(8).setMaxBins(max_bins)
        bag = (sea.BaggingClassifier()
               .setBaseLearner(
                   DecisionTreeClassifier().setMaxDepth(8)
                   .setMaxBins(max_bins))
               .setNumBaseLearners(8).setSubspaceRatio(0.8)
               .setReplacement(True).setSeed(9))
        impls = {
            "DecisionTreeClassifier depth 8": lambda: tree.fit(df),
            "BaggingClassifier 8 x depth 8": lambda: bag.fit(df),
        }
        report(f"fit {name}", alternate(impls, reps=reps, warm=1))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    assert dispatch.hip_available(), "HIP extension must be built"
    torch.manual_seed(0)
    bench_hist()
    torch.cuda.empty_cache()
    bench_split()
    torch.cuda.empty_cache()
    bench_fits()
