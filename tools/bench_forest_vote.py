"""Rows per second of wide-class forest voting on one GPU: the forest_vote
kernel route against the route it replaces.

The forest is --trees complete depth --depth voting trees of K classes with
thresholds drawn from the distribution of the rows (standard normal) and
random class-count leaves; the rows come from a seed; the in-bag mask has
the density of a Poisson(1) bootstrap (P(in bag) = 1 - 1/e).  For every K in
--classes, vote in {hard, soft} and mask in {no, yes} it prints one JSON line
with, per version, the median / min / max seconds over --reps rounds and the
rows per second at the median:

  native_raw     ops.forest_vote, f32 rows (SEA_VOTE_MODE=raw)
  native_binned  ops.forest_vote, u8 rank rows, rank transform included
  old            the same call under SEA_VOTE_WIDE=0: the v1 forest_predict
                 kernel, or with a mask the torch reference op on the GPU

Every call includes what an estimator pays: the rank transform and, with a
mask, the mask packing.  Every timing is device-synchronised and warmed
once, and the versions alternate inside each round of one process.  The
native result is compared with the old one before anything is timed.  A GPU
is required: there is no CPU fallback for timings.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def voting_tree(depth, F, K, soft, gen, dev):
    import torch

    n = 2 ** (depth + 1) - 1
    k = (n - 1) // 2
    feature = torch.full((n,), -1, dtype=torch.int32)
    feature[:k] = torch.randint(0, F, (k,), generator=gen).int()
    thr = torch.zeros(n)
    thr[:k] = torch.randn(k, generator=gen)
    left = torch.full((n,), -1, dtype=torch.int32)
    left[:k] = 2 * torch.arange(k, dtype=torch.int32) + 1
    cnt = torch.randint(0, 50, (n, K), generator=gen).float()
    if soft:
        leaf = cnt / cnt.sum(dim=1, keepdim=True).clamp_min(1e-12)
    else:
        leaf = torch.zeros_like(cnt)
        leaf.scatter_(1, cnt.argmax(dim=1, keepdim=True), 1.0)
    tree = {"feature": feature, "threshold": thr, "left_child": left,
            "leaf_value": leaf}
    return {key: v.to(dev) for key, v in tree.items()}


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


def bench_case(a, K, soft, masked, x, inbag, dev):
    import torch

    from spark_ensemble_amd.ops import dispatch

    gen = torch.Generator().manual_seed(a.seed + K)
    trees = [voting_tree(a.depth, a.features, K, soft, gen, dev)
             for _ in range(a.trees)]
    bag = inbag if masked else None
    caches = {"native_raw": {}, "native_binned": {}, "old": {}}
    envs = {"native_raw": {"SEA_VOTE_MODE": "raw"},
            "native_binned": {"SEA_VOTE_MODE": "binned"},
            "old": {"SEA_VOTE_WIDE": "0"}}

    def version(name):
        return lambda: dispatch.forest_vote(x, trees, soft, inbag=bag,
                                            cache=caches[name])

    outs, infos = {}, {}
    for name in envs:  # warm: packs, code load; and the results to compare
        _, out = timed(version(name), envs[name])
        outs[name] = out if bag is None else out[0]
        infos[name] = dict(dispatch.last_forest_vote_info)
    assert infos["native_raw"]["path"] == "native", infos
    assert infos["native_binned"]["mode"] == "binned", infos
    assert infos["old"]["path"] == "reference", infos
    same = all(torch.equal(outs[k], outs["old"]) for k in outs)

    times = {k: [] for k in envs}
    for r in range(a.reps):
        for name in envs:
            if name == "old" and masked and r >= a.ref_reps:
                continue
            times[name].append(timed(version(name), envs[name])[0])
    rec = {"classes": K, "vote": "soft" if soft else "hard", "mask": masked,
           "rows": a.rows, "features": a.features, "trees": a.trees,
           "depth": a.depth, "kp": infos["native_raw"]["kp"],
           "rows_per_lane": infos["native_raw"]["rows_per_lane"],
           "groups": infos["native_raw"]["groups"], "bitwise_equal": same}
    for name, ts in times.items():
        ts = sorted(ts)
        med = ts[len(ts) // 2]
        rec[name] = {"median_s": round(med, 6), "min_s": round(ts[0], 6),
                     "max_s": round(ts[-1], 6), "n": len(ts),
                     "Mrows_per_s": round(a.rows / med / 1e6, 1)}
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--trees", type=int, default=50)
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--features", type=int, default=64)
    p.add_argument("--rows", type=int, default=2_000_000)
    p.add_argument("--classes", type=int, nargs="+", default=[9, 16, 26, 32])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--ref-reps", type=int, default=2)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_forest_vote needs a GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(a.seed)
    x = torch.randn(a.rows, a.features, generator=g, device=dev)
    p_in = 1.0 - math.exp(-1.0)
    inbag = torch.stack(
        [torch.rand(a.rows, generator=g, device=dev) < p_in
         for _ in range(a.trees)], dim=1)
    for K in a.classes:
        for soft in (False, True):
            for masked in (False, True):
                bench_case(a, K, soft, masked, x, inbag, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
