"""Time of the out-of-bag pass over a packed forest on one GPU.

The forest is --trees complete depth --depth trees with thresholds drawn
from the distribution of the rows (standard normal), the rows come from a
seed, and the in-bag mask has the density of a Poisson(1) bootstrap
(P(in bag) = 1 - 1/e).  For every leaf width in --dims it prints one JSON
line with, per version, the median / min / max seconds over --reps rounds:

  op          ops.forest_oob as the estimators call it (rank transform of
              the rows, mask packing and the gfx950 kernel)
  kernel_*    the kernel alone on prepared inputs, per walk mode, with the
              achieved bytes/s from x bytes + mask bytes + output bytes
  reference   reference.forest_oob on the GPU (one torch walk per tree)
  predict     a full ops.forest_predict of the same rows

Every timing is device-synchronised and warmed once, and the versions
alternate inside each round of one process.  A GPU is required: there is no
CPU fallback for timings.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def complete_tree(depth, F, D, gen, dev):
    import torch

    n = 2 ** (depth + 1) - 1
    k = (n - 1) // 2
    feature = torch.full((n,), -1, dtype=torch.int32)
    feature[:k] = torch.randint(0, F, (k,), generator=gen).int()
    thr = torch.zeros(n)
    thr[:k] = torch.randn(k, generator=gen)
    left = torch.full((n,), -1, dtype=torch.int32)
    left[:k] = 2 * torch.arange(k, dtype=torch.int32) + 1
    leaf = torch.randn(n, D, generator=gen)
    leaf[:k] = 0.0
    tree = {"feature": feature, "threshold": thr, "left_child": left,
            "leaf_value": leaf}
    return {key: v.to(dev) for key, v in tree.items()}


def bench_dim(a, D, dev):
    import torch

    from spark_ensemble_amd.ops import dispatch, reference

    m = dispatch._load_hip()
    gen = torch.Generator().manual_seed(a.seed + D)
    trees = [complete_tree(a.depth, a.features, D, gen, dev)
             for _ in range(a.trees)]
    g = torch.Generator(device=dev).manual_seed(a.seed)
    x = torch.randn(a.rows, a.features, generator=g, device=dev)
    p_in = 1.0 - math.exp(-1.0)
    inbag = torch.stack(
        [torch.rand(a.rows, generator=g, device=dev) < p_in
         for _ in range(a.trees)], dim=1)

    cache, pcache = {}, {}
    versions = {}
    versions["op"] = lambda: dispatch.forest_oob(x, trees, inbag, cache=cache)
    versions["op"]()
    info = dict(dispatch.last_forest_oob_info)
    assert info["path"] == "native", info
    pack = cache["pack"]

    # the kernel alone, on prepared inputs, in every walk mode the pack has
    mask = dispatch._pack_inbag(inbag)
    sums = torch.empty(a.rows, D, dtype=torch.float32, device=dev)
    counts = torch.empty(a.rows, dtype=torch.int32, device=dev)
    out_bytes = sums.numel() * 4 + counts.numel() * 4
    kernel_bytes = {}

    def kernel(xin, nodes):
        return lambda: m.forest_oob(
            sums, counts, xin, nodes, pack["leaves"], pack["offsets32"],
            pack["groups_t"], mask, D, int(pack["max_nodes"]))

    versions["kernel_raw"] = kernel(x, pack["node64"])
    kernel_bytes["kernel_raw"] = x.numel() * 4 + mask.numel() * 4 + out_bytes
    if pack.get("binned_ok") and pack["bin_fmax"] <= a.features:
        xb = torch.empty(x.shape, dtype=torch.uint8, device=dev)
        m.bin_features(xb, x, dispatch._binned_edges(pack, a.features))
        versions["kernel_binned"] = kernel(xb, pack["node64b"])
        kernel_bytes["kernel_binned"] = (
            xb.numel() + mask.numel() * 4 + out_bytes)
    versions["reference"] = lambda: reference.forest_oob(x, trees, inbag)
    versions["predict"] = lambda: dispatch.forest_predict(
        x, trees, None, cache=pcache)

    times = {k: [] for k in versions}
    for k, fn in versions.items():  # warm: packs, mode probe, code load
        fn()
        torch.cuda.synchronize()
    for r in range(a.reps):
        for k, fn in versions.items():
            if k == "reference" and r >= a.ref_reps:
                continue
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)

    rec = {"dim": D, "rows": a.rows, "features": a.features,
           "trees": a.trees, "depth": a.depth, "op_mode": info["mode"],
           "groups": info["groups"], "rows_per_lane": info["rows_per_lane"],
           "oob_pairs": int((~inbag).sum())}
    for k, ts in times.items():
        ts = sorted(ts)
        rec[k] = {"median_s": round(ts[len(ts) // 2], 6),
                  "min_s": round(ts[0], 6), "max_s": round(ts[-1], 6),
                  "n": len(ts)}
        if k in kernel_bytes:
            rec[k]["bytes"] = kernel_bytes[k]
            rec[k]["GBps"] = round(
                kernel_bytes[k] / ts[len(ts) // 2] / 1e9, 1)
    print(json.dumps(rec), flush=True)


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--trees", type=int, default=50)
    p.add_argument("--depth", type=int, default=8)
    p.add_argument("--features", type=int, default=64)
    p.add_argument("--rows", type=int, default=4_000_000)
    p.add_argument("--dims", type=int, nargs="+", default=[1, 3])
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--ref-reps", type=int, default=2)
    p.add_argument("--seed", type=int, default=0)
    a = p.parse_args()

    import torch

    if not torch.cuda.is_available():
        print("bench_oob needs a GPU", file=sys.stderr)
        return 2
    for D in a.dims:
        bench_dim(a, D, torch.device("cuda", 0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
