"""Standalone hist_build microbench (GPU): times the kernel in isolation
across the configurations that matter for the flagship bench, so PMC runs
attribute counters to exactly this kernel.

Every row is the median (min - max) of ``--calls`` device-event timed calls
after one warm-up; a call is the whole op (upload of the chunk table, the
kernel, the staging pass of multi-chunk nodes).  ``--only A,B`` keeps the
rows whose label contains A or B; ``--skip-position`` leaves out the rows
that read gh by position (``gather_ranges_gh`` + ``gh_by_position``), so the
same script times a build from before they existed."""

import argparse
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from spark_ensemble_amd.ops import dispatch as ops  # noqa: E402

ARGS = None


def bench(label, bins, gh, rows, offs, B, by_position=False):
    if not wanted(label):
        return None
    if by_position and ARGS.skip_position:
        return None
    C = gh.shape[1]
    # per-channel maxima precomputed ONCE, as the tree grower does per fit
    # (leaving it to the dispatch default re-runs a strided 10M-row amax
    # per call and used to inflate the C=3 numbers ~2.4x)
    max_abs = gh.abs().amax(dim=0).cpu()
    d = max(1, C - 2)
    n_nodes = offs.numel() - 1
    if by_position:
        # what grow_forest does below the root: the compact matrix comes
        # from the pass that collects the rows (not timed here, see the
        # "gather" rows), the kernel streams it
        lens = offs[1:] - offs[:-1]
        col0 = torch.zeros(n_nodes, dtype=torch.int64)
        rows, gh = ops.gather_ranges_gh(rows, gh, offs[:-1], lens, col0, C)
        zero = torch.zeros(n_nodes, dtype=torch.int32)
        run = lambda: ops.hist_build_forest(  # noqa: E731
            bins, gh, rows, offs, zero, B, C, max_abs, d, gh_by_position=True)
    else:
        run = lambda: ops.hist_build(bins, gh, rows, offs, B, d, max_abs)  # noqa: E731
    return timed(label, run, rows.numel() * bins.shape[1])


def wanted(label):
    return not ARGS.only or any(s in label for s in ARGS.only.split(","))


def timed(label, run, bin_bytes):
    out = run()  # warmup
    torch.cuda.synchronize()
    ms = []
    for _ in range(ARGS.calls):
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        e0.record()
        out = run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    med = ms[len(ms) // 2]
    print(f"{label:50s} {med:8.3f} ms  ({ms[0]:.3f} - {ms[-1]:.3f})  "
          f"{bin_bytes / 1e6 / max(med, 1e-9):7.1f} GB/s bin-bytes", flush=True)
    return out


def main():
    global ARGS
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--only", default="")
    ap.add_argument("--skip-position", action="store_true")
    ARGS = ap.parse_args()

    dev = "cuda:0"
    N, F = 10_000_000, 256
    g = torch.Generator(device=dev).manual_seed(1)
    bins = torch.randint(0, 256, (N, F), generator=g, dtype=torch.uint8, device=dev)
    gh3 = torch.rand(N, 3, generator=g, device=dev)
    rows = torch.arange(N, dtype=torch.int32, device=dev)
    offs1 = torch.tensor([0, N])

    gh2 = gh3[:, :2].contiguous()
    bench("root B=256 C=3 contiguous", bins, gh3, rows, offs1, 256)
    bench("root B=256 C=2 contiguous", bins, gh2, rows, offs1, 256)
    bench("root B=64  C=3 contiguous", (bins & 63), gh3, rows, offs1, 64)

    # shuffled rows (deep-level access pattern)
    perm = torch.randperm(N, generator=g, device=dev).to(torch.int32)
    bench("root B=256 C=2 shuffled", bins, gh2, perm, offs1, 256)
    bench("root B=256 C=3 shuffled", bins, gh3, perm, offs1, 256)

    # 64-node level, half the rows
    n_nodes = 64
    seg = N // 2 // n_nodes
    offs = torch.tensor([i * seg for i in range(n_nodes + 1)])
    rows_half = perm[: seg * n_nodes]
    bench("64 nodes B=256 C=2 shuffled half-rows", bins, gh2, rows_half, offs, 256)
    bench("64 nodes B=256 C=3 shuffled half-rows", bins, gh3, rows_half, offs, 256)
    bench("64 nodes B=256 C=2 shuffled half-rows, gh by position",
          bins, gh2, rows_half, offs, 256, by_position=True)
    bench("64 nodes B=256 C=3 shuffled half-rows, gh by position",
          bins, gh3, rows_half, offs, 256, by_position=True)

    # zero-row nodes at the flagship geometry: 4 feature groups per node, so
    # 256 and 512 blocks that only clear the LDS and flush — the fixed cost
    # of a wave of blocks
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    for n_empty in (64, 128):
        bench(f"{n_empty} zero-row nodes B=256 C=2 (flush only)", bins, gh2,
              empty, torch.zeros(n_empty + 1, dtype=torch.int64), 256)
    bench("128 zero-row nodes B=256 C=3 (flush only)", bins, gh3, empty,
          torch.zeros(129, dtype=torch.int64), 256)

    # one multi-chunk node of half the rows, ascending: the staged flush
    half = torch.nonzero(
        torch.rand(N, generator=g, device=dev) < 0.5).flatten()[: N // 2]
    half = half.to(torch.int32)
    offs_h = torch.tensor([0, half.numel()])
    bench("one 5M-row node B=256 C=2 ascending", bins, gh2, half, offs_h, 256)
    bench("one 5M-row node B=256 C=2 ascending, gh by position",
          bins, gh2, half, offs_h, 256, by_position=True)

    # deepest level of a depth-8 tree: 128 built nodes out of 256, about
    # 5.0M rows, ascending row ids inside each node as the stable partition
    # leaves them
    node = torch.randint(0, 256, (N,), generator=g, device=dev)
    built = torch.nonzero(node < 128).flatten()
    order = torch.sort(node[built], stable=True).indices
    rows_deep = built[order].to(torch.int32)
    cnt = torch.bincount(node[built], minlength=128).cpu()
    offs_d = torch.zeros(129, dtype=torch.int64)
    offs_d[1:] = torch.cumsum(cnt, 0)
    bench("128 nodes B=256 C=2 ascending 5.0M rows (deepest)", bins, gh2,
          rows_deep, offs_d, 256)
    bench("128 nodes B=256 C=2 ascending 5.0M rows (deepest), gh by position",
          bins, gh2, rows_deep, offs_d, 256, by_position=True)
    bench("128 nodes B=256 C=3 ascending 5.0M rows (deepest)", bins, gh3,
          rows_deep, offs_d, 256)
    bench("128 nodes B=256 C=3 ascending 5.0M rows (deepest), gh by position",
          bins, gh3, rows_deep, offs_d, 256, by_position=True)

    # the row-collecting pass alone, without and with the gradients
    if wanted("gather_ranges"):
        starts, lens = offs_d[:-1], offs_d[1:] - offs_d[:-1]
        timed("gather_ranges 128 ranges 5.0M rows",
              lambda: ops.gather_ranges(rows_deep, starts, lens), 0)
        if not ARGS.skip_position:
            col0 = torch.zeros(128, dtype=torch.int64)
            timed("gather_ranges_gh 128 ranges 5.0M rows C=2",
                  lambda: ops.gather_ranges_gh(rows_deep, gh2, starts, lens,
                                               col0, 2), 0)


if __name__ == "__main__":
    main()
