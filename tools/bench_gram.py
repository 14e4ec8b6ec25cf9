"""Weighted Gram kernel (csrc/linear_gram.hip) against the path it replaces
in LinearRegression.fit: cat([x, ones]), x * w and two rocBLAS GEMMs in f32.

Same process, arms alternating after a warm-up, every call timed with device
events.  One JSON line per shape: median and min..max ms of the Gram step and
of the whole normal-equation fit (Gram + f64 solve), peak allocated bytes of
each fit above its starting level, bytes/s as N*F*4 / median and flop/s as
N*D^2 / median (the upper triangle, D = F + 2) for the kernel, and the max
relative difference of the two Gram matrices.

Usage: python tools/bench_gram.py [reps]
"""

import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(10_000_000, 256), (10_000_000, 64), (2_000_000, 16),
          (5_000_000, 1022)]
DEV = "cuda:0"


def gram_old(x, y, w):
    xa = torch.cat([x, torch.ones(x.shape[0], 1, device=x.device)], dim=1)
    xw = xa * w.unsqueeze(1)
    return xw.T @ xa, xw.T @ y


def gram_new(x, y, w):
    from spark_ensemble_amd.ops import dispatch

    g = dispatch.weighted_gram(x, y, w, native_only=True)
    f = x.shape[1]
    return g[:f + 1, :f + 1], g[:f + 1, f + 1]


def fit(gram_fn, x, y, w):
    gram, rhs = gram_fn(x, y, w)
    reg = torch.eye(gram.shape[0], dtype=torch.float64, device=x.device) * 1e-8
    return torch.linalg.solve(gram.double() + reg, rhs.double()).float()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return a.elapsed_time(b), peak


def main(reps):
    assert torch.cuda.is_available(), "bench_gram needs a GPU"
    for n, f in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(1)
        x = torch.randn(n, f, generator=g, device=DEV)
        y = torch.randn(n, generator=g, device=DEV)
        w = torch.rand(n, generator=g, device=DEV)
        arms = {"gram_old": lambda: gram_old(x, y, w),
                "gram_new": lambda: gram_new(x, y, w),
                "fit_old": lambda: fit(gram_old, x, y, w),
                "fit_new": lambda: fit(gram_new, x, y, w)}
        go, gn = gram_old(x, y, w)[0].double(), gram_new(x, y, w)[0]  # warm-up
        diff = float((go - gn).abs().max() / gn.abs().max())
        del go, gn
        for fn in arms.values():
            fn()
        times = {k: [] for k in arms}
        peaks = {k: 0 for k in arms}
        for _ in range(reps):
            for name, fn in arms.items():
                ms, peak = timed(fn)
                times[name].append(ms)
                peaks[name] = max(peaks[name], peak)
        row = {"n": n, "F": f, "x_bytes": n * f * 4, "max_rel_old_vs_new": diff}
        for name, ts in times.items():
            ts.sort()
            row[name] = {"ms": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3),
                         "max": round(ts[-1], 3), "peak_bytes": peaks[name]}
        med = row["gram_new"]["ms"] * 1e-3
        row["gram_new"]["tb_per_s"] = round(n * f * 4 / med / 1e12, 3)
        row["gram_new"]["tflop_per_s"] = round(n * (f + 2) ** 2 / med / 1e12, 2)
        print(json.dumps(row), flush=True)
        del x, y, w


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 7)
