"""GPU tests of the weighted Gram kernel (csrc/linear_gram.hip) through
dispatch.weighted_gram and LinearRegression.fit.

The oracle is reference.weighted_gram on float64 inputs on the CPU.  The
bound is 16x the error of the same function on the float32 inputs: the
kernel's summation order differs from torch's, its number format does not.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SINGLE = "largest single-panel F"
MULTI = "first multi-panel F"
ROUND = "one row tile past a full grid-stride round"
FLUSH = "one row past the f32 flush interval"
# every worker of a full grid one tile past its interval: the size at which
# a flush into the f64 slot happens in the middle of a launch
FLUSHED = "one row tile past a flush interval per worker"

CASES = [
    (7, 1),        # fewer rows than a k-step's tile; D = 3
    (333, 14),     # D = 16, exactly one column tile, ragged rows
    (333, 15),     # the y column alone in a second tile
    (257, 100),    # F % 4 != 0: unaligned rows, scalar loads
    (1000, SINGLE),
    (1000, MULTI),
    (300, 1022),   # D = 1024, the maximum
    (ROUND, 14),
    (FLUSH, 14),
    (FLUSHED, 14),
]


def _inputs(n, f, signed=False):
    from spark_ensemble_amd.ops import dispatch

    geo = dispatch._load_hip().linear_gram_geometry(14)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    f = {SINGLE: geo[5], MULTI: geo[5] + 1}.get(f, f)
    n = {ROUND: cus * geo[2] + 1, FLUSH: geo[4] + 1,
         FLUSHED: cus * geo[4] + 1}.get(n, n)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(n, f, generator=g)
    y = torch.randn(n, generator=g)
    w = torch.rand(n, generator=g)
    w[torch.rand(n, generator=g) < 0.1] = 0.0
    return x, y, (w - 0.5 if signed else w)


def _check(n, f, signed=False):
    from spark_ensemble_amd.ops import dispatch, reference

    x, y, w = _inputs(n, f, signed)
    f = x.shape[1]
    got = dispatch.weighted_gram(x.to(DEV), y.to(DEV), w.to(DEV), native_only=True)
    assert got is not None
    got = got.cpu()
    assert got.dtype == torch.float64 and torch.isfinite(got).all()
    want = reference.weighted_gram(x.double(), y.double(), w.double())
    ref32 = reference.weighted_gram(x, y, w).double()
    scale = want.abs().max()
    err = float((got - want).abs().max() / scale)
    err32 = float((ref32 - want).abs().max() / scale)
    sum_w = float((got[f, f] - w.double().sum()).abs() / scale)
    print(f"linear_gram {x.shape[0]}x{f} signed={signed}: {err:.2e} "
          f"(f32 torch {err32:.2e}), sum w {sum_w:.2e}, "
          f"{dispatch.last_weighted_gram_info}")
    assert torch.equal(got, got.T)
    assert err <= 16 * err32
    assert sum_w <= 16 * err32


@pytest.mark.parametrize("n,f", CASES)
def test_gram_against_float64(n, f):
    _check(n, f)


def test_negative_weights():
    _check(333, 100, signed=True)


@pytest.mark.parametrize("f", [100, MULTI])
def test_reproducible(f):
    from spark_ensemble_amd.ops import dispatch

    args = [t.to(DEV) for t in _inputs(1000, f)]
    a = dispatch.weighted_gram(*args, native_only=True)
    b = dispatch.weighted_gram(*args, native_only=True)
    assert torch.equal(a, b)


def test_declined_shape_falls_back():
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.ops import dispatch

    x, y, w = (t.to(DEV) for t in _inputs(2000, 1023))
    assert dispatch.weighted_gram(x, y, w, native_only=True) is None
    model = sea.LinearRegression().fit(TensorFrame(features=x, label=y))
    assert dispatch.last_weighted_gram_info["path"] == "reference"
    assert torch.isfinite(model.coefficients).all()


@pytest.mark.parametrize("intercept", [True, False])
def test_fit_against_float64_solve(intercept):
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.ops import dispatch
    from spark_ensemble_amd.utils.io import synthetic_regression

    df = synthetic_regression(6000, 16, seed=3)
    w = torch.rand(6000, generator=torch.Generator().manual_seed(5)) + 0.5
    df = df.withColumn("weight", w)
    xa = df["features"].double()
    if intercept:
        xa = torch.cat([xa, torch.ones(6000, 1, dtype=torch.float64)], dim=1)
    xw = xa * w.double().unsqueeze(1)
    want = torch.linalg.solve(xw.T @ xa, xw.T @ df["label"].double())
    err = []
    for frame in (df.to(DEV), df):
        m = (sea.LinearRegression().setWeightCol("weight")
             .setFitIntercept(intercept).fit(frame))
        beta = m.coefficients.cpu().double()
        if intercept:
            beta = torch.cat([beta, torch.tensor([m.intercept], dtype=torch.float64)])
        err.append(float((beta - want).abs().max()))
    print(f"linear_gram fit intercept={intercept}: gpu {err[0]:.2e}, cpu {err[1]:.2e}")
    # the CPU fit builds its normal equations without the dispatcher
    assert dispatch.last_weighted_gram_info["path"] == "native"
    assert err[0] <= 16 * err[1]


def test_fit_runs_native_with_small_peak_memory():
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.ops import dispatch
    from spark_ensemble_amd.utils.io import synthetic_regression

    df = synthetic_regression(200_000, 64, seed=3, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    sea.LinearRegression().fit(df)
    rise = torch.cuda.max_memory_allocated() - before
    print(f"linear_gram fit 200k x 64: peak +{rise} bytes, X {200_000 * 64 * 4}")
    assert dispatch.last_weighted_gram_info["path"] == "native"
    assert rise < 200_000 * 64 * 4 / 2
