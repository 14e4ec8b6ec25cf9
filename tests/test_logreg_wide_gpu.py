"""GPU tests of the MFMA logistic loss+gradient kernel (csrc/linear_wide.hip)
through dispatch.logreg_loss_grad and LogisticRegression.fit.

The reference is reference.logreg_loss_grad on float64 inputs on the CPU.
The bound is 16x the error of the same function on the float32 inputs: the
kernel's transcendental functions and its summation order differ from
torch's, its number format does not.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROUND = "one tile past a full grid-stride round"

CASES = [
    (333, 16, 26, True, 0.05),    # letter: S=1, many row groups, ragged tail
    (7, 16, 9, False, 0.05),      # fewer rows than one tile
    (257, 100, 9, False, 0.05),   # F not a multiple of 4 or 16
    (1000, 1024, 3, True, 0.05),  # narrow K on the wide path (F > 512)
    (1000, 515, 32, True, 0.05),  # KP=32 full, unaligned rows
    (70, 1024, 16, True, 0.05),   # KP=16 exactly
    (70, 1024, 17, True, 0.05),   # first K padded to 32
    (70, 1024, 32, True, 0.05),   # the largest W
    (ROUND, 16, 26, True, 0.05),  # second pass of the persistent loop
    (333, 16, 26, True, 5.0),     # margins of about +-80
]


def _inputs(n, f, k, bias, scale):
    from spark_ensemble_amd.ops import dispatch

    if n == ROUND:
        tile = dispatch._load_hip().logreg_wide_geometry(f, k)[2]
        n = torch.cuda.get_device_properties(0).multi_processor_count * tile + 1
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, f, generator=g)
    y = torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
    w = torch.rand(n, generator=g)
    wmat = torch.randn(f + (1 if bias else 0), k, generator=g) * scale
    return x, y, w, wmat


def _errors(got, want):
    loss = float((got[0].double() - want[0]).abs() / want[0].abs())
    grad = float((got[1:].double() - want[1:]).abs().max() / want[1:].abs().max())
    return loss, grad


@pytest.mark.parametrize("n,f,k,bias,scale", CASES)
def test_payload_against_float64(n, f, k, bias, scale):
    from spark_ensemble_amd.ops import dispatch, reference

    x, y, w, wmat = _inputs(n, f, k, bias, scale)
    got = dispatch.logreg_loss_grad(
        x.to(DEV), y.to(DEV), w.to(DEV), wmat.to(DEV), bias, native_only=True)
    assert got is not None
    got = got.cpu()
    assert torch.isfinite(got).all()
    want = reference.logreg_loss_grad(x.double(), y, w.double(), wmat.double(), bias)
    ref32 = reference.logreg_loss_grad(x, y, w, wmat, bias)
    loss, grad = _errors(got, want)
    loss32, grad32 = _errors(ref32, want)
    print(f"logreg_wide {x.shape[0]}x{f}x{k} scale {scale}: loss {loss:.2e} "
          f"(f32 torch {loss32:.2e}), grad {grad:.2e} (f32 torch {grad32:.2e})")
    assert loss <= 16 * loss32
    assert grad <= 16 * grad32


@pytest.mark.parametrize("n,f,k", [(1000, 515, 32), (ROUND, 16, 26)])
def test_reproducible(n, f, k):
    from spark_ensemble_amd.ops import dispatch

    args = [t.to(DEV) for t in _inputs(n, f, k, True, 0.05)]
    a = dispatch.logreg_loss_grad(*args, True, native_only=True)
    b = dispatch.logreg_loss_grad(*args, True, native_only=True)
    assert torch.equal(a, b)


def _fit_gap(k):
    """Relative gap of the float64 regularised objective between a GPU and a
    CPU fit of the same rows."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.ops import reference
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(6000, 16, k=k, seed=3)
    x = df["features"].double()
    y = df["label"].to(torch.int32)
    w = torch.ones(x.shape[0], dtype=torch.float64)
    obj = []
    for frame in (df.to(DEV), df):
        m = sea.LogisticRegression().setMaxIter(30).setRegParam(0.01).fit(frame)
        coef = m._coef.cpu().double()
        wmat = torch.cat([coef, m._intercept.cpu().double().reshape(1, -1)])
        loss = reference.logreg_loss_grad(x, y, w, wmat, True)[0] / x.shape[0]
        obj.append(float(loss + 0.005 * (coef * coef).sum()))
    return abs(obj[0] - obj[1]) / abs(obj[1])


def test_fit_reaches_cpu_objective():
    # k=3 runs the narrow kernel, as before this kernel existed: its gap is
    # the yardstick for the 26-class fit on the new one
    gap3, gap26 = _fit_gap(3), _fit_gap(26)
    print(f"logreg_wide fit gap: k=3 {gap3:.2e}, k=26 {gap26:.2e}")
    assert gap26 <= 4 * gap3
