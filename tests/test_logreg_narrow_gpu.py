"""GPU tests of the narrow logistic loss+gradient kernel (csrc/linear.hip)
through the raw ``logreg_loss_grad`` binding, which reaches the instantiations
dispatch sends to the MFMA kernel (F > 512), and of the choice dispatch makes
between the two kernels and the torch path.

Reference and bound are those of tests/logreg_util.py: float64 on the CPU,
one denominator per payload entry, 16x the error of the float32 reference.
"""

import pytest
import torch

import logreg_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

# the launch table of csrc/linear.hip: (NC, K) with NC * 4 * K <= 64
MAX_NC = {2: 8, 3: 5, 4: 4, 5: 3, 6: 2, 7: 2, 8: 2}
INSTANTIATIONS = [(nc, k) for k, top in MAX_NC.items()
                  for nc in range(1, top + 1)]


@pytest.fixture(scope="module")
def ext():
    from spark_ensemble_amd.ops import dispatch

    assert dispatch.hip_available(), "HIP extension must be built in-tree"
    return dispatch._load_hip()


def _run_narrow(ext, x, y, w, wmat, bias, x_dev=None):
    f, k = x.shape[1], wmat.shape[1]
    assert ext.logreg_fused_supported(f, k)
    # the kernel adds into the payload: the contract is a zeroed one
    payload = torch.zeros(1 + (f + 1) * k, dtype=torch.float32, device=DEV)
    ext.logreg_loss_grad(payload, x.to(DEV) if x_dev is None else x_dev,
                         y.to(DEV), w.to(DEV), wmat.to(DEV), bias)
    return payload.cpu()


def test_launch_table_is_complete(ext):
    for k, top in MAX_NC.items():
        assert ext.logreg_fused_supported(256 * top, k)
        assert not ext.logreg_fused_supported(256 * top + 1, k)
    assert not ext.logreg_fused_supported(16, 1)
    assert not ext.logreg_fused_supported(16, 9)


@pytest.mark.parametrize("nc,k", INSTANTIATIONS)
def test_every_instantiation_against_float64(ext, nc, k):
    # ragged last chunk, and F % 4 == 1: every row after the first starts
    # off a 16-byte boundary
    f = 256 * nc - 3
    x, y, w, wmat = U.inputs(333, f, k, True, 0.05)
    got = _run_narrow(ext, x, y, w, wmat, True)
    U.check(f"logreg_narrow NC={nc}", got, x, y, w, wmat, True)


@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("f", [1, 3, 4, 123, 255, 256, 257])
def test_feature_counts(ext, f, k):
    x, y, w, wmat = U.inputs(333, f, k, True, 0.05)
    got = _run_narrow(ext, x, y, w, wmat, True)
    U.check("logreg_narrow", got, x, y, w, wmat, True)


@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("n", [1, 2, 3, 31, 33])
def test_row_counts(ext, n, k):
    # the tail of the two-rows-per-iteration loop, fewer rows than waves
    x, y, w, wmat = U.inputs(n, 123, k, True, 0.05)
    got = _run_narrow(ext, x, y, w, wmat, True)
    U.check("logreg_narrow", got, x, y, w, wmat, True)


@pytest.mark.parametrize("k", [2, 3, 8])
def test_zero_weights_give_a_zero_payload(ext, k):
    x, y, w, wmat = U.inputs(333, 123, k, True, 0.05)
    got = _run_narrow(ext, x, y, torch.zeros_like(w), wmat, True)
    assert (got == 0).all()


@pytest.mark.parametrize("k", [2, 3, 8])
def test_all_weight_on_the_last_row(ext, k):
    x, y, w, wmat = U.inputs(333, 123, k, True, 0.05)
    w = torch.zeros_like(w)
    w[-1] = 1.5
    got = _run_narrow(ext, x, y, w, wmat, True)
    U.check("logreg_narrow last row only", got, x, y, w, wmat, True)


@pytest.mark.parametrize("k", [2, 3, 8])
def test_no_bias_leaves_bias_gradient_zero(ext, k):
    x, y, w, wmat = U.inputs(333, 123, k, False, 0.05)
    got = _run_narrow(ext, x, y, w, wmat, False)
    assert (got[1 + 123 * k:] == 0).all()
    U.check("logreg_narrow no bias", got, x, y, w, wmat, False)


@pytest.mark.parametrize("k", [2, 3, 8])
def test_unaligned_base_pointer(ext, k):
    n, f = 333, 256  # F % 4 == 0: only the base pointer is off the boundary
    x, y, w, wmat = U.inputs(n, f, k, True, 0.05)
    buf = torch.empty(n * f + 1, dtype=torch.float32, device=DEV)
    x_dev = buf[1:1 + n * f].view(n, f)
    x_dev.copy_(x)
    assert x_dev.is_contiguous() and x_dev.data_ptr() % 16 != 0
    got = _run_narrow(ext, x, y, w, wmat, True, x_dev=x_dev)
    U.check("logreg_narrow base pointer + 4 bytes", got, x, y, w, wmat, True)


@pytest.mark.parametrize("k", [2, 3, 8])
def test_large_margins(ext, k):
    # margins of about +-80 through __expf / __logf
    x, y, w, wmat = U.inputs(333, 123, k, True, 5.0)
    got = _run_narrow(ext, x, y, w, wmat, True)
    assert torch.isfinite(got).all()
    U.check("logreg_narrow scale 5.0", got, x, y, w, wmat, True)


def _dispatch(f, k, device, n=64):
    from spark_ensemble_amd.ops import dispatch

    x, y, w, wmat = (t.to(device) for t in U.inputs(n, f, k, True, 0.05))
    got = dispatch.logreg_loss_grad(x, y, w, wmat, True, native_only=True)
    return got, dict(dispatch.last_logreg_info)


@pytest.mark.parametrize("f,k,path", [(256, 2, "narrow"), (768, 2, "wide"),
                                      (1280, 2, "narrow")])
def test_dispatch_records_the_kernel(f, k, path):
    got, info = _dispatch(f, k, DEV)
    assert got is not None and info["path"] == path
    geometry = [info[key] for key in ("kp", "slices", "rows_per_tile",
                                      "lds_bytes", "nt", "db")]
    if path == "wide":
        assert geometry[:3] == [16, 8, 16] and geometry[3] > 0
    else:
        assert geometry == [0] * 6
    x, y, w, wmat = U.inputs(64, f, k, True, 0.05)
    U.check(f"logreg dispatch {path}", got, x, y, w, wmat, True)


def test_dispatch_reference_on_cpu():
    got, info = _dispatch(256, 2, "cpu")
    assert got is None and info["path"] == "reference"


def test_dispatch_declines_past_both_kernels():
    got, info = _dispatch(1025, 9, DEV)
    assert got is None and info["path"] == "reference"
