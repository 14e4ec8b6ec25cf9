"""GPU tests of the MFMA logistic loss+gradient kernel (csrc/linear_wide.hip)
through dispatch.logreg_loss_grad and LogisticRegression.fit.

The reference is reference.logreg_loss_grad on float64 inputs on the CPU.
The bound is 16x the error of the same function on the float32 inputs: the
kernel's transcendental functions and its summation order differ from
torch's, its number format does not.  The first ten cases keep their first
comparison (one largest-entry normaliser for the gradient); every case goes
through tests/logreg_util.py, which gives each payload entry its own
denominator.

Every case names the planner branch it is there for as (S, NT, db) and
asserts that dispatch ran that geometry on the MFMA kernel:
test_cases_cover_every_branch keeps the list honest.
"""

import pytest
import torch

import logreg_util as U

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# row counts in units of the block tile (rows of the geometry) and the grid
ROUND = "one tile past a full grid-stride round"
TWO = "one tile past two full grid-stride rounds"
TILE_M1, TILE, TILE_P1 = "one row short of a tile", "one tile", "a tile and a row"

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

# (F, K) -> (S, NT, db) of every shape in this file
GEOMETRY = {
    (1, 2): (1, 1, 1), (1, 9): (1, 1, 1), (16, 9): (1, 1, 1),
    (16, 26): (1, 1, 1),
    (31, 9): (1, 2, 1), (31, 26): (1, 2, 1),
    (36, 9): (1, 4, 1), (36, 26): (1, 4, 1),
    (100, 9): (1, 8, 1), (100, 26): (1, 8, 0), (128, 17): (1, 8, 0),
    (130, 26): (2, 8, 1), (240, 26): (2, 8, 1),
    (244, 9): (2, 8, 1), (244, 26): (2, 8, 0),
    (257, 26): (4, 8, 1), (512, 32): (4, 8, 1),
    (515, 32): (8, 8, 1), (1024, 2): (8, 8, 1), (1024, 3): (8, 8, 1),
    (1024, 16): (8, 8, 1), (1024, 17): (8, 8, 1), (1024, 32): (8, 8, 1),
}

BRANCH_CASES = [
    (333, 31, 9, True),     # KP 16, NT 2, ragged last tile, scalar staging
    (333, 31, 26, True),    # KP 32, NT 2
    (333, 36, 9, False),    # KP 16, NT 4 with 3 live tiles, vectorised
    (333, 36, 26, True),    # KP 32, NT 4
    (333, 100, 26, True),   # db = 0, single tile per block
    (ROUND, 100, 26, True),  # db = 0 with a next tile held over phase 2
    (TWO, 100, 26, False),  # db = 0, three tiles on block 0
    (ROUND, 128, 17, True),  # db = 0, T = 8, first K padded to 32
    (333, 130, 26, True),   # S = 2, slices of 5 and 4 tiles
    (ROUND, 244, 26, True),  # S = 2, db = 0
    (ROUND, 244, 9, True),  # same F, KP 16: db = 1
    (TWO, 240, 26, True),   # S = 2, db = 1: the third tile returns to buffer 0
    (333, 257, 26, True),   # S = 4, last slice 2 of 5 tiles
    (ROUND, 512, 32, True),  # S = 4 full
    (ROUND, 515, 32, True),  # S = 8, one slice with 0 tiles, past one round
    (TWO, 1024, 2, True),   # K = 2 on the wide path, largest F
    (TILE_M1, 100, 26, True),  # row-group edges
    (TILE, 100, 26, True),
    (TILE_P1, 100, 26, True),
    (1, 1, 9, True),        # the smallest shape dispatch sends here
]

EDGE_SHAPES = [(333, 100, 26), (333, 515, 32)]  # db = 0; S = 8, scalar staging


def _rows(n, f, k):
    if isinstance(n, int):
        return n
    from spark_ensemble_amd.ops import dispatch

    tile = dispatch._load_hip().logreg_wide_geometry(f, k)[2]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return {ROUND: cus * tile + 1, TWO: 2 * cus * tile + 1, TILE_M1: tile - 1,
            TILE: tile, TILE_P1: tile + 1}[n]


def _inputs(n, f, k, bias, scale, colscale=False):
    return U.inputs(_rows(n, f, k), f, k, bias, scale, colscale)


def _errors(got, want):
    loss = float((got[0].double() - want[0]).abs() / want[0].abs())
    grad = float((got[1:].double() - want[1:]).abs().max() / want[1:].abs().max())
    return loss, grad


def _run_wide(x, y, w, wmat, bias, x_dev=None):
    """The payload of the MFMA kernel on the CPU, after asserting that
    dispatch took that kernel with the geometry this file expects."""
    from spark_ensemble_amd.ops import dispatch

    f, k = x.shape[1], wmat.shape[1]
    got = dispatch.logreg_loss_grad(
        x.to(DEV) if x_dev is None else x_dev, y.to(DEV), w.to(DEV),
        wmat.to(DEV), bias, native_only=True)
    assert got is not None
    info = dispatch.last_logreg_info
    assert info["path"] == "wide", info
    assert (info["slices"], info["nt"], info["db"]) == GEOMETRY[(f, k)], info
    assert info["kp"] == (16 if k <= 16 else 32)
    assert info["rows_per_tile"] * info["slices"] == 128
    return got.cpu()


def test_cases_cover_every_branch():
    shapes = [(f, k) for _, f, k, _, _ in CASES]
    shapes += [(f, k) for _, f, k, _ in BRANCH_CASES]
    geo = [GEOMETRY[s] for s in shapes]
    templates = {(16 if k <= 16 else 32, GEOMETRY[(f, k)][1]) for f, k in shapes}
    assert templates == {(kp, nt) for kp in (16, 32) for nt in (1, 2, 4, 8)}
    assert {g[0] for g in geo} == {1, 2, 4, 8}
    assert {g[2] for g in geo} == {0, 1}
    # a single-buffer shape with more than one tile, and with a third tile
    assert any(GEOMETRY[(f, k)][2] == 0 and n == ROUND
               for n, f, k, _ in BRANCH_CASES)
    assert any(GEOMETRY[(f, k)][2] == 0 and n == TWO
               for n, f, k, _ in BRANCH_CASES)


@pytest.mark.parametrize("n,f,k,bias,scale", CASES)
def test_payload_against_float64(n, f, k, bias, scale):
    from spark_ensemble_amd.ops import reference

    x, y, w, wmat = _inputs(n, f, k, bias, scale)
    got = _run_wide(x, y, w, wmat, bias)
    assert torch.isfinite(got).all()
    want = reference.logreg_loss_grad(x.double(), y, w.double(), wmat.double(), bias)
    ref32 = reference.logreg_loss_grad(x, y, w, wmat, bias)
    loss, grad = _errors(got, want)
    loss32, grad32 = _errors(ref32, want)
    print(f"logreg_wide {x.shape[0]}x{f}x{k} scale {scale}: loss {loss:.2e} "
          f"(f32 torch {loss32:.2e}), grad {grad:.2e} (f32 torch {grad32:.2e})")
    assert loss <= 16 * loss32
    assert grad <= 16 * grad32
    U.check(f"logreg_wide scale {scale}", got, x, y, w, wmat, bias)


@pytest.mark.parametrize("n,f,k,bias", BRANCH_CASES)
def test_planner_branches_against_float64(n, f, k, bias):
    x, y, w, wmat = _inputs(n, f, k, bias, 0.05)
    got = _run_wide(x, y, w, wmat, bias)
    U.check(f"logreg_wide {GEOMETRY[(f, k)]}", got, x, y, w, wmat, bias)
    if not bias:
        assert (got[1 + f * k:] == 0).all()


def test_smallest_everything():
    # one row, one feature, two classes.  dispatch keeps K <= 8 at F <= 512 on
    # the narrow kernel, so this shape reaches the MFMA kernel through its
    # binding alone
    from spark_ensemble_amd.ops import dispatch

    m = dispatch._load_hip()
    x, y, w, wmat = _inputs(1, 1, 2, True, 0.05)
    geo = m.logreg_wide_geometry(1, 2)
    assert (geo[1], geo[4], geo[5]) == GEOMETRY[(1, 2)]
    got = torch.empty(1 + 2 * 2, dtype=torch.float32, device=DEV)
    m.logreg_loss_grad_wide(got, x.to(DEV), y.to(DEV), w.to(DEV),
                            wmat.to(DEV), True)
    U.check(f"logreg_wide {GEOMETRY[(1, 2)]}", got.cpu(), x, y, w, wmat, True)


@pytest.mark.parametrize("n,f,k", EDGE_SHAPES)
def test_zero_weights_give_a_zero_payload(n, f, k):
    x, y, w, wmat = _inputs(n, f, k, True, 0.05)
    got = _run_wide(x, y, torch.zeros_like(w), wmat, True)
    assert (got == 0).all()


@pytest.mark.parametrize("n,f,k", EDGE_SHAPES)
def test_all_weight_on_the_last_row(n, f, k):
    x, y, w, wmat = _inputs(n, f, k, True, 0.05)
    w = torch.zeros_like(w)
    w[-1] = 1.5  # the last row sits in the ragged tail tile
    got = _run_wide(x, y, w, wmat, True)
    U.check("logreg_wide last row only", got, x, y, w, wmat, True)


@pytest.mark.parametrize("last", [True, False])
@pytest.mark.parametrize("n,f,k", EDGE_SHAPES)
def test_one_label_everywhere(n, f, k, last):
    x, y, w, wmat = _inputs(n, f, k, True, 0.05)
    y = torch.full_like(y, k - 1 if last else 0)
    got = _run_wide(x, y, w, wmat, True)
    U.check(f"logreg_wide every label {int(y[0])}", got, x, y, w, wmat, True)


@pytest.mark.parametrize("n,f,k", EDGE_SHAPES)
def test_no_bias_leaves_bias_gradient_zero(n, f, k):
    x, y, w, wmat = _inputs(n, f, k, False, 0.05)
    got = _run_wide(x, y, w, wmat, False)
    assert (got[1 + f * k:] == 0).all()
    U.check("logreg_wide no bias", got, x, y, w, wmat, False)


@pytest.mark.parametrize("n,f,k", EDGE_SHAPES)
def test_large_margins(n, f, k):
    x, y, w, wmat = _inputs(n, f, k, True, 5.0)
    got = _run_wide(x, y, w, wmat, True)
    assert torch.isfinite(got).all()
    U.check("logreg_wide scale 5.0", got, x, y, w, wmat, True)


@pytest.mark.parametrize("n,f,k", EDGE_SHAPES)
def test_unequal_column_scales(n, f, k):
    x, y, w, wmat = _inputs(n, f, k, True, 0.05, colscale=True)
    got = _run_wide(x, y, w, wmat, True)
    U.check("logreg_wide columns 1e-3..1e3", got, x, y, w, wmat, True)


def test_unaligned_base_pointer():
    # F % 4 == 0, so only the base pointer sends the kernel to scalar staging
    n, f, k = 333, 100, 26
    x, y, w, wmat = _inputs(n, f, k, True, 0.05)
    buf = torch.empty(n * f + 1, dtype=torch.float32, device=DEV)
    x_dev = buf[1:1 + n * f].view(n, f)
    x_dev.copy_(x)
    assert x_dev.is_contiguous() and x_dev.data_ptr() % 16 != 0
    got = _run_wide(x, y, w, wmat, True, x_dev=x_dev)
    U.check("logreg_wide base pointer + 4 bytes", got, x, y, w, wmat, True)
    aligned = _run_wide(x, y, w, wmat, True)
    assert torch.equal(got, aligned)  # the staging path changes no arithmetic


@pytest.mark.parametrize("n,f,k", [(1000, 515, 32), (ROUND, 16, 26),
                                   (ROUND, 100, 26), (ROUND, 244, 26)])
def test_reproducible(n, f, k):
    from spark_ensemble_amd.ops import dispatch

    args = [t.to(DEV) for t in _inputs(n, f, k, True, 0.05)]
    a = dispatch.logreg_loss_grad(*args, True, native_only=True)
    b = dispatch.logreg_loss_grad(*args, True, native_only=True)
    assert dispatch.last_logreg_info["path"] == "wide"
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
