"""The gfx950 forest_staged_loss kernel against the float64 reference op,
and evaluateEachIteration on the GPU.

Tolerance, per case and per stage (tests/staged_eval_util.py):
|got[s] - r64[s]| <= 4 * e_ref32[s] + 2^-23 * sum_i w_i max(|loss_i|, 1),
r64 / r32 the reference op on x.double() / x.float(), both on the CPU.
Measured figures per shape: profiles/staged_eval.md."""

import pytest
import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.boosting.losses import LogLoss
from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.utils.io import (
    synthetic_classification, synthetic_regression)

import staged_eval_util as U

pytestmark = pytest.mark.gpu


def geometry():
    threads, rows_per_lane, max_blocks = ops._load_hip().forest_staged_geometry()
    return threads * rows_per_lane, max_blocks


def run(args, expect="native", label="", cache=None):
    x, trees, weights, init, lab, w, loss = args
    got = ops.forest_staged_loss(
        x.cuda(), trees, weights, init.shape[1], init.cuda(), lab.cuda(),
        w.cuda(), loss, cache=cache)
    torch.cuda.synchronize()
    info = dict(ops.last_forest_staged_info)
    assert info["path"] == expect, info
    assert got.is_cuda
    U.check_op(got, args, label=f"{label} {info['mode']}")
    return got, info


@pytest.mark.parametrize("n", [1, 63, 64, 65, "tile-1", "tile", "tile+1"])
def test_row_counts(n):
    tile, _ = geometry()
    if isinstance(n, str):
        n = tile + {"tile-1": -1, "tile": 0, "tile+1": 1}[n]
    _, info = run(U.case(n, n, 8, 1, 3, "squared"), label="rows")
    assert info["rows_per_lane"] * 1024 == tile


def test_row_count_wraps_the_grid():
    tile, max_blocks = geometry()
    n = max_blocks * tile + 1
    run(U.case(7, n, 8, 1, 2, "squared", depth=3), label="grid wrap")


def test_group_boundary_inside_a_stage():
    """51 full depth-9 trees (1023 nodes each) at dim 3: 17 stages in three
    LDS groups, with a group boundary between the trees of one stage."""
    args = U.case(51, 300, 12, 3, 17, "logloss",
                  tree_fn=lambda g: U.full_tree(g, 12, 9, scale=0.3))
    cache = {}
    _, info = run(args, label="3 groups", cache=cache)
    groups = cache["pack"]["groups_t"].cpu()
    assert info["groups"] == groups.shape[0] >= 3
    assert int(cache["pack"]["feats"].numel()) > 2 * ops._FP2_GROUP_NODES
    firsts = groups[1:, 0].tolist()
    assert any(f % 3 != 0 for f in firsts), firsts  # mid-stage boundary


def test_single_group_forest():
    cache = {}
    _, info = run(U.case(52, 300, 12, 3, 4, "logloss"), label="1 group",
                  cache=cache)
    assert info["groups"] == 1 == cache["pack"]["groups_t"].shape[0]


@pytest.mark.parametrize("dim", [1, 2, 3, 8])
def test_dims(dim):
    name = "logloss" if dim > 1 else "logcosh"
    run(U.case(60 + dim, 200, 9, dim, 5, name), label="dim")


def test_dim_nine_routes_to_reference():
    run(U.case(69, 130, 9, 9, 3, "logloss"), expect="reference", label="dim 9")


@pytest.mark.parametrize("stages", [0, 1])
def test_few_stages(stages):
    got, _ = run(U.case(70 + stages, 130, 9, 1, stages, "squared"),
                 label="stages")
    assert got.numel() == stages + 1
    got, _ = run(U.case(72 + stages, 130, 9, 3, stages, "logloss"),
                 label="stages")
    assert got.numel() == stages + 1


def test_forest_without_splits():
    """Single-leaf trees only: no threshold set to rank rows against."""
    g = torch.Generator().manual_seed(5)
    args = list(U.case(74, 130, 9, 1, 3, "squared"))
    args[1] = [U.random_tree(g, 9, 0) for _ in range(3)]
    assert all(t["feature"].numel() == 1 for t in args[1])
    _, info = run(tuple(args), label="leaf-only")
    assert info["mode"] == "raw"


@pytest.mark.parametrize("name", U.ALL_LOSSES)
def test_losses(name):
    dim = 3 if name == "logloss" else 1
    run(U.case(80, 500, 9, dim, 6, name), label="loss")


@pytest.mark.parametrize("name", ["exponential", "bernoulli"])
def test_large_margins(name):
    """Leaf values scaled so margins reach |85| (the conventions of
    tests/test_loss_kernels.py: exponential stays finite in f32 below 88,
    bernoulli's 2|m| = 170 is past f32 exp overflow)."""
    args = U.case(81, 500, 9, 1, 8, name, scale=12.0)
    x, trees, weights, init, lab, w, loss = args
    from spark_ensemble_amd.ops import reference

    m = init[:, 0].double() + reference.forest_predict(
        x.double(), trees, torch.tensor(weights, dtype=torch.float64))[:, 0]
    # rescale leaves and init so the largest |margin| is 85
    s = 85.0 / float(m.abs().max())
    trees = [dict(t, leaf_value=t["leaf_value"] * s) for t in trees]
    args = (x, trees, weights, init * s, lab, w, loss)
    m = m * s
    assert float(m.abs().max()) >= 80.0
    run(args, label="|margin| >= 80")


def test_absolute_loss_ties():
    """label == prediction exactly, at every stage for a block of rows."""
    args = list(U.case(82, 300, 9, 1, 3, "absolute"))
    x, trees, weights, init = args[:4]
    # dyadic leaves and weights: the margins are exact in f32
    trees = [dict(t, leaf_value=(t["leaf_value"] * 4).round() / 4)
             for t in trees]
    weights = [0.5, 1.0, 2.0]
    init = (init * 4).round() / 4
    from spark_ensemble_amd.ops import reference

    final = init[:, 0] + reference.forest_predict(
        x, trees, torch.tensor(weights))[:, 0]
    lab = args[4].clone()
    lab[:100, 0] = final[:100]   # ties after the last stage
    lab[100:200, 0] = init[100:200, 0]  # ties at entry 0
    args[1], args[2], args[3], args[4] = trees, weights, init, lab
    got, _ = run(tuple(args), label="ties")
    assert bool(torch.isfinite(got).all())


@pytest.mark.parametrize("nf", [1, 300])
def test_feature_counts(nf):
    run(U.case(90 + nf, 700, nf, 1, 5, "squared", depth=5), label="F")


@pytest.mark.parametrize("mode", ["raw", "binned"])
def test_row_modes(mode, monkeypatch):
    monkeypatch.setenv("SEA_STAGED_MODE", mode)
    for dim, name in ((1, "bernoulli"), (3, "logloss")):
        _, info = run(U.case(95, 700, 40, dim, 5, name, depth=6), label="mode")
        assert info["mode"] == mode


def test_default_row_mode_is_binned():
    _, info = run(U.case(96, 200, 9, 1, 3, "squared"), label="default mode")
    assert info["mode"] == "binned"


def test_bitwise_determinism():
    x, trees, weights, init, lab, w, loss = U.case(
        97, 9000, 12, 3, 6, "logloss", depth=6)
    dev = [t.cuda() for t in (x, init, lab, w)]
    cache = {}

    def call():
        return ops.forest_staged_loss(dev[0], trees, weights, 3, dev[1],
                                      dev[2], dev[3], loss, cache=cache)

    first = call()
    assert ops.last_forest_staged_info["path"] == "native"
    for _ in range(3):
        assert torch.equal(call(), first)


@pytest.mark.parametrize("name", ["squared", "bernoulli", "logloss"])
def test_nan_label_surfaces(name):
    dim = 3 if name == "logloss" else 1
    x, trees, weights, init, lab, w, loss = U.case(98, 300, 9, dim, 4, name)
    lab = lab.clone()
    lab[17, 0] = float("nan")
    got = ops.forest_staged_loss(x.cuda(), trees, weights, dim, init.cuda(),
                                 lab.cuda(), w.cuda(), loss)
    assert ops.last_forest_staged_info["path"] == "native"
    assert got.numel() == 5 and bool(torch.isnan(got).all())


# ---- model level -----------------------------------------------------------

def _fit_and_check(est, frame, lo, label):
    """Fit on the GPU; the curve there and the curve of the same model on
    the CPU both meet the float64 prefix definition."""
    m = est.fit(frame)
    ops.last_forest_staged_info.clear()
    got, r64, tol, _ = U.check_model(m, frame, eval_loss=lo, label=label)
    assert ops.last_forest_staged_info.get("path") == "native"
    cpu_frame = frame.to("cpu")
    cpu_got = m.evaluateEachIteration(cpu_frame)
    assert ops.last_forest_staged_info["path"] == "reference"
    assert bool(((cpu_got - r64).abs() <= tol).all())
    assert bool(((cpu_got - got).abs() <= tol).all())
    return m


def test_model_regressors():
    reg = synthetic_regression(4000, 20, seed=17, device="cuda")
    _fit_and_check(sea.GBMRegressor().setNumBaseLearners(6), reg,
                   U.make_loss("squared"), "gpu squared")
    from spark_ensemble_amd.boosting.losses import get_regression_loss

    _fit_and_check(
        sea.GBMRegressor().setLoss("quantile").setAlpha(0.7)
        .setNumBaseLearners(6).setSubspaceRatio(0.5), reg,
        get_regression_loss("quantile", alpha=0.7), "gpu quantile subspace")


def test_model_classifiers():
    binf = synthetic_classification(4000, 20, k=2, seed=13, device="cuda")
    _fit_and_check(sea.GBMClassifier().setLoss("bernoulli")
                   .setNumBaseLearners(6), binf, U.make_loss("bernoulli"),
                   "gpu bernoulli")
    clf3 = synthetic_classification(4000, 20, k=3, seed=11, device="cuda")
    _fit_and_check(sea.GBMClassifier().setLoss("logloss")
                   .setNumBaseLearners(6), clf3, LogLoss(3), "gpu logloss")


def test_model_linear_base_learner_generic_path():
    from spark_ensemble_amd.models import LinearRegression

    reg = synthetic_regression(4000, 20, seed=17, device="cuda")
    m = (sea.GBMRegressor().setBaseLearner(LinearRegression())
         .setNumBaseLearners(4).fit(reg))
    ops.last_forest_staged_info.clear()
    U.check_model(m, reg, eval_loss=U.make_loss("squared"), label="gpu linear")
    assert not ops.last_forest_staged_info


@pytest.mark.parametrize("kind", ["squared", "bernoulli"])
def test_model_replays_validation_curve(kind):
    if kind == "squared":
        frame = synthetic_regression(4000, 20, seed=17, device="cuda")
        est = sea.GBMRegressor().setLoss("squared")
    else:
        frame = synthetic_classification(4000, 20, k=2, seed=13, device="cuda")
        est = sea.GBMClassifier().setLoss("bernoulli")
    g = torch.Generator().manual_seed(3)
    val = (torch.rand(frame.count(), generator=g) < 0.3).cuda()
    full = frame.withColumn("val", val.float())
    est = (est.setNumBaseLearners(6).setValidationIndicatorCol("val")
           .setNumRounds(100))
    m = est.fit(full)
    hist = torch.tensor([r["val_loss"] for r in est._instr.history],
                        dtype=torch.float64)
    assert m.numModels == 6 and hist.numel() == 6
    got, r64, tol, e_ref32 = U.check_model(
        m, full.filter(val), eval_loss=U.make_loss(kind),
        label="gpu replay " + kind)
    assert ops.last_forest_staged_info["path"] == "native"
    # the fit's own val_loss entries, to the same tolerance
    assert bool(((got[1:] - hist).abs() <= tol[1:]).all())


def test_model_replays_early_stopped_curve():
    """A small numRounds stops the fit early and drops the last stages: the
    curve has numModels + 1 entries that match the first numModels history
    entries."""
    frame = synthetic_regression(4000, 20, seed=17, device="cuda")
    g = torch.Generator().manual_seed(4)
    val = (torch.rand(frame.count(), generator=g) < 0.3).cuda()
    full = frame.withColumn("val", val.float())
    est = (sea.GBMRegressor().setNumBaseLearners(12)
           .setValidationIndicatorCol("val").setNumRounds(1)
           .setValidationTol(0.2))
    m = est.fit(full)
    hist = torch.tensor([r["val_loss"] for r in est._instr.history],
                        dtype=torch.float64)
    k = m.numModels
    assert hist.numel() - k >= 1 and 1 <= k < 12
    got, r64, tol, _ = U.check_model(
        m, full.filter(val), eval_loss=U.make_loss("squared"),
        label="gpu replay early stop")
    assert ops.last_forest_staged_info["path"] == "native"
    assert got.numel() == k + 1
    assert bool(((got[1:] - hist[:k]).abs() <= tol[1:]).all())
