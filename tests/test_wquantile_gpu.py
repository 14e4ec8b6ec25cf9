"""The gfx950 forest_wquantile kernel against the reference op on the CPU, and
``predict`` / ``predictQuantile`` of the regression ensembles on the GPU.

Every comparison is ``torch.equal``: weights are multiples of 1/8 and
probabilities multiples of 1/16, so the float64 sums of the reference are
exact, as the integer sums of the kernel always are.  Integer leaves
(tests/serving_util.py) make equal member values common.  Shapes come from
``forest_wquantile_geometry()``."""

import pytest
import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.ensemble.utils import slice_features
from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.ops import reference
from spark_ensemble_amd.utils.io import synthetic_regression

import serving_util as S

pytestmark = pytest.mark.gpu

PROBS = {1: [0.5], 3: [0.0, 0.5, 1.0],
         16: [0.0, 1.0] + [k / 16 for k in range(1, 15)]}


def rows_per_block(M):
    m_pad = 1 << (M - 1).bit_length()
    return next(r for lim, r in ops.forest_wquantile_geometry()["rows"]
                if m_pad <= lim)


def run(x, trees, w, probs, expect="native"):
    got = ops.forest_wquantile(x.cuda(), trees, w, probs)
    info = dict(ops.last_forest_wquantile_info)
    assert info["path"] == expect, info
    assert got.is_cuda and got.dtype == torch.float32
    assert torch.equal(got.cpu(), reference.forest_wquantile(x, trees, w, probs))
    return info


def case(seed, n, M, pattern="eighths", F=7, depth=5):
    g = torch.Generator().manual_seed(seed)
    trees = [S.rand_tree(depth, F, 1, g, S.SPECIALS_POOL, p_stop=0.2)
             for _ in range(M)]
    w = torch.randint(1, 33, (M,), generator=g).float() / 8  # (0, 4]
    if pattern == "ones":  # exact-half ties at even M
        w = torch.ones(M)
    elif pattern == "signed":
        w[M // 2] = 0.0
        w[-1] = -w[-1]
    return S.special_x(n, F, S.SPECIALS_POOL, g), trees, w


@pytest.mark.parametrize("n", [1, 63, 65, "R-1", "R", "R+1"])
def test_row_counts(n):
    R = rows_per_block(35)
    if isinstance(n, str):
        n = R + {"R-1": -1, "R": 0, "R+1": 1}[n]
    info = run(*case(n, n, 35), PROBS[3])
    assert info["rows_per_block"] == R


def test_row_count_wraps_the_grid():
    n = ops.forest_wquantile_geometry()["max_blocks"] * rows_per_block(3) + 1
    run(*case(7, n, 3, F=4, depth=3), PROBS[1])


@pytest.mark.parametrize("pattern", ["ones", "eighths", "signed"])
@pytest.mark.parametrize("M", [1, 2, 3, 31, 32, 33, 64, 65, 128, 129, 256])
def test_member_counts(M, pattern):
    info = run(*case(20 + M, 300, M, pattern), PROBS[3])
    assert info["rows_per_block"] == rows_per_block(M)


@pytest.mark.parametrize("Q", sorted(PROBS))
def test_probability_counts(Q):
    run(*case(40 + Q, 300, 21, "signed"), PROBS[Q])


def test_node_group_boundary():
    budget = ops.forest_wquantile_geometry()["group_nodes"]
    g = torch.Generator().manual_seed(50)
    trees = [S.complete_tree(9, 6, 1, g, S.INT_POOL)
             for _ in range(budget // 1023 + 2)]
    x = S.special_x(300, 6, S.INT_POOL, g)
    info = run(x, trees, torch.ones(len(trees)), PROBS[3])
    assert info["groups"] >= 2


@pytest.mark.parametrize("mode", ["raw", "binned"])
def test_walk_modes(mode, monkeypatch):
    """NaN, +-inf and ties with every threshold, in both row forms."""
    monkeypatch.setenv("SEA_WQUANTILE_MODE", mode)
    info = run(*case(60, 700, 40, F=9, depth=6), PROBS[3])
    assert info["mode"] == mode


@pytest.mark.parametrize("why", ["M 257", "NaN leaf", "weights", "Q 17"])
def test_routes_to_reference(why):
    x, trees, w = case(70, 130, 257 if why == "M 257" else 2)
    probs = PROBS[3]
    if why == "NaN leaf":
        leaf = trees[1]["feature"] < 0
        trees[1]["leaf_value"][leaf.nonzero()[0, 0]] = float("nan")
        probs = [0.0]  # the smallest value: never the NaN, which sorts last
    elif why == "weights":
        w = torch.tensor([1.0, 2.0 ** -70])
    elif why == "Q 17":
        probs = [k / 16 for k in range(17)]
    run(x, trees, w, probs, expect="reference")


def test_predict_keeps_its_old_route_where_the_kernel_does_not_serve():
    from spark_ensemble_amd.ensemble.utils import weighted_median
    from spark_ensemble_amd.models.tree import DecisionTreeRegressionModel
    from spark_ensemble_amd.regression.boosting import BoostingRegressionModel

    x, trees, _ = case(80, 130, 2)
    m = BoostingRegressionModel()
    m._models = [DecisionTreeRegressionModel() for _ in trees]
    for mm, t in zip(m._models, S.to_dev(trees, "cuda")):
        mm._set_tree(t, x.shape[1])
    m._weights = [1.0, 2.0 ** -70]
    m.set("votingStrategy", "median")
    got = m.predict(x.cuda())
    assert ops.last_forest_wquantile_info["path"] == "reference"
    preds = torch.stack([mm.predict(x.cuda()) for mm in m._models], dim=1)
    w = torch.tensor(m._weights, device="cuda")
    assert torch.equal(got, weighted_median(preds, w.expand_as(preds)))


@pytest.mark.parametrize("kind", ["boosting", "bagging"])
def test_models(kind):
    df = synthetic_regression(1500, 12, seed=17, device="cuda")
    x = df["features"]
    tree = sea.DecisionTreeRegressor().setMaxDepth(4)
    if kind == "boosting":
        m = (sea.BoostingRegressor().setBaseLearner(tree)
             .setNumBaseLearners(8).fit(df))
        assert m.numModels >= 6
        w, subs = m.weights, [None] * m.numModels
    else:
        m = (sea.BaggingRegressor().setBaseLearner(tree)
             .setNumBaseLearners(9).setSubspaceRatio(0.6).setSeed(5).fit(df))
        w, subs = [1.0] * m.numModels, m.subspaces
    preds = torch.stack(
        [mm.predict(x if s is None else slice_features(x, s))
         for mm, s in zip(m.models, subs)], dim=1).cpu()
    probs = [0.25, 0.5, 1.0]
    want = reference.weighted_quantile(preds, w, probs)
    got = m.predictQuantile(x, probs)
    assert ops.last_forest_wquantile_info["path"] == "native"
    assert torch.equal(got.cpu(), want)
    assert torch.equal(m.predictQuantile(x, probs), got)
    if kind == "boosting":
        ops.last_forest_wquantile_info.clear()
        first = m.predict(x)
        assert ops.last_forest_wquantile_info["path"] == "native"
        assert torch.equal(first.cpu(), want[:, 1])
        assert torch.equal(m.predict(x), first)
