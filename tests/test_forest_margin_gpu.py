"""The gfx950 forest_margin kernel against the float64 oracle walk, plane by
plane.  Leaves are integers in [-64, 64], weights in {0.5, 1, 2} and a plane
has at most 64 trees, so every partial sum is an exact f32 and every
comparison with the oracle is ``torch.equal``."""

import pytest
import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.ensemble.utils import slice_features
from spark_ensemble_amd.models.dummy import DummyRegressionModel
from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.utils.io import synthetic_classification

import serving_util as S
from test_forest_margin import PLANES, expected, forest

pytestmark = pytest.mark.gpu

MODES = ["raw", "binned"]
POOLS = {"int": S.INT_POOL, "specials": S.SPECIALS_POOL}


def check(mp, x, trees, w, planes, P, mode=None):
    if mode is not None:
        mp.setenv("SEA_MARGIN_MODE", mode)
    got = ops.forest_margin(x.cuda(), S.to_dev(trees, "cuda"), w, planes, P)
    info = dict(ops.last_forest_margin_info)
    assert info["path"] == "native" and info["planes"] == P, info
    assert info["mode"] == (mode or "binned"), info
    assert got.dtype == torch.float32 and got.shape == (x.shape[0], P)
    assert torch.equal(got.cpu().double(), expected(x, trees, w, planes, P))
    return info


@pytest.mark.parametrize("mode", MODES)
def test_plane_and_group_boundaries_apart(monkeypatch, mode):
    g = torch.Generator().manual_seed(1)
    # 42 x 1023 nodes: group cuts at trees 19 and 38, plane cuts at 14 and 28
    trees = [S.complete_tree(9, 5, 1, g, S.INT_POOL) for _ in range(42)]
    planes = [t % 3 for t in range(42)]
    x = S.special_x(300, 5, S.INT_POOL, g)
    info = check(monkeypatch, x, trees, S.rand_weights(42, g), planes, 3, mode)
    assert info["groups"] == 3


@pytest.mark.parametrize("pool", sorted(POOLS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", PLANES)
def test_plane_switches_in_one_group(monkeypatch, P, mode, pool):
    g = torch.Generator().manual_seed(P)
    trees, w, planes = forest(P, g, POOLS[pool])
    x = S.special_x(500, 6, POOLS[pool], g)
    info = check(monkeypatch, x, trees, w, planes, P, mode)
    assert info["groups"] == 1


@pytest.mark.parametrize("n", [1, "tile-1", "tile+1", "wrap"])
def test_row_tails(monkeypatch, n):
    geo = ops.forest_margin_geometry()
    tile = geo["threads"] * geo["rows_per_lane"]
    g = torch.Generator().manual_seed(26)
    P = 26
    if n == "wrap":  # more tiles than blocks, on the three trees of P = 2
        n, P = geo["grid_cap"] * tile + 1, 2
    elif isinstance(n, str):
        n = {"tile-1": tile - 1, "tile+1": tile + 1}[n]
    trees, w, planes = forest(P, g)
    check(monkeypatch, S.special_x(n, 6, S.INT_POOL, g), trees, w, planes, P)


@pytest.mark.parametrize("ratio", [1.0, 0.5])
@pytest.mark.parametrize("k", [3, 26])
def test_gbm_classifier_predict_raw(monkeypatch, k, ratio):
    frame = synthetic_classification(3000, 12, k=k, seed=5, device="cuda")
    model = (sea.GBMClassifier().setLoss("logloss").setNumBaseLearners(3)
             .setBaseLearner(sea.DecisionTreeRegressor().setMaxDepth(4))
             .setSubspaceRatio(ratio).setSeed(4).fit(frame))
    x = frame["features"].float()
    ops.last_forest_margin_info.clear()
    raw = model.predictRaw(x)
    assert ops.last_forest_margin_info["path"] == "native"
    assert ops.last_forest_margin_info["planes"] == k
    assert "_pack_caches" not in model.__dict__
    # the per-class forest_predict2 route: one group per class, a fixed order
    monkeypatch.setenv("SEA_MARGIN_FUSED", "0")
    assert torch.equal(raw, model.predictRaw(x))
    assert ops.last_forest_margin_info["path"] == "reference"
    monkeypatch.delenv("SEA_MARGIN_FUSED")

    # a stage that is not a tree: the loop over the members serves the model
    const = DummyRegressionModel()
    const._constant = 0.25
    model._models[1][0] = const
    ops.last_forest_margin_info.clear()
    got = model.predictRaw(x).cpu().double()
    assert ops.last_forest_margin_info.get("path") != "native"
    want = model._init.predictRaw(x)[:, :k].cpu().double()
    mass = want.abs()
    for ms, wts, sub in zip(model._models, model._weights, model._subspaces):
        xs = slice_features(x, sub)
        for j, m in enumerate(ms):
            term = float(wts[j]) * m.predict(xs).cpu().double()
            want[:, j] += term
            mass[:, j] += term.abs()
    # per element three f32 products (weight and product rounded) and three
    # f32 adds of partial sums within `mass`: at most 5 * 2**-24 * mass
    # (a class without rows has a log-prior of -inf: equal, no ratio)
    fin = want.isfinite()
    assert torch.equal(got[~fin], want[~fin])
    ratio = (got - want)[fin].abs() / (2.0 ** -24 * mass[fin])
    print("member loop: max err / (2**-24 * mass)", float(ratio.max()))
    assert bool((ratio <= 8).all())


def test_wide_inputs_keep_the_per_class_route(monkeypatch):
    frame = synthetic_classification(2000, 20, k=3, seed=6, device="cuda")
    model = sea.GBMClassifier().setLoss("logloss").setNumBaseLearners(2).fit(frame)
    x = frame["features"].float()
    ops.last_forest_margin_info.clear()
    raw = model.predictRaw(x)  # 20 > MARGIN_FUSED_MAX_FEATURES
    assert not ops.last_forest_margin_info and "_pack_caches" in model.__dict__
    monkeypatch.setenv("SEA_MARGIN_FUSED", "1")
    assert torch.equal(raw, model.predictRaw(x))
    assert ops.last_forest_margin_info["path"] == "native"


def test_declines(monkeypatch):
    g = torch.Generator().manual_seed(9)
    trees, w, planes = forest(9, g)
    x = S.special_x(100, 6, S.INT_POOL, g).cuda()
    dev = S.to_dev(trees, "cuda")
    with pytest.raises(ValueError):  # a split on feature >= F
        ops.forest_margin(x[:, :3].contiguous(), dev, w, planes, 9)
    big = dev + S.to_dev(
        [S.sized_tree(ops._FP2_GROUP_NODES + 1, 6, 1, g, S.INT_POOL)], "cuda")
    w1, p1 = torch.cat([w, torch.ones(1)]), planes + [0]
    assert ops.forest_margin(x, big, w1, p1, 9, native_only=True) is None
    got = ops.forest_margin(x, big, w1, p1, 9)
    assert ops.last_forest_margin_info["path"] == "reference"
    assert torch.equal(got.cpu().double(), expected(x.cpu(), big, w1, p1, 9))
