"""The gfx950 forest_oob kernel against the reference op on the CPU, and the
out-of-bag estimates of the Bagging models on the GPU.

Every comparison is ``torch.equal``: integer-leaf forests (tests/
serving_util.py), sums in tree order, so the f32 reference, its float64 run
and the kernel agree bit for bit (tests/oob_util.py: check_exact).  Shapes
come from ``forest_oob_geometry()``."""

import pytest
import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.utils.io import (
    synthetic_classification, synthetic_regression)

import oob_util as U
import serving_util as S

pytestmark = pytest.mark.gpu


def geometry():
    threads, rows_per_lane, max_blocks = ops._load_hip().forest_oob_geometry()
    return threads * rows_per_lane, max_blocks


def run(x, trees, inbag, expect="native", label="", cache=None):
    got = ops.forest_oob(x.cuda(), trees, inbag, cache=cache)
    torch.cuda.synchronize()
    info = dict(ops.last_forest_oob_info)
    assert info["path"] == expect, info
    assert got[0].is_cuda and got[1].is_cuda
    U.check_exact(got, x, trees, inbag, label=f"{label} {info['mode']}")
    return got, info


def case(seed, n, T, D=1, F=7, depth=5, pool=S.SPECIALS_POOL):
    g = torch.Generator().manual_seed(seed)
    trees = [S.rand_tree(depth, F, D, g, pool, p_stop=0.2) for _ in range(T)]
    return S.special_x(n, F, pool, g), trees, U.mask_patterns(n, T, g)


# ---- the op ----------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, "tile-1", "tile", "tile+1"])
def test_row_counts(n):
    tile, _ = geometry()
    if isinstance(n, str):
        n = tile + {"tile-1": -1, "tile": 0, "tile+1": 1}[n]
    _, info = run(*case(n, n, 35), label="rows")
    threads, rows_per_lane, _ = ops._load_hip().forest_oob_geometry()
    assert info["rows_per_lane"] == rows_per_lane
    assert threads * rows_per_lane == tile


def test_row_count_wraps_the_grid():
    tile, max_blocks = geometry()
    n = max_blocks * tile + 1
    run(*case(7, n, 3, F=4, depth=3), label="grid wrap")


@pytest.mark.parametrize("T", [1, 31, 32, 33, 64, 65])
def test_tree_counts(T):
    run(*case(20 + T, 300, T), label="trees")


@pytest.mark.parametrize("D", [1, 2, 3, 8])
def test_leaf_widths(D):
    got, _ = run(*case(40 + D, 300, 37, D=D), label="D")
    assert got[0].shape == (300, D)


def test_leaf_width_nine_routes_to_reference():
    run(*case(49, 130, 5, D=9), expect="reference", label="D 9")


@pytest.mark.parametrize("D", [1, 3])
def test_group_boundary_inside_word_0(D):
    """20 trees fill the first LDS group exactly, 13 more follow: two
    groups, the second starting at tree 20."""
    g = torch.Generator().manual_seed(50 + D)
    trees = S.exact_fill_forest(6, D, g, S.INT_POOL, tail=13)
    x = S.special_x(300, 6, S.INT_POOL, g)
    inbag = U.mask_patterns(300, len(trees), g)
    cache = {}
    _, info = run(x, trees, inbag, label="2 groups", cache=cache)
    groups = cache["pack"]["groups_t"].cpu()
    assert info["groups"] == groups.shape[0] == 2
    assert groups[:, 0].tolist() == [0, 20]


def test_group_boundary_inside_word_1():
    """Two exactly filled groups and a tail: boundaries at trees 20 (mask
    word 0) and 40 (mask word 1)."""
    g = torch.Generator().manual_seed(53)
    trees = (S.exact_fill_forest(6, 1, g, S.INT_POOL, tail=0)
             + S.exact_fill_forest(6, 1, g, S.INT_POOL, tail=5))
    x = S.special_x(300, 6, S.INT_POOL, g)
    inbag = U.mask_patterns(300, len(trees), g)
    cache = {}
    _, info = run(x, trees, inbag, label="3 groups", cache=cache)
    groups = cache["pack"]["groups_t"].cpu()
    assert info["groups"] == groups.shape[0] == 3
    assert groups[:, 0].tolist() == [0, 20, 40]


@pytest.mark.parametrize("mode", ["raw", "binned"])
@pytest.mark.parametrize("D", [1, 3])
def test_walk_modes(mode, D, monkeypatch):
    """NaN, +-inf and ties with every threshold, in both row forms."""
    monkeypatch.setenv("SEA_OOB_MODE", mode)
    _, info = run(*case(60 + D, 700, 40, D=D, F=9, depth=6), label="mode")
    assert info["mode"] == mode


def test_default_walk_mode_is_binned():
    _, info = run(*case(63, 200, 5), label="default mode")
    assert info["mode"] == "binned"


def test_many_thresholds_take_raw(monkeypatch):
    """One feature with more than 255 distinct thresholds has no u8 rank."""
    g = torch.Generator().manual_seed(64)
    pool = torch.arange(300, dtype=torch.float32)
    trees = [S.complete_tree(9, 1, 1, g, pool) for _ in range(4)]
    thr = torch.cat([t["threshold"][t["feature"] >= 0] for t in trees])
    assert thr.unique().numel() > 255
    x = S.special_x(500, 1, pool, g)
    inbag = U.mask_patterns(500, 4, g)
    cache = {}
    _, info = run(x, trees, inbag, label=">255", cache=cache)
    assert info["mode"] == "raw" and not cache["pack"].get("binned_ok")
    monkeypatch.setenv("SEA_OOB_MODE", "binned")
    with pytest.raises(ValueError):
        ops.forest_oob(x.cuda(), trees, inbag, cache=cache)


def test_oversize_tree_routes_to_reference():
    g = torch.Generator().manual_seed(65)
    big = S.sized_tree(ops._FP2_GROUP_NODES + 1, 6, 1, g, S.INT_POOL)
    trees = [S.rand_tree(4, 6, 1, g, S.INT_POOL), big]
    x = S.special_x(200, 6, S.INT_POOL, g)
    run(x, trees, U.mask_patterns(200, 2, g), expect="reference",
        label="oversize")


def test_calling_contract():
    x, trees, inbag = case(66, 9000, 37, D=3, F=9)
    g = torch.Generator().manual_seed(67)
    wide = torch.randn(9000, 18, generator=g)
    wide[:, ::2] = x
    xs = wide.cuda()[:, ::2]
    assert not xs.is_contiguous()
    cache = {}
    first = ops.forest_oob(xs, trees, inbag, cache=cache)
    assert ops.last_forest_oob_info["path"] == "native"
    U.check_exact(first, x, trees, inbag, label="non-contiguous")
    pack = cache["pack"]
    for _ in range(2):
        again = ops.forest_oob(xs, trees, inbag.cuda(), cache=cache)
        assert cache["pack"] is pack
        assert torch.equal(again[0], first[0])
        assert torch.equal(again[1], first[1])


def test_weighted_pack_in_the_cache_is_not_used():
    """A cache dict that forest_predict filled with a weighted pack of the
    same forest: forest_oob packs for itself and leaves that pack alone."""
    x, trees, inbag = case(69, 300, 9)
    cache = {}
    w = torch.full((9,), 0.5)
    ops.forest_predict(x.cuda(), trees, w, cache=cache)
    theirs = cache["pack"]
    run(x, trees, inbag, label="shared cache", cache=cache)
    assert cache["pack"] is theirs


def test_argument_errors_and_empty_input():
    x, trees, inbag = case(68, 50, 4)
    xd = x.cuda()
    with pytest.raises(ValueError):
        ops.forest_oob(xd, trees, inbag[:, :3])
    f_max = max(int(t["feature"].max()) for t in trees)
    with pytest.raises(ValueError):
        ops.forest_oob(xd[:, :f_max], trees, inbag)
    sums, counts = ops.forest_oob(xd[:0], trees, inbag[:0])
    assert sums.shape == (0, 1) and counts.shape == (0,) and sums.is_cuda


# ---- estimator level -------------------------------------------------------

@pytest.mark.parametrize("path", ["fused", "generic_tree", "generic_linear"])
def test_regressor_equals_brute_force(path):
    reg = synthetic_regression(1500, 12, seed=17, device="cuda")
    tree = sea.DecisionTreeRegressor().setMaxDepth(4)
    if path == "generic_tree":
        tree = tree.set("minWeightFractionPerNode", 0.01)
    learner = sea.LinearRegression() if path == "generic_linear" else tree
    est = (sea.BaggingRegressor().setBaseLearner(learner)
           .setNumBaseLearners(6).setSubspaceRatio(0.6).setSeed(5))
    ops.last_forest_oob_info.clear()
    m = U.check_regressor(est, reg)
    assert m.oobPrediction.is_cuda
    if path == "generic_linear":
        assert not ops.last_forest_oob_info
    else:
        assert ops.last_forest_oob_info["path"] == "native"


@pytest.mark.parametrize("vote", ["hard", "soft"])
@pytest.mark.parametrize("path", ["fused", "generic_tree", "generic_linear"])
def test_classifier_equals_brute_force(path, vote):
    clf = synthetic_classification(1500, 12, k=3, seed=11, device="cuda")
    tree = sea.DecisionTreeClassifier().setMaxDepth(4)
    if path == "generic_tree":
        tree = tree.set("minWeightFractionPerNode", 0.01)
    learner = (sea.LogisticRegression().setMaxIter(5)
               if path == "generic_linear" else tree)
    est = (sea.BaggingClassifier().setBaseLearner(learner)
           .setNumBaseLearners(5).setSubspaceRatio(0.6).setSeed(9)
           .setVotingStrategy(vote))
    ops.last_forest_oob_info.clear()
    m = U.check_classifier(est, clf)
    assert m.oobRawPrediction.is_cuda
    if path == "generic_linear":
        assert not ops.last_forest_oob_info
    else:
        assert ops.last_forest_oob_info["path"] == "native"


def test_no_leakage_on_noise_labels():
    train, score, coverage = U.leakage_experiment("cuda")
    print(f"train acc {train:.4f} oob acc {score:.4f} coverage {coverage:.4f}")
    assert ops.last_forest_oob_info["path"] == "native"
    assert train >= 0.85
    assert abs(score - 0.5) <= 0.05
    assert coverage >= 0.97
