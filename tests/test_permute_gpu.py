"""forest_permute_loss on the GPU (csrc/forest_permute.hip) against the
float64 reference op on the CPU: ``torch.equal`` on integer-leaf forests
under the squared loss, the project's per-row-loss rule for the other eight
losses, routing asserted on ``last_forest_permute_info``, and the model-level
interface on the native route.  Shapes are sized from
``forest_permute_geometry()``."""

import functools

import pytest
import torch

import permute_util as pu
import serving_util as su
import spark_ensemble_amd as sea
from spark_ensemble_amd.boosting.losses import (
    BernoulliLoss, HuberLoss, SquaredLoss, get_classification_loss)
from spark_ensemble_amd.frame import TensorFrame
from spark_ensemble_amd.ops import dispatch
from spark_ensemble_amd.utils.io import (
    synthetic_classification, synthetic_regression)

pytestmark = pytest.mark.gpu

DEV = "cuda"


@functools.lru_cache(maxsize=None)
def geom():
    threads, rpl, max_blocks, fc, budget, max_depth = \
        dispatch.forest_permute_geometry()
    assert rpl == 1 and threads % 64 == 0 and 1 <= fc <= 64
    assert threads * fc * 4 + budget * 8 <= 163840
    return threads, max_blocks, fc, budget, max_depth


def info():
    return dict(dispatch.last_forest_permute_info)


def run_native(args, mode=None, groups=None, cache=None):
    got = pu.run_op(args, DEV, cache=cache)
    i = info()
    assert i["path"] == "native", i
    assert i["feature_chunk"] == geom()[2]
    if mode is not None:
        assert i["mode"] == mode, i
    if groups is not None:
        assert i["groups"] == groups, i
    return got


# ---- exact: rows and repeats ------------------------------------------------

def _row_counts():
    return ["1", "63", "64", "65", "tile-1", "tile", "tile+1"]


@pytest.mark.parametrize("n_name", _row_counts())
@pytest.mark.parametrize("R", [1, 3])
def test_rows_and_repeats(n_name, R):
    tile = geom()[0]
    N = eval(n_name, {"tile": tile})
    args = pu.forest_case(20 + R, N, 5, 6, R=R)
    pu.check_exact(run_native(args, mode="binned", groups=1), args)


def test_grid_wrap():
    tile, max_blocks = geom()[:2]
    N = (max_blocks + 3) * tile + 5  # blocks 0 .. 3 take a second tile
    args = pu.forest_case(31, N, 2, 2, depth=3, R=1)
    pu.check_exact(run_native(args), args)


# ---- exact: feature chunks --------------------------------------------------

@pytest.mark.parametrize("f_name", ["1", "FC-1", "FC", "FC+1", "2*FC+1"])
def test_feature_chunks(f_name):
    F = max(eval(f_name, {"FC": geom()[2]}), 1)
    args = pu.forest_case(40, 300, F, 8, R=1)
    pu.check_exact(run_native(args), args)


def test_last_chunk_only_and_unused_columns():
    fc = geom()[2]
    F = 2 * fc + 3
    used = [2 * fc, 2 * fc + 1, 2 * fc + 2]
    args = pu.forest_case(41, 300, F, 8, R=2, used=used)
    base, perm = run_native(args)
    pu.check_exact((base, perm), args)
    assert torch.equal(perm[:, :2 * fc], base.expand(2, 2 * fc))
    assert not torch.equal(perm[:, 2 * fc:], base.expand(2, 3))


# ---- exact: LDS groups ------------------------------------------------------

def _group_forest(n_big, leaf_at=None):
    budget = geom()[3]
    n = (budget // 2 - 1) | 1  # two of them fill a group, three do not fit
    g = torch.Generator().manual_seed(50 + n_big)
    trees = [su.sized_tree(n, 6, 1, g, su.INT_POOL) for _ in range(n_big)]
    if leaf_at is not None:
        trees.insert(leaf_at, su.leaf_tree())
    weights = su.rand_weights(len(trees), g)
    x = su.special_x(300, 6, su.INT_POOL, g)
    return pu.exact_args(trees, weights, x, 2, seed=n_big)


def test_two_groups():
    args = _group_forest(3)
    pu.check_exact(run_native(args, groups=2), args)


def test_three_groups_with_a_leaf_tree_in_the_middle():
    args = _group_forest(5, leaf_at=2)
    pu.check_exact(run_native(args, groups=3), args)


def test_leaves_only_forest_takes_raw_mode(monkeypatch):
    g = torch.Generator().manual_seed(3)
    trees = [su.leaf_tree(value=v) for v in (7.0, -3.0, 2.0)]
    x = su.special_x(200, 4, su.INT_POOL, g)
    args = pu.exact_args(trees, [0.5, 1.0, 2.0], x, 2)
    base, perm = run_native(args, mode="raw")
    pu.check_exact((base, perm), args)
    assert torch.equal(perm, base.expand(2, 4))
    monkeypatch.setenv("SEA_PERMUTE_MODE", "binned")
    with pytest.raises(ValueError, match="no u8 rank form"):
        pu.run_op(args, DEV)


# ---- exact: paths and donors ------------------------------------------------

TWICE_X = torch.tensor(
    [[-3.0, -1.0], [-1.0, -1.0], [3.0, 5.0], [1.0, 0.0],
     [float("nan"), 1.0], [float("inf"), -1.0],
     [float("-inf"), float("nan")]])


@pytest.mark.parametrize("mode", ["binned", "raw"])
@pytest.mark.parametrize("donor", [
    [2, 1, 2, 0, 0, 1, 4],   # row 0: the donor disagrees at both x0 nodes
    [1, 1, 2, 2, 5, 6, 3],   # row 0: agrees at the root, disagrees below
    [3, 3, 3, 3, 3, 3, 3],   # x0 = 1: the sub-walk meets x0 again at node 2
    [4, 5, 6, 4, 3, 4, 5],   # NaN and +-inf as donor values
])
def test_path_splits_twice_on_one_feature(mode, donor, monkeypatch):
    monkeypatch.setenv("SEA_PERMUTE_MODE", mode)
    trees = [pu.twice_tree(), su.leaf_tree(), pu.twice_tree()]
    args = pu.exact_args(trees, [1.0, 2.0, 0.5], TWICE_X, 1,
                         donor=torch.tensor([donor]))
    got = run_native(args, mode=mode)
    pu.check_exact(got, args)
    pu.check_exact(got, args, want=pu.oracle64(args))


def test_identity_donors():
    args = pu.forest_case(60, 333, 7, 6, R=1)
    x, trees, weights = args[:3]
    ident = torch.arange(333).expand(3, 333).contiguous()
    a2 = pu.exact_args(trees, weights, x, 3, donor=ident)
    base, perm = run_native(a2)
    assert torch.equal(perm, base.expand(3, 7))
    pu.check_exact((base, perm), a2)


@pytest.mark.parametrize("mode", ["binned", "raw"])
def test_special_values_own_and_donor(mode, monkeypatch):
    monkeypatch.setenv("SEA_PERMUTE_MODE", mode)
    args = pu.forest_case(61, 700, 6, 8, depth=5, R=2,
                          pool=su.SPECIALS_POOL)
    x = args[0]
    assert bool(x.isnan().any()) and bool(x.isinf().any())
    pu.check_exact(run_native(args, mode=mode), args)


# ---- routing ----------------------------------------------------------------

def test_depth_cap():
    """Depth at the cap is native and one beyond is the reference route;
    without a cap (max_depth == 0) a chain far deeper than any register
    list would hold stays native (60 levels: the reference walk stops at
    64)."""
    max_depth = geom()[4]
    g = torch.Generator().manual_seed(5)
    x = su.special_x(200, 3, su.INT_POOL, g)
    for depth in ([max_depth, max_depth + 1] if max_depth else [60]):
        trees = [pu.chain_tree(depth, 3), pu.chain_tree(3, 3)]
        args = pu.exact_args(trees, [1.0, 2.0], x, 2)
        got = pu.run_op(args, DEV)
        want = "reference" if max_depth and depth > max_depth else "native"
        assert info()["path"] == want
        pu.check_exact(got, args)


def test_tree_over_the_group_budget_takes_the_reference_route():
    budget = geom()[3]
    g = torch.Generator().manual_seed(6)
    x = su.special_x(100, 4, su.INT_POOL, g)
    fits = [su.sized_tree(budget - 1 | 1, 4, 1, g, su.INT_POOL)]
    args = pu.exact_args(fits, [1.0], x, 1)
    pu.check_exact(run_native(args, groups=1), args)
    over = [su.sized_tree((budget + 1) | 1, 4, 1, g, su.INT_POOL)]
    args = pu.exact_args(over, [1.0], x, 1)
    got = pu.run_op(args, DEV)
    assert info()["path"] == "reference"
    pu.check_exact(got, args)


def test_vector_leaves_and_custom_loss_take_the_reference_route():
    g = torch.Generator().manual_seed(7)
    x = su.special_x(100, 4, su.INT_POOL, g)
    trees2 = [su.rand_tree(3, 4, 2, g, su.INT_POOL) for _ in range(3)]
    args = pu.exact_args(trees2, [1.0, 0.5, 2.0], x, 1)
    got = pu.run_op(args, DEV)
    assert info()["path"] == "reference"
    pu.check_exact(got, args)

    class MySquared(SquaredLoss):
        pass

    args = list(pu.forest_case(8, 100, 4, 3))
    args[6] = MySquared()
    got = pu.run_op(tuple(args), DEV)
    assert info()["path"] == "reference"
    pu.check_exact(got, tuple(args))


def test_more_than_255_thresholds_takes_raw_mode():
    g = torch.Generator().manual_seed(9)
    # 511 splits on feature 0 with cuts drawn from 600 values, depth 9
    tree = su.sized_tree(1023, 1, 1, g, torch.arange(600.0))
    cuts = tree["threshold"][tree["feature"] >= 0]
    assert cuts.unique().numel() > 255
    x = torch.randint(-5, 620, (400, 2), generator=g).float()
    args = pu.exact_args([tree, pu.twice_tree()], [1.0, 0.5], x, 2)
    pu.check_exact(run_native(args, mode="raw"), args)


def test_non_contiguous_x():
    args = list(pu.forest_case(62, 300, 10, 6, R=2))
    wide = torch.zeros(300, 20)
    wide[:, ::2] = args[0]
    x = wide.to(DEV)[:, ::2]
    assert not x.is_contiguous()
    trees, weights, init, label, w, loss, donor = args[1:]
    base, perm = dispatch.forest_permute_loss(
        x, su.to_dev(trees, DEV), weights, init, label, w, loss, donor)
    assert info()["path"] == "native"
    pu.check_exact((base.cpu(), perm.cpu()), tuple(args))


def test_cache_reuse_and_reproducible_bits():
    args = pu.toleranced_case(63, 900, geom()[2] + 3, 10, "logcosh")
    cache = {}
    first = run_native(args, cache=cache)
    pack = cache["pack"]
    second = run_native(args, cache=cache)
    assert cache["pack"] is pack
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1])
    third = run_native(args)  # no cache: a fresh pack, the same bits
    assert torch.equal(first[1], third[1])


def test_argument_errors():
    x, trees, weights, init, label, w, loss, donor = \
        pu.forest_case(6, 10, 3, 2, R=2)
    xd, td = x.to(DEV), su.to_dev(trees, DEV)

    def call(xx, dn):
        return dispatch.forest_permute_loss(
            xx, td, weights, init, label, w, loss, dn)

    with pytest.raises(ValueError, match="donor is"):
        call(xd, donor[:, :9])
    bad = donor.clone()
    bad[0, 0] = 10
    with pytest.raises(ValueError, match="outside"):
        call(xd, bad)
    f_max = max(int(t["feature"].max()) for t in trees)
    with pytest.raises(ValueError, match="splits on feature"):
        call(xd[:, :f_max].contiguous(), donor)
    base, perm = call(xd[:0], donor[:, :0])
    assert float(base) == 0.0 and perm.shape == (2, 3) and perm.is_cuda


# ---- toleranced: the other eight losses -------------------------------------

@pytest.mark.parametrize("name", pu.OTHER_LOSSES)
def test_other_losses(name):
    args = pu.toleranced_case(70, 777, geom()[2] + 3, 10, name)
    pu.check_tol(run_native(args), args, label=name)


# ---- model level ------------------------------------------------------------

def _frame(df, **extra):
    cols = {k: df[k].to(DEV) for k in ("features", "label")}
    cols.update({k: v.to(DEV) for k, v in extra.items()})
    return TensorFrame(**cols)


def _check_native(model, df, loss, margins, call_loss=None, weight=None,
                  label=""):
    dispatch.last_forest_permute_info.clear()
    res = model.permutationImportance(df, numRepeats=2, seed=1,
                                      loss=call_loss)
    assert info().get("path") == "native", info()
    want = pu.brute_force_model(model, df, loss, margins, 2, 1, weight)
    pu.check_model(res, want, label)
    return res


def test_gbm_regressor_squared_huber_and_weights():
    df = _frame(synthetic_regression(1500, 6, seed=0))
    m = (sea.GBMRegressor().setNumBaseLearners(5)
         .setBaseLearner(sea.DecisionTreeRegressor().setMaxDepth(4)).fit(df))
    mg = lambda x: m.predict(x).unsqueeze(1)  # noqa: E731
    res = _check_native(m, df, SquaredLoss(), mg, label="gbm squared")
    _check_native(m, df, HuberLoss(0.7), mg, call_loss=HuberLoss(0.7),
                  label="gbm huber")
    again = m.permutationImportance(df, numRepeats=2, seed=1)
    assert torch.equal(again.importances, res.importances)
    other = m.permutationImportance(df, numRepeats=2, seed=2)
    assert not torch.equal(other.importances, res.importances)
    one = m.permutationImportance(df, numRepeats=1, seed=1)
    assert one.importances.shape == (1, 6) and not bool(one.std.any())

    g = torch.Generator().manual_seed(5)
    wt = (0.25 + torch.rand(1500, generator=g)).to(DEV)
    dfw = TensorFrame(features=df["features"], label=df["label"], w=wt)
    mw = (sea.GBMRegressor().setNumBaseLearners(3).setWeightCol("w")
          .setBaseLearner(sea.DecisionTreeRegressor().setMaxDepth(3))
          .fit(dfw))
    _check_native(mw, dfw, SquaredLoss(),
                  lambda x: mw.predict(x).unsqueeze(1), weight=wt,
                  label="gbm weighted")


def test_gbm_classifier_bernoulli():
    df = _frame(synthetic_classification(1500, 6, k=2, seed=1))
    m = (sea.GBMClassifier().setLoss("bernoulli").setNumBaseLearners(4)
         .fit(df))
    _check_native(m, df, BernoulliLoss(), lambda x: m._margins(x),
                  label="gbm bernoulli")


def test_bagging_subspace_and_tree():
    df = _frame(synthetic_regression(1500, 8, seed=0))
    m = (sea.BaggingRegressor().setNumBaseLearners(4).setSubspaceRatio(0.4)
         .setBaseLearner(sea.DecisionTreeRegressor().setMaxDepth(3))
         .setSeed(3).fit(df))
    res = _check_native(m, df, SquaredLoss(),
                        lambda x: m.predict(x).unsqueeze(1), label="bagging")
    used = set()
    for sub in m._subspaces:
        used |= set(sub.tolist())
    outside = [f for f in range(8) if f not in used]
    assert outside, "pick a seed that leaves a feature out"
    for f in outside:
        assert not bool(res.importances[:, f].any())  # exactly 0.0
    t = sea.DecisionTreeRegressor().setMaxDepth(4).fit(df)
    _check_native(t, df, SquaredLoss(), lambda x: t.predict(x).unsqueeze(1),
                  label="tree")


def test_generic_routes_do_not_call_the_op(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("fused op called")

    monkeypatch.setattr(dispatch, "forest_permute_loss", boom)
    df3 = _frame(synthetic_classification(600, 5, k=3, seed=2))
    m3 = (sea.GBMClassifier().setLoss("logloss").setNumBaseLearners(2)
          .fit(df3))
    res = m3.permutationImportance(df3, numRepeats=2, seed=1)
    want = pu.brute_force_model(
        m3, df3, get_classification_loss("logloss", 3),
        lambda x: m3._margins(x), 2, 1)
    pu.check_model(res, want, "gbm logloss")

    dfr = _frame(synthetic_regression(600, 5, seed=0))
    mb = (sea.BaggingRegressor().setNumBaseLearners(3)
          .setBaseLearner(sea.LinearRegression()).fit(dfr))
    res = mb.permutationImportance(dfr, numRepeats=2, seed=1)
    want = pu.brute_force_model(
        mb, dfr, SquaredLoss(), lambda x: mb.predict(x).unsqueeze(1), 2, 1)
    pu.check_model(res, want, "bagging linear")


def test_sanity_order():
    cpu = pu.sanity_frame()
    df = _frame(cpu)
    m = (sea.GBMRegressor().setNumBaseLearners(10)
         .setBaseLearner(sea.DecisionTreeRegressor().setMaxDepth(3)).fit(df))
    mean = m.permutationImportance(df, numRepeats=2, seed=0).mean
    assert info()["path"] == "native"
    assert mean[0] > mean[1] > mean[2:].max()
