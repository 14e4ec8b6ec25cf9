"""Out-of-bag estimates on the CPU: the reference op against its own
float64 run, the Bagging models against a brute-force loop over the public
API, the no-leakage experiment, and the edge cases of the model surface.

Exact comparisons are ``torch.equal`` (integer-leaf forests; member sums in
member order, f32, weight 1).  The leakage bounds: with labels independent
of the features a vote of trees that never saw a row is a coin flip, sd
0.008 at n = 4000, so |oobScore - 0.5| <= 0.05 is six of them, while a vote
with in-bag members in it memorises (training accuracy >= 0.85)."""

import json
import math
import os

import pytest
import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.frame import TensorFrame
from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.parallel import get_comm
from spark_ensemble_amd.utils.io import (
    synthetic_classification, synthetic_regression)

import oob_util as U
import serving_util as S


# ---- 1. the reference op ---------------------------------------------------

@pytest.mark.parametrize("T,D", [(1, 1), (31, 1), (33, 3), (65, 1), (40, 8)])
def test_reference_f32_equals_float64(T, D):
    g = torch.Generator().manual_seed(100 + T)
    F = 7
    trees = [S.rand_tree(5, F, D, g, S.SPECIALS_POOL, p_stop=0.2)
             for _ in range(T)]
    x = S.special_x(300, F, S.SPECIALS_POOL, g)
    inbag = U.mask_patterns(300, T, g)
    got = ops.forest_oob(x, trees, inbag)
    assert ops.last_forest_oob_info["path"] == "reference"
    U.check_exact(got, x, trees, inbag, label=f"T={T} D={D}")


def test_reference_multi_group_forest():
    """The exact-fill forest of the serving tests (two LDS groups on the
    GPU) through the reference op."""
    g = torch.Generator().manual_seed(7)
    trees = S.exact_fill_forest(6, 1, g, S.INT_POOL, tail=13)
    x = S.special_x(200, 6, S.INT_POOL, g)
    inbag = U.mask_patterns(200, len(trees), g)
    U.check_exact(ops.forest_oob(x, trees, inbag), x, trees, inbag)


def test_op_argument_errors():
    g = torch.Generator().manual_seed(3)
    trees = [S.rand_tree(3, 5, 1, g, S.INT_POOL) for _ in range(4)]
    x = torch.randn(10, 5)
    with pytest.raises(ValueError):
        ops.forest_oob(x, trees, torch.zeros(10, 3, dtype=torch.bool))
    with pytest.raises(ValueError):
        ops.forest_oob(x, trees, torch.zeros(4, 10, dtype=torch.bool))
    f_max = max(int(t["feature"].max()) for t in trees)
    with pytest.raises(ValueError):
        ops.forest_oob(x[:, :f_max], trees,
                       torch.zeros(10, 4, dtype=torch.bool))
    sums, counts = ops.forest_oob(x[:0], trees,
                                  torch.zeros(0, 4, dtype=torch.bool))
    assert sums.shape == (0, 1) and counts.shape == (0,)


def test_mask_packing_bit_31():
    g = torch.Generator().manual_seed(4)
    inbag = U.mask_patterns(50, 65, g)
    words = ops._pack_inbag(inbag)
    assert words.dtype == torch.int32 and words.shape == (3, 50)
    assert words.is_contiguous()
    for t in range(65):
        bit = (words[t >> 5].long() >> (t & 31)) & 1
        assert torch.equal(bit.bool(), inbag[:, t]), t
    # bits past T are clear
    assert bool(((words[2].long() >> 1) == 0).all())


# ---- 2. brute force --------------------------------------------------------

def _weights(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) + 0.5


@pytest.fixture(scope="module")
def reg():
    return synthetic_regression(1500, 12, seed=17)


@pytest.fixture(scope="module")
def clf():
    return synthetic_classification(1500, 12, k=3, seed=11)


@pytest.mark.parametrize("path", ["fused", "generic_tree", "generic_linear"])
def test_regressor_equals_brute_force(reg, path):
    tree = sea.DecisionTreeRegressor().setMaxDepth(4)
    if path == "generic_tree":
        tree = tree.set("minWeightFractionPerNode", 0.01)
    learner = sea.LinearRegression() if path == "generic_linear" else tree
    est = (sea.BaggingRegressor().setBaseLearner(learner)
           .setNumBaseLearners(6).setSubspaceRatio(0.6).setSeed(5))
    ops.last_forest_oob_info.clear()
    U.check_regressor(est, reg)
    # tree members take the op, anything else the member loop
    assert bool(ops.last_forest_oob_info) == (path != "generic_linear")


@pytest.mark.parametrize("vote", ["hard", "soft"])
@pytest.mark.parametrize("path", ["fused", "generic_tree", "generic_linear"])
def test_classifier_equals_brute_force(clf, path, vote):
    tree = sea.DecisionTreeClassifier().setMaxDepth(4)
    if path == "generic_tree":
        tree = tree.set("minWeightFractionPerNode", 0.01)
    learner = (sea.LogisticRegression().setMaxIter(5)
               if path == "generic_linear" else tree)
    est = (sea.BaggingClassifier().setBaseLearner(learner)
           .setNumBaseLearners(5).setSubspaceRatio(0.6).setSeed(9)
           .setVotingStrategy(vote))
    ops.last_forest_oob_info.clear()
    U.check_classifier(est, clf)
    assert bool(ops.last_forest_oob_info) == (path != "generic_linear")


def test_weighted_fit_and_subsampling_without_replacement(reg):
    w = _weights(reg.count(), 21)
    frame = reg.withColumn("w", w)
    est = (sea.BaggingRegressor().setNumBaseLearners(5).setWeightCol("w")
           .setReplacement(False).setSubsampleRatio(0.7).setSeed(2)
           .setBaseLearner(sea.DecisionTreeRegressor().setMaxDepth(3)))
    U.check_regressor(est, frame, weight=w)


def test_soft_vote_needs_probabilistic_members(clf):
    class Hard:
        def predict(self, xs):
            return torch.zeros(xs.shape[0])

    est = sea.BaggingClassifier().setVotingStrategy("soft")
    x = clf["features"]
    n = x.shape[0]
    with pytest.raises(RuntimeError):
        est._oob_estimates(
            x, clf["label"], torch.ones(n), [Hard()],
            [torch.arange(x.shape[1])], torch.zeros(n, 1, dtype=torch.bool),
            3, get_comm())


# ---- 3. no leakage ---------------------------------------------------------

def test_no_leakage_on_noise_labels():
    train, score, coverage = U.leakage_experiment("cpu")
    print(f"train acc {train:.4f} oob acc {score:.4f} coverage {coverage:.4f}")
    assert train >= 0.85
    assert abs(score - 0.5) <= 0.05
    assert coverage >= 0.97


# ---- 4. edge cases ---------------------------------------------------------

def test_no_row_out_of_bag(reg, clf):
    m = (sea.BaggingRegressor().setNumBaseLearners(3).setReplacement(False)
         .setSubsampleRatio(1.0).setComputeOob(True).fit(reg))
    assert int(m.oobCounts.max()) == 0
    assert math.isnan(m.oobScore) and m.oobCoverage == 0.0
    assert bool(m.oobPrediction.isnan().all())
    c = (sea.BaggingClassifier().setNumBaseLearners(3).setReplacement(False)
         .setSubsampleRatio(1.0).setComputeOob(True).fit(clf))
    assert int(c.oobCounts.max()) == 0
    assert math.isnan(c.oobScore) and c.oobCoverage == 0.0
    assert bool(c.oobProbability.isnan().all())
    assert bool((c.oobRawPrediction == 0).all())


def test_zero_weight_rows(reg):
    n = reg.count()
    w = torch.ones(n)
    w[::7] = 0.0
    k = 5
    est = (sea.BaggingRegressor().setNumBaseLearners(k).setWeightCol("w")
           .setSeed(3).setComputeOob(True))
    m = est.fit(reg.withColumn("w", w))
    assert bool((m.oobCounts[::7] == k).all())
    assert bool(torch.isfinite(m.oobPrediction[::7]).all())
    # the zero-weight rows do not move the score: corrupt their labels
    y = reg["label"].clone()
    y[::7] += 1000.0
    noisy = TensorFrame(features=reg["features"], label=y, w=w)
    m2 = est.fit(noisy)
    assert torch.equal(m2.oobCounts, m.oobCounts)
    assert torch.equal(m2.oobPrediction.nan_to_num(nan=-7.0),
                       m.oobPrediction.nan_to_num(nan=-7.0))
    assert m2.oobScore == m.oobScore and m2.oobCoverage == m.oobCoverage


def _meta(path):
    with open(os.path.join(path, "metadata", "part-00000")) as f:
        return json.loads(f.readline())


@pytest.mark.parametrize("kind", ["reg", "clf"])
def test_unset_gives_none_and_unchanged_metadata(reg, clf, kind, tmp_path):
    est = (sea.BaggingRegressor() if kind == "reg"
           else sea.BaggingClassifier()).setNumBaseLearners(2)
    assert est.getComputeOob() is False
    m = est.fit(reg if kind == "reg" else clf)
    names = ["oobPrediction", "oobCounts", "oobScore", "oobCoverage"]
    if kind == "clf":
        names += ["oobRawPrediction", "oobProbability"]
    for name in names:
        assert getattr(m, name) is None, name
    p = str(tmp_path / "m")
    m.save(p)
    meta = _meta(p)
    assert "oobScore" not in meta and "oobCoverage" not in meta
    assert "computeOob" not in json.dumps(meta)
    loaded = type(m).load(p)
    for name in names:
        assert getattr(loaded, name) is None, name


@pytest.mark.parametrize("kind", ["reg", "clf"])
def test_save_load_round_trips_score_and_coverage(reg, clf, kind, tmp_path):
    est = (sea.BaggingRegressor() if kind == "reg"
           else sea.BaggingClassifier())
    frame = reg if kind == "reg" else clf
    m = est.setNumBaseLearners(4).setComputeOob(True).fit(frame)
    assert 0.0 < m.oobCoverage <= 1.0 and math.isfinite(m.oobScore)
    p = str(tmp_path / "m")
    m.save(p)
    meta = _meta(p)
    assert meta["oobScore"] == m.oobScore
    assert meta["oobCoverage"] == m.oobCoverage
    loaded = type(m).load(p)
    assert loaded.oobScore == m.oobScore
    assert loaded.oobCoverage == m.oobCoverage
    # the per-row tensors are training-set-sized and are not saved
    assert loaded.oobPrediction is None and loaded.oobCounts is None
    x = frame["features"]
    assert torch.equal(loaded.predict(x), m.predict(x))


def test_nan_score_round_trips(reg, tmp_path):
    m = (sea.BaggingRegressor().setNumBaseLearners(2).setReplacement(False)
         .setSubsampleRatio(1.0).setComputeOob(True).fit(reg))
    p = str(tmp_path / "m")
    m.save(p)
    loaded = sea.BaggingRegressionModel.load(p)
    assert math.isnan(loaded.oobScore) and loaded.oobCoverage == 0.0


def test_copy_and_estimator_persistence_carry_the_param(tmp_path):
    for est in (sea.BaggingRegressor(), sea.BaggingClassifier()):
        est.setComputeOob(True)
        assert est.copy().getComputeOob() is True
        assert est.copy({"computeOob": False}).getComputeOob() is False
        p = str(tmp_path / type(est).__name__)
        est.save(p)
        assert type(est).load(p).getComputeOob() is True
        with pytest.raises(ValueError):
            est.setComputeOob(1)


def test_stacking_fold_fits_compute_no_oob(reg):
    est = sea.BaggingRegressor().setNumBaseLearners(2).setComputeOob(True)
    fold = torch.arange(reg.count()) % 2
    for m in est._fit_folds(reg, fold, 2):
        assert m.oobScore is None and m.oobCounts is None
