"""The weighted-quantile rule on the CPU: ``reference.forest_wquantile``
against ``weighted_median`` and a brute force, and ``predictQuantile`` of the
boosting and bagging regressors.

Forests come from tests/serving_util.py: integer leaves make equal member
values common.  Weights are multiples of 1/8, so the float64 sums of the
reference and the f32 sums of ``weighted_median`` are both exact and every
comparison is ``torch.equal``."""

import pytest
import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.ensemble.utils import weighted_median
from spark_ensemble_amd.ops import reference
from spark_ensemble_amd.utils.io import synthetic_regression

import serving_util as S

WEIGHTS = {
    1: [3.0],
    2: [1.0, 1.0],                      # exact half after the first value
    5: [0.125, 2.0, 0.5, 1.375, 3.0],
    8: [1.0] * 8,                       # exact half after the fourth
}


def case(seed, M, n=200, F=5):
    g = torch.Generator().manual_seed(seed)
    trees = [S.rand_tree(4, F, 1, g, S.SPECIALS_POOL, p_stop=0.2)
             for _ in range(M)]
    x = S.special_x(n, F, S.SPECIALS_POOL, g)
    vals = torch.stack([reference.tree_predict(
        x, t["feature"], t["threshold"], t["left_child"], t["leaf_value"],
        64)[:, 0] for t in trees], dim=1)
    return x, trees, vals


def brute(vals, weights, p):
    out = []
    for row in vals.tolist():
        pairs = sorted(zip(row, range(len(row))))  # by (value, member)
        need, cum, hit = p * sum(weights), 0.0, pairs[0][0]
        for v, t in pairs:
            cum += weights[t]
            if cum >= need:
                hit = v
                break
        out.append(hit)
    return torch.tensor(out)


@pytest.mark.parametrize("M", sorted(WEIGHTS))
def test_half_is_the_weighted_median(M):
    x, trees, vals = case(M, M)
    w = torch.tensor(WEIGHTS[M])
    got = reference.forest_wquantile(x, trees, w, [0.5])
    assert got.shape == (x.shape[0], 1)
    assert torch.equal(got[:, 0], weighted_median(vals, w))


@pytest.mark.parametrize("last", [0.0, -1.0])
@pytest.mark.parametrize("p", [0.0, 0.25, 0.5, 1.0])
def test_against_brute_force(p, last):
    x, trees, vals = case(11, 5)
    w = WEIGHTS[5][:4] + [last]
    got = reference.forest_wquantile(x, trees, w, [p])
    assert torch.equal(got[:, 0], brute(vals, w, p))


def test_none_reaches_the_threshold_takes_the_first():
    vals = torch.tensor([[2.0, 1.0]])
    got = reference.weighted_quantile(vals, [0.0, -2.0], [0.5])
    assert got.tolist() == [[1.0]]  # cum = -2, -2 never reaches 0.5 * -2


def test_models():
    df = synthetic_regression(400, 8, seed=3)
    x = df["features"]
    tree = sea.DecisionTreeRegressor().setMaxDepth(3)
    boost = (sea.BoostingRegressor().setBaseLearner(tree)
             .setNumBaseLearners(6).fit(df))
    q = boost.predictQuantile(x, [0.5])
    assert q.shape == (400, 1)
    assert torch.equal(q[:, 0], boost.predict(x))
    bag = (sea.BaggingRegressor().setBaseLearner(tree).setNumBaseLearners(7)
           .setSubspaceRatio(0.6).setSeed(2).fit(df))
    q = bag.predictQuantile(x, [0.0, 0.25, 0.5, 1.0])
    assert q.shape == (400, 4)
    assert bool((q[:, 1:] >= q[:, :-1]).all())
    for m in (boost, bag):
        with pytest.raises(ValueError):
            m.predictQuantile(x, [1.5])
