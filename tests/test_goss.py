"""GOSS on the CPU: ``reference.goss_weights`` against first principles, and
the wiring of ``sampling="goss"`` through the GBM estimators.

``check_one_round`` is shared with tests/test_goss_gpu.py, which runs it on the
device."""

import math

import numpy as np
import pytest
import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.boosting.losses import get_regression_loss
from spark_ensemble_amd.frame import TensorFrame
from spark_ensemble_amd.models.dummy import DummyRegressor
from spark_ensemble_amd.ops import dispatch as ops

RATES = [(0.2, 0.1), (0.5, 0.5), (0.01, 0.9)]


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("top,other", RATES)
def test_reference_first_principles(d, top, other):
    n = 200_000
    gen = torch.Generator().manual_seed(d)
    g = torch.randn(n, d, generator=gen)
    g[::3] = g[1::3][: g[::3].shape[0]]  # tie groups across the threshold
    w = torch.rand(n, generator=gen) + 0.5
    w[::3] = w[1::3][: w[::3].shape[0]]
    m = ops.goss_weights(g, w, top, other, seed=7).numpy()

    s = np.abs(g.numpy()[:, 0])
    for c in range(1, d):
        s = s + np.abs(g.numpy()[:, c])
    key = (s * w.numpy()).view(np.uint32) & np.uint32(0x7FFFFFFF)
    k = math.ceil(top * n)
    kept = np.argsort(-key.astype(np.int64), kind="stable")[:k]
    assert (m[kept] == 1.0).all()

    rest = np.delete(m, kept)
    amp = np.float32((1.0 - top) / other)
    drawn = int((rest == amp).sum())
    assert drawn + int((rest == 0.0).sum()) == rest.size
    p = other / (1.0 - top)
    assert abs(drawn - rest.size * p) <= 6 * math.sqrt(rest.size * p * (1 - p))


def check_one_round(device):
    """A one-round squared-loss GOSS fit is the init plus the base tree fitted
    by hand on (-g, goss_weights(g, w) * w)."""
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(3000, 5, generator=gen).to(device)
    y = (x[:, 0] * 2 + x[:, 1] ** 2 + torch.randn(3000, generator=gen).to(device))
    w = (torch.rand(3000, generator=gen) + 0.5).to(device)
    df = TensorFrame(features=x, label=y, weight=w)
    est = (sea.GBMRegressor().setWeightCol("weight").setNumBaseLearners(1)
           .setSampling("goss").setTopRate(0.3).setOtherRate(0.2).setSeed(5)
           .setOptimizedWeights(False).setLearningRate(1.0))
    got = est.fit(df).predict(x)

    init = DummyRegressor().setStrategy("mean").fit(df).predict(x)
    g, _ = get_regression_loss("squared").grad_hess_fused(
        y.unsqueeze(1), init.unsqueeze(1), want_hess=False)
    bag = ops.goss_weights(g, w, 0.3, 0.2, 5, 0)
    assert 0 < int((bag == 0).sum()) and (bag.max() > 1)
    tree = sea.DecisionTreeRegressor().setWeightCol("weight").fit(
        TensorFrame(features=x, label=-g.squeeze(1), weight=bag * w))
    assert torch.equal(got, init + tree.predict(x))


def test_one_round_fit_cpu():
    check_one_round("cpu")


@pytest.mark.parametrize("cls", [sea.GBMRegressor, sea.GBMClassifier])
def test_params_roundtrip_and_errors(cls, tmp_path):
    est = cls().setSampling("goss").setTopRate(0.25).setOtherRate(0.125)
    est.save(str(tmp_path / "e"))
    back = cls.load(str(tmp_path / "e"))
    assert [back.getOrDefault(p) for p in ("sampling", "topRate", "otherRate")
            ] == ["goss", 0.25, 0.125]

    gen = torch.Generator().manual_seed(0)
    df = TensorFrame(features=torch.randn(50, 2, generator=gen),
                     label=torch.randint(0, 2, (50,), generator=gen).float())
    for bad in (cls().setSampling("goss").setTopRate(0.6).setOtherRate(0.5),
                cls().setSampling("goss").setSubsampleRatio(0.5),
                cls().setSampling("goss").setReplacement(True)):
        with pytest.raises(ValueError):
            bad.fit(df)
