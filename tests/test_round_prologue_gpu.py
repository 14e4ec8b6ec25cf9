"""``gbm_round_prologue`` and the GBM rounds that use it, against the composed
round on the GPU.

The composed round (``reference.gbm_round_prologue`` on GPU tensors: the
``grad_hess`` kernel, negation, ``w *``, ``cat``, ``abs().amax()``; whole
fits: ``SEA_ROUND_FUSED=0``) is the oracle.  The native op does the same f32
operations per row in the same order and a maximum has no rounding, so every
comparison is ``torch.equal``: there are no tolerances.  The extension op is
called with NaN-filled outputs, so a row it never wrote shows up."""

import pytest
import torch

from spark_ensemble_amd.boosting.losses import (
    LOSS_IDS, get_classification_loss, get_regression_loss,
)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN = float("nan")
SCALAR_LOSSES = [nm for nm in LOSS_IDS if nm != "logloss"]
# where bernoulli and exponential saturate or overflow
MARGINS = [0.0, 1e-6, -1e-6, 30.0, -30.0, 100.0, -100.0, 1e4, -1e4]
SMALL_N = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def hip():
    from spark_ensemble_amd.ops import dispatch

    assert dispatch.hip_available(), "HIP extension must be built in-tree"
    return dispatch


def make_loss(name):
    if name in ("exponential", "bernoulli"):
        return get_classification_loss(name, 2)
    return get_regression_loss(name, alpha=0.3, delta=0.5, quantile=0.7)


def make_rows(name, n, unit, seed):
    """Margins cycle through MARGINS with a random one after each cycle;
    labels are +-1 for the classification losses, near the margin's scale
    otherwise (exact ties included: label == margin at every 7th row)."""
    g = torch.Generator().manual_seed(seed)
    m = torch.tensor(MARGINS + [NAN])
    pred = m[torch.arange(n) % len(m)].clone()
    filler = torch.isnan(pred)
    pred[filler] = torch.randn(int(filler.sum()), generator=g) * 3.0
    if name in ("exponential", "bernoulli"):
        label = torch.randint(0, 2, (n,), generator=g).float() * 2.0 - 1.0
    else:
        label = pred + torch.randn(n, generator=g)
        label[::7] = pred[::7]
    if unit:
        weight = torch.ones(n)
    else:
        weight = torch.rand(n, generator=g) + 0.25
        weight[0::5] = 1e-30
        weight[min(1, n - 1)::5] = 1e30
        weight[min(2, n - 1)::5] = 1.0
    return (label.unsqueeze(1).to(DEV), pred.unsqueeze(1).to(DEV),
            weight.to(DEV))


def run_native(hip, label, pred, weight, loss, unit):
    n = pred.shape[0]
    gh = torch.full((n, 2 if unit else 3), NAN, device=DEV)
    grad = torch.full((n,), NAN, device=DEV)
    gmax = torch.full((1,), NAN, device=DEV)
    hip._load_hip().gbm_round_prologue(
        gh, grad, gmax, label, pred, weight, loss.loss_id, float(loss.param),
        unit)
    torch.cuda.synchronize()
    return gh, grad, gmax


def one_past_a_trip(hip):
    threads, blocks = hip.gbm_round_prologue_geometry(1 << 40)
    n = threads * blocks + 1
    assert hip.gbm_round_prologue_geometry(n) == (threads, blocks)
    return n


def check_case(hip, name, n, unit):
    from spark_ensemble_amd.ops import reference

    loss = make_loss(name)
    label, pred, weight = make_rows(name, n, unit, 100 * LOSS_IDS[name] + unit)
    gh0, grad0, gmax0 = reference.gbm_round_prologue(
        label, pred, weight, loss, unit)
    gh, grad, gmax = run_native(hip, label, pred, weight, loss, unit)
    assert not torch.isnan(grad0).any(), "the case is meant to be NaN-free"
    assert torch.equal(grad, grad0)
    assert torch.equal(gh, gh0)
    assert torch.equal(gmax, gmax0)
    # through the wrapper, which allocates the outputs itself
    out = hip.gbm_round_prologue(label, pred, weight, loss, unit)
    assert all(torch.equal(a, b) for a, b in zip(out, (gh0, grad0, gmax0)))


@pytest.mark.parametrize("unit", [True, False], ids=["ones", "weights"])
@pytest.mark.parametrize("n", SMALL_N)
@pytest.mark.parametrize("name", SCALAR_LOSSES)
def test_kernel_matches_composed(hip, name, n, unit):
    check_case(hip, name, n, unit)


@pytest.mark.parametrize("unit", [True, False], ids=["ones", "weights"])
@pytest.mark.parametrize("name", SCALAR_LOSSES)
def test_kernel_second_trip_of_the_stride_loop(hip, name, unit):
    check_case(hip, name, one_past_a_trip(hip), unit)


@pytest.mark.parametrize("unit", [True, False], ids=["ones", "weights"])
@pytest.mark.parametrize("row", [0, 200, 256])
@pytest.mark.parametrize("name", SCALAR_LOSSES)
def test_nan_margin_reaches_the_maximum(hip, name, row, unit):
    """One NaN margin: the maximum is NaN exactly when the composed one is
    (fmaxf alone would drop it), and every other row is untouched."""
    from spark_ensemble_amd.ops import reference

    loss = make_loss(name)
    label, pred, weight = make_rows(name, 257, unit, 7)
    pred[row, 0] = NAN
    gh0, grad0, gmax0 = reference.gbm_round_prologue(
        label, pred, weight, loss, unit)
    gh, grad, gmax = run_native(hip, label, pred, weight, loss, unit)
    assert bool(torch.isnan(gmax[0])) == bool(torch.isnan(gmax0[0]))
    if not torch.isnan(gmax0[0]):  # absolute / quantile: a NaN compares false
        assert torch.equal(gmax, gmax0)
    assert torch.equal(torch.isnan(grad), torch.isnan(grad0))
    keep = ~torch.isnan(grad0)
    assert torch.equal(grad[keep], grad0[keep])
    assert torch.equal(gh[keep], gh0[keep])
    assert torch.equal(torch.isnan(gh), torch.isnan(gh0))


def test_no_rows_no_launch(hip):
    loss = make_loss("bernoulli")
    z = torch.zeros(0, 1, device=DEV)
    for unit in (True, False):
        gh, grad, gmax = hip.gbm_round_prologue(
            z, z, torch.zeros(0, device=DEV), loss, unit)
        assert gh.shape == (0, 2 if unit else 3) and grad.shape == (0,)
        assert gmax.tolist() == [0.0]


# ---- whole fits against SEA_ROUND_FUSED=0 in the same process -------------


def _frame(kind, weights):
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.utils.io import (
        synthetic_classification, synthetic_regression,
    )

    if kind == "clf":
        df = synthetic_classification(3000, 16, k=2, seed=21, device=DEV)
    else:
        df = synthetic_regression(3000, 16, seed=22, device=DEV)
    cols = {"features": df["features"], "label": df["label"]}
    if weights != "none":
        g = torch.Generator().manual_seed(23)
        w = torch.rand(3000, generator=g) * 2.0 + 0.25
        w[::9] = 1.0
        if weights == "zero":
            w[5::11] = 0.0
        cols["weight"] = w.to(DEV)
    return TensorFrame(**cols)


def _estimator(kind, loss, weights, **kw):
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.models import DecisionTreeRegressor

    est = sea.GBMClassifier() if kind == "clf" else sea.GBMRegressor()
    est = (est.setBaseLearner(DecisionTreeRegressor().setMaxDepth(3))
           .setLoss(loss).setNumBaseLearners(5).setSeed(3))
    if weights != "none":
        est = est.setWeightCol("weight")
    if "subsample" in kw:
        est = est.setSubsampleRatio(kw["subsample"])
    if "updates" in kw:
        est = est.setUpdates(kw["updates"])
    return est


def _fit_both(hip, monkeypatch, kind, loss, weights, **kw):
    """[(model, native prologue calls)] under SEA_ROUND_FUSED = 1 and 0.

    The stage-weight search sizes its device chain from the previous search
    of the process (``line_search._CHAIN_K``), and a search that outruns its
    chain finishes on the host in float64, so both fits start from the
    module's initial chain length: same history, same last bits."""
    from spark_ensemble_amd.boosting import line_search

    calls = []
    real = hip.gbm_round_prologue

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(hip, "gbm_round_prologue", spy)
    out = []
    for flag in ("1", "0"):
        monkeypatch.setenv("SEA_ROUND_FUSED", flag)
        line_search._CHAIN_K[0] = 4
        del calls[:]
        model = _estimator(kind, loss, weights, **kw).fit(
            _frame(kind, weights))
        torch.cuda.synchronize()
        out.append((model, len(calls)))
    return out


def _trees(model):
    ms = model._models
    return [m._tree for r in ms for m in (r if isinstance(r, list) else [r])]


def _assert_same_model(a, b):
    ta, tb = _trees(a), _trees(b)
    assert len(ta) == len(tb) == 5
    for x, y in zip(ta, tb):
        for key in ("feature", "threshold", "left_child", "leaf_value"):
            assert torch.equal(x[key], y[key]), key
    assert a._weights == b._weights


@pytest.mark.parametrize("kind,loss,weights", [
    ("clf", "bernoulli", "none"),
    ("clf", "bernoulli", "random"),
    ("reg", "squared", "none"),
    ("reg", "huber", "none"),
    ("reg", "huber", "random"),
])
def test_fused_round_fits_the_same_model(hip, monkeypatch, kind, loss,
                                         weights):
    (fused, n_fused), (composed, n_composed) = _fit_both(
        hip, monkeypatch, kind, loss, weights)
    assert n_fused == 5 and n_composed == 0
    _assert_same_model(fused, composed)
    assert any(int((t["feature"] >= 0).sum()) > 1 for t in _trees(fused))


@pytest.mark.parametrize("kind,loss,weights,kw", [
    ("clf", "bernoulli", "none", {"subsample": 0.5}),
    ("clf", "bernoulli", "none", {"updates": "newton"}),
    ("clf", "bernoulli", "zero", {}),
    ("reg", "squared", "zero", {}),
    ("clf", "logloss", "none", {}),
], ids=["subsample", "newton", "zero-weight-clf", "zero-weight-reg",
        "logloss-dim2"])
def test_ineligible_rounds_keep_the_composed_path(hip, monkeypatch, kind,
                                                  loss, weights, kw):
    (a, n_a), (b, n_b) = _fit_both(hip, monkeypatch, kind, loss, weights,
                                   **kw)
    assert n_a == 0 and n_b == 0
    ta, tb = _trees(a), _trees(b)
    assert len(ta) == len(tb) == (10 if loss == "logloss" else 5)
    for x, y in zip(ta, tb):
        for key in ("feature", "threshold", "left_child", "leaf_value"):
            assert torch.equal(x[key], y[key]), key
    assert a._weights == b._weights
