"""The composed form of the GBM round prologue (ops/reference.py) and the
split of the tree fit statistics, on the CPU.

``reference.gbm_round_prologue`` has to be the expressions the round ran
before, so every comparison is ``torch.equal``."""

import pytest
import torch

from spark_ensemble_amd.boosting.losses import (
    LOSS_IDS, get_classification_loss, get_regression_loss,
)
from spark_ensemble_amd.models import tree as tree_mod
from spark_ensemble_amd.ops import dispatch, reference
from spark_ensemble_amd.parallel import Comm

SCALAR_LOSSES = [nm for nm in LOSS_IDS if nm != "logloss"]


def make_loss(name):
    if name in ("exponential", "bernoulli"):
        return get_classification_loss(name, 2)
    return get_regression_loss(name, alpha=0.3, delta=0.5, quantile=0.7)


def make_rows(name, n, seed):
    g = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, 1, generator=g) * 3.0
    if name in ("exponential", "bernoulli"):
        label = torch.randint(0, 2, (n, 1), generator=g).float() * 2.0 - 1.0
    else:
        label = torch.randn(n, 1, generator=g)
    weight = torch.rand(n, generator=g) + 0.25
    return label, pred, weight


def composed(loss, label, pred, weight, unit):
    g = loss.grad_hess_fused(label, pred, want_hess=False)[0]
    grad = weight * (-g).squeeze(1)
    cols = [grad.unsqueeze(1), weight.unsqueeze(1)]
    if not unit:
        cols.append(torch.ones(len(grad), 1))
    return torch.cat(cols, dim=1), grad, grad.abs().amax().reshape(1)


def test_every_scalar_loss_is_covered():
    assert len(SCALAR_LOSSES) == len(LOSS_IDS) - 1 == 8


@pytest.mark.parametrize("unit", [True, False], ids=["C2", "C3"])
@pytest.mark.parametrize("name", SCALAR_LOSSES)
def test_reference_is_the_composed_round(name, unit):
    loss = make_loss(name)
    label, pred, weight = make_rows(name, 257, LOSS_IDS[name])
    if unit:
        weight = torch.ones_like(weight)
    gh, grad, gmax = reference.gbm_round_prologue(
        label, pred, weight, loss, unit)
    gh0, grad0, gmax0 = composed(loss, label, pred, weight, unit)
    assert gh.shape == (257, 2 if unit else 3) and gh.is_contiguous()
    assert grad.shape == (257,) and gmax.shape == (1,)
    assert torch.equal(gh, gh0)
    assert torch.equal(grad, grad0)
    assert torch.equal(gmax, gmax0)
    # the CPU dispatch is the reference
    out = dispatch.gbm_round_prologue(label, pred, weight, loss, unit)
    assert all(torch.equal(a, b) for a, b in zip(out, (gh, grad, gmax)))


def test_reference_nan_and_empty():
    loss = make_loss("squared")
    label, pred, weight = make_rows("squared", 9, 1)
    pred[4, 0] = float("nan")
    _, grad, gmax = reference.gbm_round_prologue(
        label, pred, weight, loss, False)
    assert torch.isnan(grad[4]) and torch.isnan(gmax[0])
    gh, grad, gmax = reference.gbm_round_prologue(
        label[:0], pred[:0], weight[:0], loss, True)
    assert gh.shape == (0, 2) and grad.shape == (0,)
    assert gmax.tolist() == [0.0]


def _fit_stats_before(grad, w, comm):
    """``models.tree._fused_fit_stats`` as it was before it was split."""
    d = grad.shape[1]
    n = grad.shape[0]
    dev = grad.device
    sums = torch.cat([
        w.sum().reshape(1),
        (w == 0).sum().reshape(1).to(torch.float32),
        (w != 1).sum().reshape(1).to(torch.float32),
        torch.tensor([float(n)], device=dev),
        grad.sum(dim=0).reshape(-1),
    ])
    maxs = torch.cat([
        grad.abs().amax(dim=0).reshape(-1) if n else torch.zeros(d, device=dev),
        w.abs().amax().reshape(1) if n else torch.zeros(1, device=dev),
    ])
    sums_c = sums.cpu()
    maxs_c = maxs.cpu()
    return {
        "total_w": float(sums_c[0]),
        "has_zero": float(sums_c[1]) > 0,
        "all_one": float(sums_c[2]) == 0,
        "n_global": float(sums_c[3]),
        "gsum": sums_c[4:],
        "gmax": maxs_c[:d],
        "hmax": float(maxs_c[d]),
    }


def _same_stats(a, b):
    assert set(a) == set(b)
    for k, v in a.items():
        if torch.is_tensor(v):
            assert torch.equal(v, b[k]), k
        else:
            assert type(v) is type(b[k]) and v == b[k], k


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("kind", ["random", "ones"])
def test_split_fit_stats_match_the_combined_pass(kind, d):
    g = torch.Generator().manual_seed(5 + d)
    n = 1001
    w = torch.rand(n, generator=g) + 0.1 if kind == "random" \
        else torch.ones(n)
    grad = torch.randn(n, d, generator=g) * w.unsqueeze(1)
    comm = Comm()
    want = _fit_stats_before(grad, w, comm)
    got = tree_mod._fused_fit_stats(grad, w, comm)
    _same_stats(got, want)
    assert want["all_one"] == (kind == "ones") and not want["has_zero"]
    # the weight half alone, and both halves put together again
    wst = tree_mod.fit_weight_stats(w, comm)
    _same_stats(wst, {k: v for k, v in want.items()
                      if k not in ("gsum", "gmax")})
    both = dict(wst, gsum=want["gsum"], gmax=want["gmax"])
    for a, b in zip(tree_mod._grow_args(both), tree_mod._grow_args(want)):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b


def test_weight_stats_see_a_zero_weight():
    w = torch.tensor([1.0, 0.0, 2.0])
    st = tree_mod.fit_weight_stats(w, Comm())
    assert st["has_zero"] and not st["all_one"]
    assert st["total_w"] == 3.0 and st["hmax"] == 2.0 and st["n_global"] == 3.0
