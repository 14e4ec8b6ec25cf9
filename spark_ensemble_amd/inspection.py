"""Permutation importance (docs/importance.md).

How much a fitted model's loss on a frame of the user's choice grows when one
feature column is shuffled::

    importances[r, f] = (sum_i w_i loss_i(x with column f shuffled by
                         permutation r) - sum_i w_i loss_i(x)) / sum_i w_i

One permutation per repeat is shared by all features (only one column is
swapped at a time, so the per-feature estimates stay independent); it is
drawn on the CPU from ``seed + r`` so every device sees the same donors.

``permutation_importance`` serves any fitted model through a column-swap
loop over ``predict``: F * R predicts.  The ``permutationImportance`` methods
of the GBM, bagging-regression and tree-regression models go through
``ensemble_permutation_importance``: with built-in tree members the whole
``[R, F]`` table is ONE ``forest_permute_loss`` pass (csrc/forest_permute.hip
on the GPU), anything else is the same loop over the model's margins.
"""

from __future__ import annotations

import torch

from .parallel import get_comm


class PermutationImportance:
    """Result of a permutation-importance run.  ``baseline`` is the weighted
    mean loss on the unshuffled frame (a float), ``importances`` the
    ``[R, F]`` CPU float64 table of mean-loss increases; ``mean`` and ``std``
    are over the repeats (population standard deviation: 0 for R = 1)."""

    def __init__(self, baseline: float, importances: torch.Tensor):
        self.baseline = float(baseline)
        self.importances = importances.to("cpu", torch.float64)

    @property
    def mean(self) -> torch.Tensor:
        return self.importances.mean(dim=0)

    @property
    def std(self) -> torch.Tensor:
        return self.importances.std(dim=0, unbiased=False)

    def __repr__(self):
        r, f = self.importances.shape
        return (f"PermutationImportance(baseline={self.baseline:.6g}, "
                f"repeats={r}, features={f})")


def draw_donors(n: int, num_repeats: int, seed: int) -> torch.Tensor:
    """``[R, n]`` int64 on the CPU: row r is
    ``torch.randperm(n, generator=torch.Generator().manual_seed(seed + r))``."""
    if not isinstance(num_repeats, int) or num_repeats < 1:
        raise ValueError(f"numRepeats must be a positive integer, "
                         f"got {num_repeats!r}")
    return torch.stack([
        torch.randperm(n, generator=torch.Generator().manual_seed(seed + r))
        for r in range(num_repeats)]).reshape(num_repeats, n)


def column_swap_sums(x, donors, loss_sum):
    """``(base, perm [R, F])`` float64 on the CPU by the definition: one
    call of ``loss_sum(x')`` (a weighted loss SUM over the rows) per repeat
    and feature, x' being x with the one column taken from the donors."""
    donors = donors.to(x.device)
    R, F = donors.shape[0], x.shape[1]
    base = float(loss_sum(x))
    perm = torch.empty(R, F, dtype=torch.float64)
    for r in range(R):
        for f in range(F):
            xp = x.clone()
            xp[:, f] = x[donors[r], f]
            perm[r, f] = float(loss_sum(xp))
    return base, perm


def _frame(model, dataset):
    """(x, y, w) f32 of ``dataset`` under the model's column settings; row
    weights from ``weightCol`` when it is set and present, else ones (as
    ``evaluateEachIteration``).  Sharded frames are out of scope."""
    if get_comm().is_distributed:
        raise ValueError(
            "permutation importance of a frame sharded over several ranks "
            "is not supported: run it on one rank")
    x = dataset[model.getFeaturesCol()].float()
    y = dataset[model.getLabelCol()].float()
    wcol = model.getWeightCol()
    if wcol and wcol in dataset:
        w = dataset[wcol].float()
    else:
        w = torch.ones(x.shape[0], dtype=torch.float32, device=x.device)
    return x, y, w


def _result(base, perm, w):
    wsum = float(w.double().sum())
    base = float(base)
    perm = perm.to("cpu", torch.float64)
    return PermutationImportance(base / wsum, (perm - base) / wsum)


def squared_only(loss):
    """The squared loss of the models whose importance loss is fixed."""
    from .boosting.losses import SquaredLoss

    if loss is not None and loss != "squared" and type(loss) is not SquaredLoss:
        raise ValueError(
            f"this model's permutation importance is under the squared loss; "
            f"got loss={loss!r}")
    return SquaredLoss()


def permutation_importance(model, dataset, numRepeats=5, seed=0, loss=None):
    """Permutation importance of ANY fitted model on ``dataset`` through the
    column-swap loop over ``model.predict`` on the model's own device.

    ``loss``: None for the project's squared loss ``0.5 (y - p)^2`` of
    ``predict`` (regressors) or the zero-one error of ``predict``
    (classifiers); or a callable ``loss(y [N], prediction [N]) -> [N]``."""
    from .estimator import ClassificationModel

    x, y, w = _frame(model, dataset)
    donors = draw_donors(x.shape[0], numRepeats, seed)
    if loss is None:
        if isinstance(model, ClassificationModel):
            def loss(y_, p):
                return (p != y_).to(torch.float32)
        else:
            def loss(y_, p):
                return 0.5 * (y_ - p) ** 2

    def loss_sum(xx):
        return (loss(y, model.predict(xx).float()) * w).double().sum()

    return _result(*column_swap_sums(x, donors, loss_sum), w)


def ensemble_permutation_importance(model, dataset, numRepeats, seed, loss,
                                    dim, stages, init, margins):
    """Permutation importance of an additive ensemble under the ``GBMLoss``
    ``loss``.  ``stages`` is a list of (models, weights, subspace) with
    ``dim`` models and weights each, ``init`` the init model (None: zero)
    and ``margins(x)`` the model's full ``[N, dim]`` margins.

    Fused route: ``dim == 1``, every stage model a built-in scalar-leaf
    regression tree (the test ``packed_forest_margin`` applies; subspaces
    are mapped back to full-frame columns as there), and an init that is
    absent, constant, or itself such a tree (it joins the forest with weight
    1).  Everything else is the column-swap loop over ``margins``."""
    from .boosting.staged import _stage_trees
    from .models.dummy import DummyClassificationModel, DummyRegressionModel
    from .models.tree import DecisionTreeRegressionModel
    from .ops import dispatch as _ops

    x, y, w = _frame(model, dataset)
    N = x.shape[0]
    donors = draw_donors(N, numRepeats, seed)
    label = loss.encode_label(y)

    trees = _stage_trees(stages, x.shape[1]) if dim == 1 and stages else None
    if trees is not None:
        tw = [float(v) for _, wts, _ in stages for v in wts]
        if init is None:
            init_m = torch.zeros(N, dtype=torch.float32, device=x.device)
        elif isinstance(init, DummyRegressionModel):
            init_m = init.predict(x).float()  # a constant: no column in it
        elif isinstance(init, DummyClassificationModel):
            init_m = init.predictRaw(x)[:, 0].float()
        elif (isinstance(init, DecisionTreeRegressionModel)
              and init._tree["leaf_value"].shape[1] == 1):
            trees, tw = [init._tree] + trees, [1.0] + tw
            init_m = torch.zeros(N, dtype=torch.float32, device=x.device)
        else:
            trees = None
    if trees is not None:
        base, perm = _ops.forest_permute_loss(
            x, trees, tw, init_m, label.reshape(N), w, loss, donors,
            cache=model.__dict__.setdefault("_permute_cache", {}))
        return _result(base, perm, w)

    def loss_sum(xx):
        m = margins(xx).float().reshape(N, dim)
        return (loss.loss(label, m) * w).double().sum()

    return _result(*column_swap_sums(x, donors, loss_sum), w)
