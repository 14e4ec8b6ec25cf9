"""Per-stage evaluation and truncation of fitted GBM models.

``evaluateEachIteration(dataset, loss)`` of Spark ML's GBT models: the
weighted mean loss on a frame after the init model alone and after every
boosting stage.  When every stage is a built-in tree the whole curve is ONE
``forest_staged_loss`` pass over the rows (csrc/forest_staged.hip on the GPU:
x is read once, no [N, stages] intermediate); any other base learner takes
the generic path, stage by stage through ``predict``.  Both GBM model classes
share this module; they differ only in how a loss name is resolved and in
the shape of their stage lists.
"""

from __future__ import annotations

from typing import List

import torch

from ..ensemble.utils import orig_space_features, slice_features
from ..parallel import get_comm
from .losses import GBMLoss


def resolve_loss(model, loss, from_name, dim: int) -> GBMLoss:
    """``loss`` as a GBMLoss: None -> the model's own loss name, a name ->
    ``from_name(name)``, an instance as it is.  Huber's delta is adapted per
    round during the fit and not stored on the model, so it only comes as an
    instance."""
    if loss is None:
        loss = model.getLoss()
    if isinstance(loss, str):
        if loss.lower() == "huber":
            raise ValueError(
                "the huber delta is adapted per round during the fit and is "
                "not stored on the model; pass a HuberLoss(delta) instance")
        loss = from_name(loss)
    if not isinstance(loss, GBMLoss):
        raise ValueError(f"loss must be a name or a GBMLoss, not {loss!r}")
    if loss.dim != dim:
        raise ValueError(
            f"loss {loss.name!r} has dim {loss.dim} but the model's margins "
            f"have dim {dim}")
    return loss


def _stage_trees(stages, num_features):
    """Tree dicts in stage-major order with split features in the original
    feature space, or None when a stage model is not a built-in scalar-leaf
    regression tree."""
    from ..models.tree import DecisionTreeRegressionModel

    trees = []
    for models, _, sub in stages:
        for m in models:
            if not isinstance(m, DecisionTreeRegressionModel):
                return None
            t = m._tree
            if t["leaf_value"].shape[1] != 1:
                return None
            feat = orig_space_features(m, sub, num_features)
            if feat is not t["feature"]:
                t = dict(t, feature=feat)
            trees.append(t)
    return trees


def evaluate_each_iteration(model, dataset, loss: GBMLoss, dim: int,
                            stages: List, init_margins) -> torch.Tensor:
    """CPU float64 ``[len(stages) + 1]``: entry s is the weighted mean of
    ``loss`` on ``dataset`` after the first s stages, entry 0 the init model
    alone.  ``stages`` is a list of (models, weights, subspace) with ``dim``
    models and weights each; ``init_margins(x)`` gives ``[N, dim]``.

    Under a distributed communicator the S + 1 numerators and the weight sum
    travel in one all-reduce, so every rank returns the same tensor and the
    collective sequence does not depend on the data."""
    from ..ops import dispatch as _ops

    x = dataset[model.getFeaturesCol()].float()
    y = dataset[model.getLabelCol()].float()
    wcol = model.getWeightCol()
    if wcol and wcol in dataset:
        w = dataset[wcol].float()
    else:
        w = torch.ones(x.shape[0], dtype=torch.float32, device=x.device)
    label = loss.encode_label(y)
    margins = init_margins(x).float().reshape(x.shape[0], dim).contiguous()

    trees = _stage_trees(stages, x.shape[1])
    if trees is not None:
        flat_w = [float(v) for _, wts, _ in stages for v in wts]
        sums = _ops.forest_staged_loss(
            x, trees, flat_w, dim, margins, label, w, loss,
            cache=model.__dict__.setdefault("_staged_cache", {}),
        ).double()
    else:
        # generic path: any base learner, one predict per (stage, column)
        sums = [(loss.loss(label, margins) * w).double().sum()]
        for models, wts, sub in stages:
            xs = slice_features(x, sub)
            margins = margins.clone()
            for j, m in enumerate(models):
                margins[:, j] += float(wts[j]) * m.predict(xs)
            sums.append((loss.loss(label, margins) * w).double().sum())
        sums = torch.stack(sums)

    red = torch.cat([sums, w.double().sum().reshape(1).to(sums.device)])
    comm = get_comm()
    if comm.is_distributed:
        comm.all_reduce_(red)
    red = red.cpu()
    return red[:-1] / red[-1]


def truncated(model, n: int):
    """A new model of ``model``'s class keeping the init and the first n
    stages: stage lists sliced, params and column settings copied
    (``Params.copy``), stage models shared.  Only the fitted fields listed
    below travel, so caches (packs, contribution tables) are not inherited."""
    n_models = len(model._models)
    if not isinstance(n, int) or isinstance(n, bool) or not 0 <= n <= n_models:
        raise ValueError(
            f"truncate: n must be an integer in [0, {n_models}], got {n!r}")
    out = model.copy()  # same class, params and column settings
    # the fitted state, field by field: caches and per-fit records stay behind
    for name in ("_init", "_num_features", "_num_classes", "_dim"):
        if hasattr(model, name):
            setattr(out, name, getattr(model, name))
    out._models = list(model._models[:n])
    out._weights = list(model._weights[:n])
    out._subspaces = list(model._subspaces[:n])
    return out
