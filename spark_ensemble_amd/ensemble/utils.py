"""Ensemble utilities.

``weighted_median`` reproduces reference ensemble/Utils.scala:26-40 (sort by
value, first index where cumulative weight >= half of total); ``subspace`` /
``slice_features`` reproduce the sub-bagging primitives of reference
HasSubBag.scala:73-84 (Bernoulli(ratio) filter over feature indices with a
per-learner seed; sorted indices; dense gather).
"""

from __future__ import annotations

import torch


def weighted_median(values: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """Row-wise weighted median.

    values, weights: [N, M] (M models per row) or [M].  Returns [N] (or
    scalar).  Rule (reference Utils.scala:26-40): sort by value, take the
    first value whose cumulative weight >= 0.5 * total weight.
    """
    single = values.dim() == 1
    if single:
        values = values.unsqueeze(0)
        weights = weights.unsqueeze(0).expand_as(values)
    if weights.dim() == 1:
        weights = weights.unsqueeze(0).expand_as(values)
    order = values.argsort(dim=1)
    v_sorted = values.gather(1, order)
    w_sorted = weights.gather(1, order)
    cum = w_sorted.cumsum(dim=1)
    half = 0.5 * w_sorted.sum(dim=1, keepdim=True)
    # first index with cumulative weight >= half
    idx = (cum >= half).float().argmax(dim=1, keepdim=True)
    out = v_sorted.gather(1, idx).squeeze(1)
    return out[0] if single else out


def subspace(ratio: float, num_features: int, seed: int) -> torch.Tensor:
    """Bernoulli(ratio) feature-index filter, deterministic in ``seed``.

    Mirrors reference HasSubBag.scala:73-79 (XORShiftRandom(seed) Bernoulli
    over 0..numFeatures-1; indices come out sorted).  Guarantees at least one
    feature.  Ratio 1 is the identity (tested property, reference
    HasSubBagSuite.scala:60-105).
    """
    if ratio >= 1.0:
        return torch.arange(num_features, dtype=torch.long)
    g = torch.Generator().manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    mask = torch.rand(num_features, generator=g) < ratio
    idx = mask.nonzero(as_tuple=True)[0]
    if idx.numel() == 0:
        idx = torch.randint(0, num_features, (1,), generator=g)
    return idx.sort().values


def slice_features(x: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
    """Dense feature gather [N, F] -> [N, |indices|]
    (reference HasSubBag.scala:81-84)."""
    if indices.numel() == x.shape[1]:
        # identity subspace — avoid the gather
        if bool((indices == torch.arange(x.shape[1], device=indices.device)).all()):
            return x
    return x.index_select(1, indices.to(x.device))


def orig_space_features(m, sub, num_features):
    """Split-feature ids of the built-in tree model ``m`` in the ORIGINAL
    feature space: ``m._tree["feature"]`` itself under an identity (or
    absent) subspace ``sub``, else the ids mapped through ``sub`` (leaves
    keep their negative marker), built once and cached on the model as
    ``_tree_orig_feats``.  The packed predictors, the contribution pack and
    the staged evaluation walk the unsliced x with these."""
    feat = m._tree["feature"]
    identity = sub is None or (
        sub.numel() == num_features
        and bool((sub.cpu() == torch.arange(num_features)).all())
    )
    if identity:
        return feat
    remapped = getattr(m, "_tree_orig_feats", None)
    if remapped is None:
        fl = feat.long()
        sub_dev = sub.to(fl.device)
        remapped = torch.where(
            fl >= 0, sub_dev[fl.clamp_min(0)], fl
        ).to(torch.int32)
        m._tree_orig_feats = remapped
    return remapped


def packed_forest_margin(x, models, weights, subspaces, num_features,
                         cache=None):
    """Batched ensemble inference fast path: when every stage model is a
    built-in regression tree, the whole ensemble is ONE forest_predict
    kernel call instead of a launch (plus a feature-slice copy) per
    stage.  Non-identity subspaces are handled by remapping each tree's
    split-feature ids back into the ORIGINAL feature space, so the packed
    forest walks the unsliced x.  Returns [N] margins or None when a
    stage is not a tree.  ``cache``: caller-owned dict holding the packed
    arena across transform calls (models are immutable post-fit)."""
    from ..models.tree import DecisionTreeRegressionModel
    from ..ops import dispatch as _ops

    if not models:
        return None
    trees = []
    for m, sub in zip(models, subspaces):
        if not isinstance(m, DecisionTreeRegressionModel):
            return None
        t = m._tree
        feat = orig_space_features(m, sub, num_features)
        if feat is not t["feature"]:
            t = dict(t, feature=feat)
        trees.append(t)
    w = torch.tensor([float(v) for v in weights], dtype=torch.float32)
    return _ops.forest_predict(x, trees, w, cache=cache).squeeze(1)


def _vote_leaves(m, soft):
    """Per-node leaf transform of a classification tree under voting
    (cached on the model): normalized probabilities for soft voting, the
    one-hot argmax for hard voting."""
    attr = "_leaf_soft" if soft else "_leaf_hard"
    lv = getattr(m, attr, None)
    if lv is None:
        leaf = m._tree["leaf_value"]
        if soft:
            lv = leaf / leaf.sum(dim=1, keepdim=True).clamp_min(1e-12)
        else:
            lv = torch.zeros_like(leaf)
            lv.scatter_(1, leaf.argmax(dim=1, keepdim=True), 1.0)
        setattr(m, attr, lv)
    return lv


def packed_forest_vote(x, models, subspaces, num_features, soft,
                       cache=None):
    """Bagging-classifier voting as ONE packed forest_predict call.

    Exactness by leaf transform (cached per model): soft voting sums
    per-row probability vectors — equal to summing leaf vectors
    NORMALIZED per node; hard voting sums one-hot argmax votes — equal to
    summing per-node ONE-HOT(argmax(leaf)) vectors.  Returns [N, K] vote
    sums or None when a member is not a built-in classification tree."""
    from ..models.tree import DecisionTreeClassificationModel
    from ..ops import dispatch as _ops

    if not models:
        return None
    trees = []
    for m, sub in zip(models, subspaces):
        if not isinstance(m, DecisionTreeClassificationModel):
            return None
        t = m._tree
        lv = _vote_leaves(m, soft)
        feat = orig_space_features(m, sub, num_features)
        trees.append(dict(t, feature=feat, leaf_value=lv))
    w = torch.ones(len(trees), dtype=torch.float32)
    return _ops.forest_predict(x, trees, w, cache=cache)


def packed_forest_oob(x, models, subspaces, num_features, inbag, vote=None,
                      cache=None):
    """Out-of-bag sums and counts of a bagged ensemble of built-in trees as
    ONE ``forest_oob`` call: ``(sums [N, D] f32, counts [N] int32)``, member
    i left out of row r's sum where ``inbag[r, i]``.  Regression trees
    (``vote=None``) add their leaf value; classification trees add the
    per-node leaf transform of ``packed_forest_vote`` (``vote`` "soft" /
    "hard"), so the sums are the vote sums of the out-of-bag members.
    Subspaced members walk the unsliced x through the ``_tree_orig_feats``
    remap.  Returns None when a member is not such a tree."""
    from ..models.tree import (
        DecisionTreeClassificationModel, DecisionTreeRegressionModel)
    from ..ops import dispatch as _ops

    if not models:
        return None
    kind = (DecisionTreeRegressionModel if vote is None
            else DecisionTreeClassificationModel)
    trees = []
    for m, sub in zip(models, subspaces):
        if not isinstance(m, kind):
            return None
        t = m._tree
        if vote is not None:
            t = dict(t, leaf_value=_vote_leaves(m, vote == "soft"))
        feat = orig_space_features(m, sub, num_features)
        if feat is not m._tree["feature"]:
            t = dict(t, feature=feat)
        trees.append(t)
    return _ops.forest_oob(x, trees, inbag, cache=cache)


def oob_weighted_sums(comm, terms):
    """float64 sums over the rows of every rank of each ``[N]`` tensor in
    ``terms``: one all-reduce, so every rank gets the same numbers."""
    s = torch.stack([t.double().sum() for t in terms])
    return comm.all_reduce_(s, "sum").tolist()


class OobResults:
    """Out-of-bag results of a bagging model (docs/bagging.md).  ``_oob`` is
    None for a model fitted without ``computeOob``.  The per-row tensors are
    training-set-sized and rank-local, and are not saved; the score and the
    coverage go into the saved metadata, so a loaded model answers those two
    and None for the rest."""

    _oob = None
    _OOB_SAVED = ("oobScore", "oobCoverage")

    def _oob_get(self, key):
        return None if self._oob is None else self._oob.get(key)

    @property
    def oobPrediction(self):
        """``[N]`` f32 out-of-bag prediction of every training row, NaN
        where no member left the row out."""
        return self._oob_get("oobPrediction")

    @property
    def oobCounts(self):
        """``[N]`` int32: the members that left the row out of their bag."""
        return self._oob_get("oobCounts")

    @property
    def oobScore(self):
        """Weighted R^2 (regression) or accuracy (classification) of the
        out-of-bag predictions over the rows that have one; NaN if none."""
        return self._oob_get("oobScore")

    @property
    def oobCoverage(self):
        """Weighted share of the rows with an out-of-bag prediction."""
        return self._oob_get("oobCoverage")

    def _oob_meta(self):
        if self._oob is None:
            return {}
        return {k: self._oob[k] for k in self._OOB_SAVED}

    def _load_oob(self, meta):
        if all(k in meta for k in self._OOB_SAVED):
            self._oob = {k: float(meta[k]) for k in self._OOB_SAVED}


def packed_forest_contrib(x, models, weights, planes, subspaces, num_planes,
                          vote=None, cache=None):
    """Per-row feature contributions of an ensemble of built-in trees as ONE
    ``forest_contrib`` call: ``[N, num_planes, F + 1]``, column F the bias
    (semantics in docs/contributions.md).  Member i adds ``weights[i]``
    times its tree into plane ``planes[i]`` (a K-vector-leaf tree into
    planes ``planes[i] .. planes[i] + K - 1``).  Subspaced members are
    reported in the ORIGINAL feature space through the same
    ``_tree_orig_feats`` remap the packed predictors use.  ``vote``
    ("soft" / "hard") swaps in the per-node leaf transform of
    ``packed_forest_vote`` to explain the vote sums.  Raises
    ValueError for a member that is not a built-in tree."""
    from ..models.tree import _TreeModelMixin
    from ..ops import dispatch as _ops

    num_features = x.shape[1]
    trees = []
    for i, (m, sub) in enumerate(zip(models, subspaces)):
        if not isinstance(m, _TreeModelMixin):
            raise ValueError(
                f"predictContrib needs built-in tree members; member {i} is "
                f"a {type(m).__name__}"
            )
        t = m._tree
        if vote is not None:
            t = dict(t, leaf_value=_vote_leaves(m, vote == "soft"))
        feat = orig_space_features(m, sub, num_features)
        if feat is not m._tree["feature"]:
            t = dict(t, feature=feat)
        trees.append(t)
    return _ops.forest_contrib(
        x, trees, [float(v) for v in weights], [int(p) for p in planes],
        num_planes, cache=cache,
    )


def ensemble_feature_importances(models, weights, subspaces, num_features):
    """Weighted, subspace-mapped aggregate of member featureImportances
    (normalized to sum 1; zeros when no member exposes importances)."""
    agg = torch.zeros(num_features, dtype=torch.float64)
    for m, w, sub in zip(models, weights, subspaces):
        fi = getattr(m, "featureImportances", None)
        if fi is None:
            continue
        fi = fi.double() * abs(float(w))
        if sub is None or fi.numel() == num_features:
            agg[: fi.numel()] += fi
        else:
            agg.index_add_(0, sub.cpu().long(), fi)
    t = float(agg.sum())
    return (agg / t if t > 0 else agg).float()
