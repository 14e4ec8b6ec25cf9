"""BaggingClassifier (reference classification/BaggingClassifier.scala).

Voting (reference :55-67, 260-287): ``soft`` sums per-model
``predictProbability``; ``hard`` sums one-hot votes of per-model ``predict``
(default hard, :67); soft voting with a non-probabilistic base model raises
(:275-277).  ``raw2probability`` divides by numModels (:285-287).
Same per-learner subspace seed+i scheme and seed deviation as
BaggingRegressor (see its docstring).
"""

from __future__ import annotations

import os
from typing import List

import torch

from .. import persistence
from ..ensemble.binning import BinnedDataset
from ..ensemble.params import (
    HasBaseLearner,
    HasComputeOob,
    HasNumBaseLearners,
    HasParallelism,
    HasSubBag,
)
from ..ensemble.utils import OobResults, slice_features, subspace
from ..estimator import (
    ProbabilisticClassificationModel,
    ProbabilisticClassifier,
)
from ..frame import TensorFrame
from ..params import ParamValidators
from ..parallel import get_comm


class _BaggingClassifierParams(
    HasNumBaseLearners, HasBaseLearner, HasParallelism, HasSubBag
):
    def _declare_params(self):
        super()._declare_params()
        self.votingStrategy = self._str_param(
            "votingStrategy",
            "hard (majority vote) or soft (mean probability)",
            ParamValidators.inArray(["hard", "soft"]),
        )
        self.seed = self._int_param("seed", "random seed")
        self._setDefault(numBaseLearners=10, votingStrategy="hard", seed=0)

    def getVotingStrategy(self):
        return self.getOrDefault("votingStrategy")

    def setVotingStrategy(self, v):
        return self.set("votingStrategy", v)

    def setSeed(self, v):
        return self.set("seed", v)


class BaggingClassifier(ProbabilisticClassifier, _BaggingClassifierParams,
                        HasComputeOob):
    def _default_base_learner(self):
        from ..models.tree import DecisionTreeClassifier

        return DecisionTreeClassifier()

    def _fit(self, dataset: TensorFrame) -> "BaggingClassificationModel":
        comm = get_comm()
        learner = self.getOrNone("baseLearner") or self._default_base_learner()
        seed = self.getOrDefault("seed")
        k = self.getNumBaseLearners()
        x, y, w = self._extract_xyw(dataset)
        n, num_features = x.shape
        num_classes = int(comm.all_reduce_scalar(self._get_num_classes(dataset), "max"))
        binned = BinnedDataset(x, dataset)

        subspaces = [
            subspace(self.getSubspaceRatio(), num_features, seed + i) for i in range(k)
        ]

        from ..models.tree import (
            DecisionTreeClassifier, _class_mode_ok, fit_class_tree_forest,
        )

        oob = self.getComputeOob()
        # 7..32 classes fuse too on the GPU (the grower's class mode)
        wide_fused = x.is_cuda and _class_mode_ok(num_classes)
        if (
            type(learner) is DecisionTreeClassifier
            and learner.getOrDefault("minWeightFractionPerNode") == 0.0
            and (num_classes + 2 <= 8 or wide_fused)
        ):
            # fused path: all k gini trees (K one-hot channels each) grow
            # level-synchronously; subspaces as split masks, bags as root
            # row sets — same machinery as the regression fusion
            f_edges, f_bins = binned.get(int(learner.getOrDefault("maxBins")))
            bag_w = torch.stack([
                self.sample_weights(
                    self.getReplacement(), self.getSubsampleRatio(), n,
                    seed + i, x.device, w, comm.rank,
                )
                for i in range(k)
            ], dim=1)
            root_rows = [
                (bag_w[:, i] > 0).nonzero(as_tuple=True)[0].to(torch.int32)
                for i in range(k)
            ]
            onehot = None
            if not wide_fused:  # class mode reads the labels directly
                onehot = torch.zeros(n, num_classes, dtype=torch.float32,
                                     device=x.device)
                onehot.scatter_(1, y.long().unsqueeze(1), 1.0)
            models = fit_class_tree_forest(
                learner, f_edges, f_bins, onehot, bag_w, num_classes, comm,
                subspaces=subspaces, root_rows=root_rows, labels=y,
            )
            model = BaggingClassificationModel()
            model._models = models
            model._subspaces = subspaces
            model._num_classes = num_classes
            model._num_features = num_features
            model.set("votingStrategy", self.getVotingStrategy())
            for p in (
                "featuresCol", "labelCol", "predictionCol",
                "rawPredictionCol", "probabilityCol",
            ):
                model.set(p, self.getOrDefault(p))
            if oob:
                model._oob = self._oob_estimates(
                    x, y, w, models, subspaces, bag_w > 0, num_classes, comm)
            return model

        if learner is not None and learner.hasParam("maxBins"):
            binned.get(int(learner.getOrDefault("maxBins")))  # pre-warm once

        def fit_one(i):
            def task():
                bag_w = self.sample_weights(
                    self.getReplacement(),
                    self.getSubsampleRatio(),
                    n,
                    seed + i,
                    x.device,
                    w,
                    comm.rank,
                )
                fr = binned.fit_frame(learner, y, bag_w, subspaces[i])
                fitted = self.fit_base_learner(learner, fr, weight_col="weight")
                return (fitted, bag_w > 0) if oob else fitted
            return task

        from ..parallel.streams import parallel_fits

        models = parallel_fits([fit_one(i) for i in range(k)],
                               self.getParallelism())
        inbag = None
        if oob:
            inbag = torch.stack([b for _, b in models], dim=1)
            models = [m for m, _ in models]

        model = BaggingClassificationModel()
        model._models = models
        model._subspaces = subspaces
        model._num_classes = num_classes
        model._num_features = num_features
        model.set("votingStrategy", self.getVotingStrategy())
        for p in (
            "featuresCol", "labelCol", "predictionCol",
            "rawPredictionCol", "probabilityCol",
        ):
            model.set(p, self.getOrDefault(p))
        if oob:
            model._oob = self._oob_estimates(
                x, y, w, models, subspaces, inbag, num_classes, comm)
        return model

    def _oob_estimates(self, x, y, w, models, subspaces, inbag, num_classes,
                       comm):
        """Out-of-bag votes of the training rows and their weighted
        accuracy: member i votes on row r only where ``not inbag[r, i]``,
        under the estimator's voting strategy.  Tree members are one
        ``forest_oob`` pass; anything else is a loop over the members in
        order.  A row of instance weight 0 is out of every bag: it gets a
        prediction and weighs nothing in the score.  The score and the
        coverage are sums over all ranks, in float64."""
        from ..ensemble.utils import oob_weighted_sums, packed_forest_oob

        soft = self.getVotingStrategy() == "soft"
        res = packed_forest_oob(x, models, subspaces, x.shape[1], inbag,
                                vote="soft" if soft else "hard")
        if res is not None:
            raw, counts = res
        else:
            n = x.shape[0]
            raw = torch.zeros(n, num_classes, dtype=torch.float32,
                              device=x.device)
            counts = torch.zeros(n, dtype=torch.int32, device=x.device)
            zero = torch.zeros((), dtype=torch.float32, device=x.device)
            for i, (sub, m) in enumerate(zip(subspaces, models)):
                out = ~inbag[:, i]
                xs = slice_features(x, sub)
                if soft:
                    if not hasattr(m, "predictProbability"):
                        raise RuntimeError(
                            "soft voting requires probabilistic base models "
                            "(reference BaggingClassifier.scala:275-277)"
                        )
                    raw = raw + torch.where(
                        out[:, None], m.predictProbability(xs).float(), zero)
                else:
                    pred = m.predict(xs).long()
                    raw.scatter_add_(1, pred.unsqueeze(1),
                                     out.float().unsqueeze(1))
                counts += out.to(torch.int32)
        has = counts > 0
        nan = torch.full((), float("nan"), dtype=torch.float32,
                         device=x.device)
        prob = torch.where(has[:, None], raw / counts[:, None], nan)
        pred = torch.where(has, raw.argmax(dim=1).float(), nan)
        wc = torch.where(has, w, torch.zeros_like(w))
        s_all, s_w, s_hit = oob_weighted_sums(
            comm, [w, wc, wc * (pred == y).float()])
        return {
            "oobRawPrediction": raw, "oobProbability": prob,
            "oobPrediction": pred, "oobCounts": counts,
            "oobScore": s_hit / s_w if s_w > 0 else float("nan"),
            "oobCoverage": s_w / s_all if s_all > 0 else float("nan"),
        }

    def _save_impl(self, path: str):
        persistence.save_metadata(self, path)
        self._save_learner(path)

    def _load_extra(self, path: str, meta: dict):
        self.setBaseLearner(self._load_learner(path))


class BaggingClassificationModel(
    ProbabilisticClassificationModel, _BaggingClassifierParams, OobResults
):
    @property
    def oobRawPrediction(self):
        """``[N, K]`` vote sums of the members that left the row out."""
        return self._oob_get("oobRawPrediction")

    @property
    def oobProbability(self):
        """``oobRawPrediction / oobCounts``; NaN rows where the count is 0."""
        return self._oob_get("oobProbability")

    @property
    def models(self):
        return list(self._models)

    @property
    def subspaces(self):
        return list(self._subspaces)
    _models: List = []
    _subspaces: List[torch.Tensor] = []

    @property
    def numModels(self):
        return len(self._models)

    @property
    def featureImportances(self):
        from ..ensemble.utils import ensemble_feature_importances

        return ensemble_feature_importances(
            self._models, [1.0] * len(self._models), self._subspaces, self._num_features
        )

    def predictRaw(self, features: torch.Tensor) -> torch.Tensor:
        from ..ensemble.utils import packed_forest_vote

        x = features.float()
        k = self._num_classes
        soft = self.getVotingStrategy() == "soft"
        # fast path: every member a built-in classification tree -> ONE
        # packed forest kernel with per-node leaf transforms (normalized
        # probs for soft, one-hot argmax for hard) — exact
        packed = packed_forest_vote(
            x, self._models, self._subspaces, x.shape[1], soft,
            cache=self.__dict__.setdefault(
                "_pack_cache_soft" if soft else "_pack_cache_hard", {}),
        )
        if packed is not None:
            return packed
        acc = torch.zeros(x.shape[0], k, dtype=torch.float32, device=x.device)
        for sub, m in zip(self._subspaces, self._models):
            xs = slice_features(x, sub)
            if soft:
                if not hasattr(m, "predictProbability"):
                    raise RuntimeError(
                        "soft voting requires probabilistic base models "
                        "(reference BaggingClassifier.scala:275-277)"
                    )
                acc += m.predictProbability(xs)
            else:
                pred = m.predict(xs).long()
                acc.scatter_add_(
                    1, pred.unsqueeze(1),
                    torch.ones(x.shape[0], 1, device=x.device),
                )
        return acc

    def predictContrib(self, features: torch.Tensor) -> torch.Tensor:
        """Per-row additive feature contributions ``[N, K, F + 1]`` of the
        vote sums, one plane per class, in the original feature space
        (path-dependent TreeSHAP, docs/contributions.md): column F is the
        bias and plane k of every row sums to ``predictRaw[:, k]``.  Soft
        and hard voting are both sums over leaves of the per-node leaf
        transforms ``predictRaw`` packs, so both are explained exactly.
        Raises ValueError for a member that is not a built-in
        classification tree.  NaN features are not supported."""
        from ..ensemble.utils import packed_forest_contrib
        from ..models.tree import DecisionTreeClassificationModel

        for i, m in enumerate(self._models):
            if not isinstance(m, DecisionTreeClassificationModel):
                raise ValueError(
                    "predictContrib needs built-in classification tree "
                    f"members; member {i} is a {type(m).__name__}"
                )
        soft = self.getVotingStrategy() == "soft"
        mcount = len(self._models)
        return packed_forest_contrib(
            features.float(), self._models, [1.0] * mcount, [0] * mcount,
            self._subspaces, self._num_classes,
            vote="soft" if soft else "hard",
            cache=self.__dict__.setdefault(
                "_contrib_cache_soft" if soft else "_contrib_cache_hard", {}),
        )

    def raw2probabilityInPlace(self, raw: torch.Tensor) -> torch.Tensor:
        raw /= len(self._models)
        return raw

    def _save_impl(self, path: str):
        persistence.save_metadata(
            self, path,
            extra={
                "numClasses": self._num_classes,
                "numModels": len(self._models),
                "numFeatures": self._num_features,
                **self._oob_meta(),
            },
        )
        for i, m in enumerate(self._models):
            m.save(os.path.join(path, f"model-{i}"), overwrite=True)
            persistence.save_json_rows(
                os.path.join(path, f"data-{i}"),
                [{"subspace": self._subspaces[i].tolist()}],
            )

    def _load_extra(self, path: str, meta: dict):
        self._num_classes = meta["numClasses"]
        self._num_features = meta.get("numFeatures", -1)
        self._load_oob(meta)
        self._models = []
        self._subspaces = []
        i = 0
        while os.path.isdir(os.path.join(path, f"model-{i}")):
            self._models.append(
                persistence.load_instance(os.path.join(path, f"model-{i}"))
            )
            row = persistence.load_json_rows(os.path.join(path, f"data-{i}"))[0]
            self._subspaces.append(torch.tensor(row["subspace"], dtype=torch.long))
            i += 1
