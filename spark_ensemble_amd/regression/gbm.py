"""GBMRegressor — gradient/newton boosting for regression.

Re-creates reference regression/GBMRegressor.scala:237-476 on the MI355X
stack: margins and residuals are resident [N] tensors updated by fused
kernels; every reference treeAggregate becomes an RCCL all-reduce
(SURVEY.md section 2.6); base learners are fit through the same
``fit_base_learner`` choke point with per-round pseudo-residual labels.

Reference semantics kept exactly:
  * initStrategy {constant, zero, base}; constant maps loss -> Dummy
    statistic (squared->mean, absolute|huber->median, quantile->quantile)
    (reference :287-303)
  * huber adaptive delta: label alpha-quantile at init, |residual|
    alpha-quantile each round (:305-309, 342-353)
  * newton pseudo-residuals with hessian floor 1e-2 and weight
    0.5 * h / sum(h) * w (:368-385)
  * stage-weight line search on [0, 100] (:398-425) — Brent for
    non-smooth losses exactly as the reference; for losses with a
    continuous second derivative a safeguarded Newton iteration finds the
    SAME minimizer in 3-6 fused evaluations (documented deviation from
    the reference's always-Brent; equivalence tested in test_losses)
  * patience early stop: v += 1 when bestErr - err <
    validationTol * max(err, 0.01); final model keeps i - v stages (:444-474)

Documented deviation: the reference resamples its bag with the SAME seed
every round (GBMRegressor.scala:357-359, a known quirk); we use seed + i
per round (as the reference itself does for subspaces, :141-143).
"""

from __future__ import annotations

import os
from typing import List, Optional

import torch

from .. import persistence
from ..boosting.gbm_params import GBMParams
from ..boosting.line_search import optimize_weight_1d
from ..boosting.losses import get_regression_loss
from ..ensemble.binning import BinnedDataset
from ..ensemble.utils import slice_features, subspace
from ..estimator import RegressionModel, Regressor
from ..frame import TensorFrame
from ..models.dummy import DummyRegressor
from ..params import ParamValidators
from ..parallel import get_comm
from ..utils.stats import dist_mean, dist_quantile

SUPPORTED_LOSSES = ["squared", "absolute", "huber", "quantile", "logcosh", "scaledlogcosh"]
SUPPORTED_INIT = ["constant", "zero", "base"]


class _GBMRegressorParams(GBMParams):
    def _declare_params(self):
        super()._declare_params()
        self.initStrategy = self._str_param(
            "initStrategy",
            "init prediction strategy: constant|zero|base",
            ParamValidators.inArray(SUPPORTED_INIT),
        )
        self.loss = self._str_param(
            "loss",
            "loss function: " + "|".join(SUPPORTED_LOSSES),
            ParamValidators.inArray(SUPPORTED_LOSSES),
        )
        self.alpha = self._float_param(
            "alpha",
            "quantile for huber/quantile losses",
            ParamValidators.inRange(0.0, 1.0),
        )
        self._setDefault(initStrategy="constant", loss="squared", alpha=0.9)

    def getLoss(self):
        return self.getOrDefault("loss")

    def setLoss(self, v):
        return self.set("loss", v)

    def setInitStrategy(self, v):
        return self.set("initStrategy", v)

    def setAlpha(self, v):
        return self.set("alpha", v)

    def _make_loss(self, delta: float):
        return get_regression_loss(
            self.getLoss(),
            alpha=self.getOrDefault("alpha"),
            delta=delta,
            quantile=self.getOrDefault("alpha"),
        )


class GBMRegressor(Regressor, _GBMRegressorParams):
    def __init__(self, uid=None):
        super().__init__(uid)

    def _default_base_learner(self):
        from ..models.tree import DecisionTreeRegressor

        return DecisionTreeRegressor()

    def _fit(self, dataset: TensorFrame) -> "GBMRegressionModel":
        from ..utils.instrumentation import Instrumentation

        instr = Instrumentation(self, dataset)
        instr.log_params(self, "loss", "numBaseLearners", "updates",
                         "learningRate", "optimizedWeights")
        comm = get_comm()
        learner = (
            self.getOrNone("baseLearner") or self._default_base_learner()
        )
        alpha = self.getOrDefault("alpha")
        seed = self.getOrDefault("seed")
        k_stages = self.getNumBaseLearners()
        lr_rate = self.getOrDefault("learningRate")
        use_newton = self.getOrDefault("updates") == "newton"
        optimized = self.getOrDefault("optimizedWeights")

        # -- validation split (reference :265-273) -------------------------
        vcol = self.getOrNone("validationIndicatorCol")
        if vcol:
            vmask = dataset[vcol].bool()
            train = dataset.filter(~vmask)
            val = dataset.filter(vmask)
        else:
            train, val = dataset, None

        x, y, w = self._extract_xyw(train)
        n, num_features = x.shape
        device = x.device
        binned = BinnedDataset(x, train)

        subspaces = [
            subspace(self.getSubspaceRatio(), num_features, seed + i)
            for i in range(k_stages)
        ]

        # -- init model (reference :287-303) -------------------------------
        init_strategy = self.getOrDefault("initStrategy")
        loss_name = self.getLoss()
        if init_strategy == "base":
            init = self.fit_base_learner(
                learner, binned.fit_frame(learner, y, w)
            )
        else:
            if init_strategy == "zero":
                dummy = DummyRegressor().setStrategy("constant").setConstant(0.0)
            else:
                if loss_name == "squared":
                    dummy = DummyRegressor().setStrategy("mean")
                elif loss_name in ("absolute", "huber", "logcosh", "scaledlogcosh"):
                    dummy = DummyRegressor().setStrategy("median")
                else:  # quantile
                    dummy = DummyRegressor().setStrategy("quantile").setQuantile(alpha)
            init = dummy.fit(TensorFrame(features=x, label=y, weight=w))

        # huber initial delta from the label alpha-quantile (reference :305-309)
        delta = (
            dist_quantile(y, alpha, None, comm) if loss_name == "huber" else alpha
        )

        predictions = init.predict(x)  # [N]
        if val is not None:
            xv, yv, wv = self._extract_xyw(val)
            val_pred = init.predict(xv)
            l0 = self._make_loss(delta)
            best_err = dist_mean(
                l0.loss(yv.unsqueeze(1), val_pred.unsqueeze(1)), comm
            )
        else:
            best_err = 0.0

        models: List = []
        weights: List[float] = []
        i = 0
        v = 0

        # -- resume from a round-state checkpoint ----------
        from ..utils import checkpoint as ckpt

        ckpt_dir = self.getCheckpointDir()
        ck_fp = (
            ckpt.fingerprint(self, n, num_features, y, w) if ckpt_dir else None
        )
        ck_saved: set = set()
        resumed = ckpt.load_round_state(ckpt_dir, ck_fp)
        if resumed:
            r0, models, weights, extra = resumed
            r0 = min(r0, k_stages)
            models, weights = models[:r0], weights[:r0]
            for j, (m, wt) in enumerate(zip(models, weights)):
                xs_j = slice_features(x, subspaces[j])
                predictions = predictions + wt * m.predict(xs_j)
                if val is not None:
                    val_pred = val_pred + wt * m.predict(
                        slice_features(xv, subspaces[j])
                    )
            best_err = extra.get("best_err", best_err)
            v = int(extra.get("v", 0))
            i = r0
            instr.log_named_value("resumed_from_round", r0)

        while i < k_stages and v < self.getOrDefault("numRounds"):
            if loss_name == "huber":
                delta = dist_quantile((y - predictions).abs(), alpha, None, comm)
            loss = self._make_loss(delta)

            idx = subspaces[i]
            xs = binned.sliced_features(idx)

            # bag multiplicities (sampling only) and full weights
            bag_m = self.sample_weights(
                self.getReplacement(),
                self.getSubsampleRatio(),
                n,
                seed + i,
                device,
                None,
                comm.rank,
            )
            bag_w = bag_m * w

            ylab = y.unsqueeze(1)
            pred2 = predictions.unsqueeze(1)
            newton = use_newton and loss.has_hessian
            g, h = loss.grad_hess_fused(ylab, pred2, want_hess=newton)
            if newton:
                h = h.squeeze(1).clamp_min(1e-2)
                sum_h = comm.all_reduce_scalar(float((h * bag_m).sum()))
                res_label = -g.squeeze(1) / h
                res_weight = 0.5 * h / sum_h * bag_w
            else:
                res_label = -g.squeeze(1)
                res_weight = bag_w

            fr = binned.fit_frame(learner, res_label, res_weight, idx, xs)
            model = self.fit_base_learner(learner, fr, weight_col="weight")

            # tree base learners capture train-row predictions during
            # growth (leaf scatter) — avoids a full tree walk per round
            direction = getattr(model, "_train_pred", None)
            if direction is None or direction.shape[0] != xs.shape[0]:
                direction = model.predict(xs)  # [N]

            if optimized:
                sol = optimize_weight_1d(
                    loss,
                    ylab,
                    pred2,
                    direction.unsqueeze(1),
                    bag_w,
                    comm,
                    self.getOrDefault("maxIter"),
                    self.getOrDefault("tol"),
                )
            else:
                sol = 1.0
            weight = lr_rate * sol

            models.append(model)
            weights.append(weight)

            predictions = predictions + weight * direction

            if val is not None:
                val_pred = val_pred + weight * model.predict(slice_features(xv, idx))
                err = dist_mean(
                    loss.loss(yv.unsqueeze(1), val_pred.unsqueeze(1)), comm
                )
                if best_err - err < self.getOrDefault("validationTol") * max(err, 0.01):
                    v += 1
                elif err < best_err:
                    best_err = err
                    v = 0
                from ..boosting import line_search as _ls
                instr.log_round(i, weight=weight, val_loss=err, patience=v,
                                ls_evals=_ls.LAST_EVALS)
            else:
                from ..boosting import line_search as _ls
                instr.log_round(i, weight=weight, ls_evals=_ls.LAST_EVALS)
            interval = self.getCheckpointInterval()
            if ckpt_dir and interval > 0 and (i + 1) % interval == 0:
                ckpt.save_round_state(
                    ckpt_dir, i + 1, models, weights,
                    extra={"best_err": best_err, "v": v},
                    fingerprint=ck_fp, _saved_dirs=ck_saved,
                )
            i += 1
        instr.finish()
        # a completed fit owns no resume state (resume is crash recovery
        # only — checkpointInterval must never change the fitted result)
        ckpt.clear(ckpt_dir)

        keep = i - v
        model = GBMRegressionModel()
        model._init = init
        model._models = models[:keep]
        model._weights = weights[:keep]
        model._subspaces = [s for s in subspaces[:keep]]
        model._num_features = num_features
        # loss and alpha: what evaluateEachIteration(loss=None) evaluates
        for p in ("featuresCol", "labelCol", "predictionCol", "loss", "alpha"):
            model.set(p, self.getOrDefault(p))
        if self.getWeightCol():  # ... and the rows' weights
            model.set("weightCol", self.getWeightCol())
        return model

    # ---- fold-vectorized fitting (OOF stacking fast path) ----------------
    def _can_fit_folds(self) -> bool:
        """The fold-fused fit covers the default configuration: squared
        loss, gradient updates, constant init, full bags, identity
        subspace, built-in tree learner, no validation/checkpointing.
        Anything else falls back to independent per-fold fits."""
        from ..models.tree import DecisionTreeRegressor

        learner = self.getOrNone("baseLearner") or self._default_base_learner()
        return (
            self.getLoss() == "squared"
            and self.getOrDefault("initStrategy") == "constant"
            and self.getOrDefault("updates") == "gradient"
            and self.getSubspaceRatio() >= 1.0
            and self.getSubsampleRatio() >= 1.0
            and not self.getReplacement()
            and self.getOrNone("validationIndicatorCol") is None
            and not self.getCheckpointDir()
            and type(learner) is DecisionTreeRegressor
            and learner.getOrDefault("minWeightFractionPerNode") == 0.0
        )

    def _fit_folds(self, dataset: TensorFrame, fold: torch.Tensor,
                   num_folds: int, include_full: bool = False):
        """num_folds leave-one-fold-out GBM fits grown JOINTLY: every
        boosting round builds ONE fused forest (grow_forest with per-tree
        root row sets = each fold's training rows) and the squared-loss
        stage weights come in closed form (a* = sum(w d r)/sum(w d^2) on
        the fold's rows — the exact minimizer Brent/Newton converge to),
        so a round costs one forest build + two reductions regardless of
        the fold count.  The MI355X answer to OOF stacking's many small
        sequential fits (reference StackingRegressor.scala:141-153 runs
        whole fits in driver futures)."""
        from ..models.dummy import DummyRegressionModel
        from ..models.tree import DecisionTreeRegressionModel
        from ..models.tree_grower import grow_forest

        comm = get_comm()
        learner = self.getOrNone("baseLearner") or self._default_base_learner()
        T = int(num_folds)
        k_stages = self.getNumBaseLearners()
        lr_rate = self.getOrDefault("learningRate")
        optimized = self.getOrDefault("optimizedWeights")

        x, y, w = self._extract_xyw(dataset)
        n, num_features = x.shape
        device = x.device
        binned = BinnedDataset(x, dataset)
        edges, bins = binned.get(int(learner.getOrDefault("maxBins")))

        fold = fold.to(device)
        masks = [(fold != f) for f in range(T)]
        if include_full:
            # one extra "fold" seeing every row = the final full-data
            # refit, grown in the same fused forest
            masks.append(torch.ones_like(fold, dtype=torch.bool))
            T = T + 1
        root_rows = [m.nonzero(as_tuple=True)[0].to(torch.int32)
                     for m in masks]
        mask_f = torch.stack([m.float() for m in masks], dim=1)  # [N, T]
        w2 = w.unsqueeze(1) * mask_f

        # constant init: the sequential path's DummyRegressor reproduces
        # the reference's UNWEIGHTED SQL mean (DummyRegressor.scala:113-129
        # ignores instance weights — a reference quirk), so every fold
        # model starts from the same global unweighted label mean
        red = torch.stack([y.sum(), torch.tensor(float(n), device=device)])
        comm.all_reduce_(red)
        init_c = (red[0] / red[1].clamp_min(1e-12)).expand(T)  # [T] device

        margins = init_c.unsqueeze(0).expand(n, T).contiguous()
        hic = bool((w == 1).all())
        gp = learner._grow_params(1.0)

        fold_trees: List[List] = [[] for _ in range(T)]
        alphas_per_round: List[torch.Tensor] = []
        for i in range(k_stages):
            resid = y.unsqueeze(1) - margins
            grads = (resid * w.unsqueeze(1)).contiguous()
            stats = torch.stack([grads.abs().max(), w.max()])
            if comm.is_distributed:
                comm.all_reduce_(stats, "max")
            sc = stats.cpu()
            gh_max = torch.tensor(
                [float(sc[0]), float(sc[1])] + ([] if hic else [1.0])
            )
            tp: list = []
            trees = grow_forest(bins, edges, grads, w, gp, comm,
                                hess_is_count=hic, train_pred_out=tp,
                                gh_max_in=gh_max, root_rows=root_rows)
            d = tp[0]  # [N, T]; zero on held-out rows
            if optimized:
                red = torch.cat([
                    (w2 * d * resid).sum(0), (w2 * d * d).sum(0)
                ])
                comm.all_reduce_(red)
                alphas = (red[:T] / red[T:].clamp_min(1e-30)).clamp(0.0, 100.0)
            else:
                alphas = torch.ones(T, device=device)
            alphas = alphas * lr_rate
            alphas_per_round.append(alphas)
            margins = margins + d * alphas.unsqueeze(0)
            for t, tree in enumerate(trees):
                m = DecisionTreeRegressionModel()
                m._set_tree(tree, num_features)
                m._copy_cols_from(learner)
                fold_trees[t].append(m)

        stage_w = torch.stack(alphas_per_round).cpu()  # [k, T] one sync
        init_cpu = init_c.cpu()
        ident = torch.arange(num_features)
        out: List[GBMRegressionModel] = []
        for t in range(T):
            init = DummyRegressionModel()
            init._constant = float(init_cpu[t])
            init._num_features = num_features
            init.set("strategy", "constant")
            model = GBMRegressionModel()
            model._init = init
            model._models = fold_trees[t]
            model._weights = [float(v) for v in stage_w[:, t]]
            model._subspaces = [ident] * k_stages
            model._num_features = num_features
            for p in ("featuresCol", "labelCol", "predictionCol", "loss",
                      "alpha"):
                model.set(p, self.getOrDefault(p))
            if self.getWeightCol():
                model.set("weightCol", self.getWeightCol())
            out.append(model)
        if include_full:
            return out[:-1], out[-1]
        return out

    def _save_impl(self, path: str):
        persistence.save_metadata(self, path)
        self._save_learner(path)

    def _load_extra(self, path: str, meta: dict):
        self.setBaseLearner(self._load_learner(path))


class GBMRegressionModel(RegressionModel, _GBMRegressorParams):
    @property
    def models(self):
        """Per-stage base models (reference GBMRegressionModel.models)."""
        return list(self._models)

    @property
    def weights(self):
        """Per-stage weights (reference .weights)."""
        return list(self._weights)
    _init = None
    _models: List = []
    _weights: List[float] = []
    _subspaces: List[torch.Tensor] = []

    def predict(self, features: torch.Tensor) -> torch.Tensor:
        from ..ensemble.utils import packed_forest_margin

        x = features.float()
        out = self._init.predict(x)
        packed = packed_forest_margin(
            x, self._models, self._weights, self._subspaces, x.shape[1],
            cache=self.__dict__.setdefault("_pack_cache", {}),
        )
        if packed is not None:
            return out + packed
        for wgt, sub, m in zip(self._weights, self._subspaces, self._models):
            out = out + wgt * m.predict(slice_features(x, sub))
        return out

    def predictContrib(self, features: torch.Tensor) -> torch.Tensor:
        """Per-row additive feature contributions ``[N, F + 1]`` (path-
        dependent TreeSHAP, docs/contributions.md): column F is the bias and
        every row sums to ``predict``.  A constant init goes into the bias;
        an init that is a tree model joins the forest with weight 1; any
        other init, or a stage that is not a built-in tree, raises
        ValueError.  NaN features are not supported."""
        from ..ensemble.utils import packed_forest_contrib
        from ..models.dummy import DummyRegressionModel
        from ..models.tree import DecisionTreeRegressionModel

        x = features.float()
        models, weights = list(self._models), list(self._weights)
        subs = list(self._subspaces)
        const = 0.0
        if isinstance(self._init, DummyRegressionModel):
            const = float(self._init._constant)
        elif isinstance(self._init, DecisionTreeRegressionModel):
            models.insert(0, self._init)
            weights.insert(0, 1.0)
            subs.insert(0, None)
        else:
            raise ValueError(
                "predictContrib needs a constant or tree init model, not a "
                f"{type(self._init).__name__}"
            )
        out = packed_forest_contrib(
            x, models, weights, [0] * len(models), subs, 1,
            cache=self.__dict__.setdefault("_contrib_cache", {}),
        )[:, 0, :]
        out[:, -1] += const
        return out

    @property
    def numModels(self) -> int:
        return len(self._models)

    def evaluateEachIteration(self, dataset: TensorFrame, loss=None):
        """Weighted mean loss on ``dataset`` after the init model alone
        (entry 0) and after each boosting stage: a CPU float64 tensor of
        length ``numModels + 1`` (Spark ML GBT ``evaluateEachIteration``).
        ``loss``: None for the model's own loss, a regression loss name
        (built with the model's alpha), or a ``GBMLoss`` instance.  Huber's
        delta is not stored on the model: pass ``HuberLoss(delta)``.  Row
        weights come from ``weightCol`` when it is set and present.  With
        built-in tree stages the whole curve is one fused pass over the
        rows (docs/gbm.md, "Learning curves")."""
        from ..boosting import staged

        alpha = self.getOrDefault("alpha")
        loss = staged.resolve_loss(
            self, loss, lambda name: get_regression_loss(name, alpha=alpha), 1)
        stages = [([m], [wt], sub) for m, wt, sub in
                  zip(self._models, self._weights, self._subspaces)]
        return staged.evaluate_each_iteration(
            self, dataset, loss, 1, stages,
            lambda x: self._init.predict(x).unsqueeze(1))

    def permutationImportance(self, dataset: TensorFrame, numRepeats=5,
                              seed=0, loss=None):
        """Permutation importance on ``dataset`` (docs/importance.md): a
        ``PermutationImportance`` with the ``[numRepeats, F]`` increases of
        the weighted mean loss when one feature column is shuffled.
        ``loss`` is resolved as in ``evaluateEachIteration``.  With built-in
        tree stages and a constant or tree init the whole table is one
        fused pass over the rows; anything else is a column-swap loop over
        ``predict``."""
        from .. import inspection
        from ..boosting import staged

        alpha = self.getOrDefault("alpha")
        loss = staged.resolve_loss(
            self, loss, lambda name: get_regression_loss(name, alpha=alpha), 1)
        stages = [([m], [wt], sub) for m, wt, sub in
                  zip(self._models, self._weights, self._subspaces)]
        return inspection.ensemble_permutation_importance(
            self, dataset, numRepeats, seed, loss, 1, stages, self._init,
            lambda x: self.predict(x).unsqueeze(1))

    def truncate(self, n: int) -> "GBMRegressionModel":
        """A new model keeping the init and the first ``n`` stages
        (``0 <= n <= numModels``); stage models are shared, not copied."""
        from ..boosting import staged

        return staged.truncated(self, n)

    @property
    def featureImportances(self):
        from ..ensemble.utils import ensemble_feature_importances

        return ensemble_feature_importances(
            self._models, self._weights, self._subspaces, self._num_features
        )

    # -- persistence (reference GBMRegressor.scala:563-605 layout) ---------
    def _save_impl(self, path: str):
        persistence.save_metadata(
            self, path,
            extra={"numFeatures": self._num_features, "numModels": len(self._models)},
        )
        self._init.save(os.path.join(path, "init"), overwrite=True)
        for i, m in enumerate(self._models):
            m.save(os.path.join(path, f"model-{i}"), overwrite=True)
            persistence.save_json_rows(
                os.path.join(path, f"data-{i}"),
                [{
                    "weight": float(self._weights[i]),
                    "subspace": self._subspaces[i].tolist(),
                }],
            )

    def _load_extra(self, path: str, meta: dict):
        self._num_features = meta.get("numFeatures", -1)
        self._init = persistence.load_instance(os.path.join(path, "init"))
        self._models = []
        self._weights = []
        self._subspaces = []
        i = 0
        while os.path.isdir(os.path.join(path, f"model-{i}")):
            self._models.append(persistence.load_instance(os.path.join(path, f"model-{i}")))
            row = persistence.load_json_rows(os.path.join(path, f"data-{i}"))[0]
            self._weights.append(row["weight"])
            self._subspaces.append(torch.tensor(row["subspace"], dtype=torch.long))
            i += 1
