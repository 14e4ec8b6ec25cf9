"""GBM shared params (reference boosting/GBMParams.scala:26-136).

Defaults (reference :121-129): optimizedWeights=true, updates=gradient,
learningRate=1.0, numBaseLearners=10, tol=1e-6, maxIter=100, numRounds=1,
validationTol=0.01, and replacement=false for GBM's sub-bagging.
"""

from __future__ import annotations

from ..ensemble.params import (
    HasAggregationDepth,
    HasBaseLearner,
    HasCheckpointInterval,
    HasNumBaseLearners,
    HasSubBag,
)
from ..params import Params, ParamValidators

SUPPORTED_UPDATES = ["newton", "gradient"]
SUPPORTED_SAMPLING = ["uniform", "goss"]


class GBMParams(
    HasNumBaseLearners,
    HasBaseLearner,
    HasSubBag,
    HasCheckpointInterval,
    HasAggregationDepth,
):
    def _declare_params(self):
        super()._declare_params()
        self.optimizedWeights = self._bool_param(
            "optimizedWeights", "line-search the stage weights"
        )
        self.updates = self._str_param(
            "updates",
            "pseudo-residual mode: newton or gradient",
            ParamValidators.inArray(SUPPORTED_UPDATES),
        )
        self.learningRate = self._float_param(
            "learningRate", "shrinkage per stage", ParamValidators.gt(0.0)
        )
        self.validationTol = self._float_param(
            "validationTol",
            "early-stop tolerance on validation loss",
            ParamValidators.gtEq(0.0),
        )
        self.numRounds = self._int_param(
            "numRounds",
            "patience rounds before early stop",
            ParamValidators.gtEq(1),
        )
        self.maxIter = self._int_param(
            "maxIter", "max line-search iterations", ParamValidators.gtEq(1)
        )
        self.tol = self._float_param(
            "tol", "line-search / quantile tolerance", ParamValidators.gtEq(0.0)
        )
        self.validationIndicatorCol = self._str_param(
            "validationIndicatorCol",
            "boolean column marking validation rows",
            lower=False,
        )
        self.seed = self._int_param("seed", "random seed")
        self.sampling = self._str_param(
            "sampling",
            "row sampling per round: uniform (subsampleRatio / replacement) "
            "or goss (gradient-based one-side sampling)",
            ParamValidators.inArray(SUPPORTED_SAMPLING),
        )
        self.topRate = self._float_param(
            "topRate",
            "goss: fraction of rows kept for their gradient magnitude",
            ParamValidators.inRange(0.0, 1.0, False, False),
        )
        self.otherRate = self._float_param(
            "otherRate",
            "goss: fraction of rows drawn from the rest",
            ParamValidators.inRange(0.0, 1.0, False, False),
        )
        self._setDefault(sampling="uniform", topRate=0.2, otherRate=0.1)
        self._setDefault(
            optimizedWeights=True,
            updates="gradient",
            learningRate=1.0,
            numBaseLearners=10,
            tol=1e-6,
            maxIter=100,
            numRounds=1,
            validationTol=0.01,
            replacement=False,
            subsampleRatio=1.0,
            subspaceRatio=1.0,
            seed=0,
        )

    def _fused_round_wstats(self, learner, dim, idx, x, w, comm, state):
        """The per-fit weight statistics when this round may run through
        ``models.tree.fit_gbm_round_tree`` (one native pass from the margins
        to the grower's gradient matrix), else None: one margin column,
        gradient updates, full bags, the identity subspace, the built-in
        regression tree without a weight-fraction threshold, GPU tensors with
        the HIP extension, no zero weight, and ``SEA_ROUND_FUSED`` not "0"
        (read at every call).  ``state`` is fit-local and caches the
        statistics, taken with one host sync on the first eligible round: the
        weights of a full bag are the same in every round."""
        from ..ensemble.binning import _is_identity
        from ..models.tree import DecisionTreeRegressor, fit_weight_stats
        from ..ops import dispatch as ops

        if "static_ok" not in state:
            state["static_ok"] = (
                type(learner) is DecisionTreeRegressor
                and learner.getOrDefault("minWeightFractionPerNode") == 0.0
            )
        if not (
            dim == 1
            and state["static_ok"]
            and self.getOrDefault("sampling") == "uniform"
            and self.getOrDefault("updates") == "gradient"
            and self.getSubsampleRatio() >= 1.0
            and not self.getReplacement()
            and x.is_cuda
            and ops.round_fused_enabled()
            and ops.hip_available()
            and _is_identity(idx, x.shape[1])
        ):
            return None
        if state.get("wstats") is None:
            state["wstats"] = fit_weight_stats(w, comm)
        return None if state["wstats"]["has_zero"] else state["wstats"]

    def _check_sampling(self):
        """What ``fit`` refuses under ``sampling="goss"``."""
        if self.getOrDefault("sampling") != "goss":
            return
        top, other = self.getOrDefault("topRate"), self.getOrDefault("otherRate")
        if top + other > 1.0:
            raise ValueError(
                f"goss: topRate + otherRate = {top + other} exceeds 1")
        if self.getSubsampleRatio() != 1.0:
            raise ValueError("goss: subsampleRatio must be 1, the rates of "
                             "goss replace it")
        if self.getReplacement():
            raise ValueError("goss samples without replacement")

    def _round_bag(self, g, w, seed, comm, instr):
        """The bag multiplicities [N] of one round: Bernoulli / Poisson draws
        under ``sampling="uniform"``, else GOSS on the round's gradients
        ``g`` [N, dim] and the row weights ``w``, over this rank's rows."""
        if self.getOrDefault("sampling") != "goss":
            return self.sample_weights(
                self.getReplacement(), self.getSubsampleRatio(), g.shape[0],
                seed, g.device, None, comm.rank,
            )
        from ..ops import dispatch as ops

        bag_m = ops.goss_weights(
            g, w, self.getOrDefault("topRate"), self.getOrDefault("otherRate"),
            seed, comm.rank,
        )
        instr.log_named_value("goss_kept_rows", int((bag_m > 0).sum()))
        return bag_m

    def setSampling(self, v):
        return self.set("sampling", v)

    def setTopRate(self, v):
        return self.set("topRate", v)

    def setOtherRate(self, v):
        return self.set("otherRate", v)

    def setOptimizedWeights(self, v):
        return self.set("optimizedWeights", v)

    def setUpdates(self, v):
        return self.set("updates", v)

    def setLearningRate(self, v):
        return self.set("learningRate", v)

    def setValidationTol(self, v):
        return self.set("validationTol", v)

    def setNumRounds(self, v):
        return self.set("numRounds", v)

    def setMaxIter(self, v):
        return self.set("maxIter", v)

    def setTol(self, v):
        return self.set("tol", v)

    def setValidationIndicatorCol(self, v):
        return self.set("validationIndicatorCol", v)

    def setSeed(self, v):
        return self.set("seed", v)
