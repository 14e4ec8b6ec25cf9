"""Multi-process distributed tests over gloo (world_size 2, CPU).

These exercise the same code paths RCCL takes on an 8-GPU node: the
histogram all-reduce inside tree growth, scalar reductions in boosting,
distributed quantiles, and the full GBM round loop.  The parity assertion:
a 2-rank fit over a row-sharded dataset must closely match a 1-rank fit of
the union (identical split decisions come from identical all-reduced
histograms)."""

import json
import os
import subprocess
import sys
import tempfile

import pytest
import torch

WORKER = r"""
import json, os, sys
import torch
import torch.distributed as dist

sys.path.insert(0, os.environ["SEA_REPO"])
from spark_ensemble_amd.parallel import init_from_env
from spark_ensemble_amd.utils.io import synthetic_classification, synthetic_regression
from spark_ensemble_amd.utils.stats import dist_quantile, dist_weighted_mean
from spark_ensemble_amd.models import DecisionTreeClassifier
import spark_ensemble_amd as sea

comm = init_from_env(backend="gloo")
rank, world = comm.rank, comm.world_size
out = {}

# --- dist_quantile / mean over a sharded vector -------------------------
g = torch.Generator().manual_seed(99 + rank)
local = torch.randn(20000, generator=g) * 2 + 1
q = dist_quantile(local, 0.5, None, comm)
mw = dist_weighted_mean(local, torch.ones_like(local), comm)
out["median"] = q
out["mean"] = mw

# --- tree fit parity: sharded 2-rank fit vs the same global data --------
df = synthetic_classification(30000, 16, k=3, seed=5, shard=(rank, world))
m = DecisionTreeClassifier().setMaxDepth(5).fit(df)
test = synthetic_classification(5000, 16, k=3, seed=5, split=1)
pred = m.transform(test)["prediction"]
out["tree_pred"] = pred.tolist()

# --- GBM fit across ranks ------------------------------------------------
dfr = synthetic_regression(20000, 12, seed=6, shard=(rank, world))
gbm = sea.GBMRegressor().setNumBaseLearners(3).fit(dfr)
testr = synthetic_regression(4000, 12, seed=6, split=1)
out["gbm_rmse"] = float(((gbm.predict(testr["features"]) - testr["label"]) ** 2).mean() ** 0.5)

# --- boosting across ranks ----------------------------------------------
bst = sea.BoostingRegressor().setNumBaseLearners(3).fit(dfr)
out["boost_rmse"] = float(((bst.predict(testr["features"]) - testr["label"]) ** 2).mean() ** 0.5)

# --- out-of-fold stacking across ranks (collective sequence must match
#     on every rank through 2 learners x 5 folds + final refits) ---------
from spark_ensemble_amd.models import LinearRegression
stk = (sea.StackingRegressor()
       .setBaseLearners([sea.GBMRegressor().setNumBaseLearners(2),
                         sea.BaggingRegressor().setNumBaseLearners(2)])
       .setStacker(LinearRegression())
       .setNumFolds(3).setSeed(4).fit(dfr))
out["stack_rmse"] = float(((stk.predict(testr["features"]) - testr["label"]) ** 2).mean() ** 0.5)

# --- logistic regression: fused payload all-reduce -----------------------
lr = sea.LogisticRegression().setMaxIter(15).fit(df)
outp = lr.transform(test)
out["logreg_acc"] = float((outp["prediction"] == test["label"]).float().mean())

# --- evaluator all-reduce -------------------------------------------------
from spark_ensemble_amd.tuning import MulticlassClassificationEvaluator
ev = MulticlassClassificationEvaluator("accuracy")
out["eval_acc"] = ev.evaluate(m.transform(df))

# --- BIT-EXACT sharded-vs-single parity ---------------------------------
# categorical (identity-edge) features kill the only nondeterminism
# source (sample-dependent quantile edges), and integer-valued labels
# with unit weights make every histogram cell an exact small-integer f32
# sum — order-independent, so the 2-rank all-reduced tree must equal the
# single-process tree BITWISE.
from spark_ensemble_amd.frame import TensorFrame
from spark_ensemble_amd.models import DecisionTreeRegressor

ge = torch.Generator().manual_seed(17)
xi_all = torch.randint(0, 32, (40000, 8), generator=ge).float()
yi_all = (xi_all[:, 0] > 15).float() * 4 + (xi_all[:, 1] % 3).float()
xi = xi_all[rank::world]
yi = yi_all[rank::world]
dfx = TensorFrame(features=xi, label=yi)
dfx.set_categorical({f: 32 for f in range(8)})
mex = DecisionTreeRegressor().setMaxDepth(6).setMaxBins(32).fit(dfx)
out["exact_tree"] = {
    k: v.tolist() for k, v in mex._tree.items() if k != "feature_importance"
}

if rank == 0:
    with open(os.environ["SEA_OUT"], "w") as f:
        json.dump(out, f)
dist.barrier()
"""


def _run_world(tmpdir, nproc=2):
    script = os.path.join(tmpdir, "worker.py")
    with open(script, "w") as f:
        f.write(WORKER)
    outfile = os.path.join(tmpdir, "out.json")
    env = dict(os.environ)
    env["SEA_REPO"] = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env["SEA_OUT"] = outfile
    env["MASTER_ADDR"] = "127.0.0.1"
    # gloo/CPU worlds: hide the GPUs from the workers, otherwise on a GPU
    # host every rank binds cuda:<local_rank> and ranks past the device
    # count die (a 2-rank world on a 1-GPU machine)
    env["HIP_VISIBLE_DEVICES"] = "-1"
    env["CUDA_VISIBLE_DEVICES"] = "-1"
    import random

    last = None
    for attempt in range(2):
        prt = "29871" if attempt == 0 else str(random.randint(29500, 29989))
        cmd = [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", f"--nproc-per-node={nproc}",
            "--master-addr", "127.0.0.1", "--master-port", prt,
            script,
        ]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True,
                           timeout=600)
        if r.returncode == 0:
            break
        last = r
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(outfile) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def world2_results(tmp_path_factory):
    return _run_world(str(tmp_path_factory.mktemp("dist")))


def test_dist_quantile_and_mean(world2_results):
    # both ranks' shards are N(1, 2): global median/mean ~ 1
    assert abs(world2_results["median"] - 1.0) < 0.06
    assert abs(world2_results["mean"] - 1.0) < 0.06


def test_sharded_tree_close_to_single_process(world2_results):
    from spark_ensemble_amd.models import DecisionTreeClassifier
    from spark_ensemble_amd.utils.io import synthetic_classification

    # single-process fit over BOTH shards concatenated
    a = synthetic_classification(30000, 16, k=3, seed=5, shard=(0, 2))
    b = synthetic_classification(30000, 16, k=3, seed=5, shard=(1, 2))
    xs = torch.cat([a["features"], b["features"]])
    ys = torch.cat([a["label"], b["label"]])
    from spark_ensemble_amd.frame import TensorFrame

    df = TensorFrame(features=xs, label=ys)
    m = DecisionTreeClassifier().setMaxDepth(5).fit(df)
    test = synthetic_classification(5000, 16, k=3, seed=5, split=1)
    pred1 = m.transform(test)["prediction"]
    pred2 = torch.tensor(world2_results["tree_pred"])
    # quantile edges differ slightly (shard-local sampling), so demand high
    # agreement rather than bit equality
    agree = float((pred1 == pred2).float().mean())
    assert agree > 0.9, agree


def test_dist_gbm_quality(world2_results):
    # distributed GBM must actually learn (far below label std ~ 5.7)
    assert world2_results["gbm_rmse"] < 4.0


def test_dist_boosting_quality(world2_results):
    assert world2_results["boost_rmse"] < 5.0


def test_dist_stacking_quality(world2_results):
    assert world2_results["stack_rmse"] < 1.2 * world2_results["gbm_rmse"]


def test_dist_logreg_and_evaluator(world2_results):
    assert world2_results["logreg_acc"] > 0.5


def test_sharded_tree_bit_exact_with_fixed_edges(world2_results):
    """With categorical identity edges (no sample-dependent quantiles)
    and exact-integer histogram sums, the 2-rank all-reduced tree equals
    the single-process tree BITWISE (pin the
    collectives with a fixed-edge variant)."""
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.models import DecisionTreeRegressor

    ge = torch.Generator().manual_seed(17)
    xi = torch.randint(0, 32, (40000, 8), generator=ge).float()
    yi = (xi[:, 0] > 15).float() * 4 + (xi[:, 1] % 3).float()
    dfx = TensorFrame(features=xi, label=yi)
    dfx.set_categorical({f: 32 for f in range(8)})
    m = DecisionTreeRegressor().setMaxDepth(6).setMaxBins(32).fit(dfx)
    got = world2_results["exact_tree"]
    for k in ("feature", "threshold", "left_child", "leaf_value"):
        single = m._tree[k]
        dist2 = torch.tensor(got[k], dtype=single.dtype).reshape(single.shape)
        assert torch.equal(single, dist2), k
    assert 0.0 <= world2_results["eval_acc"] <= 1.0
