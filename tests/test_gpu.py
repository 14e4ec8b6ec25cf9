"""GPU tests (MI355X): HIP kernel numerics vs the torch fp32 reference,
and end-to-end estimator fits on device.  All marked @pytest.mark.gpu."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from spark_ensemble_amd.ops import dispatch

    assert dispatch.hip_available(), "HIP extension must be built in-tree"
    return dispatch


@pytest.fixture(scope="module")
def ref():
    from spark_ensemble_amd.ops import reference

    return reference


def test_native_extension_loaded(hip):
    import spark_ensemble_amd._hip_ops as m

    assert m.__file__.endswith(".so")


def test_bin_features_matches_reference(hip, ref):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(20000, 37, generator=g).to(DEV)
    edges = ref.quantile_bins(x, 64)
    got = hip.bin_features(x, edges)
    want = ref.bin_features(x, edges)
    assert torch.equal(got.cpu(), want.cpu())


def test_sample_weights_stats(hip):
    w = hip.sample_weights(True, 0.7, 1_000_000, 5, DEV)
    assert abs(float(w.mean()) - 0.7) < 0.01
    assert (w == w.round()).all()
    b = hip.sample_weights(False, 0.25, 1_000_000, 6, DEV)
    assert set(b.unique().cpu().tolist()) <= {0.0, 1.0}
    assert abs(float(b.mean()) - 0.25) < 0.01
    # deterministic in seed
    assert torch.equal(
        hip.sample_weights(True, 0.5, 1000, 9, DEV),
        hip.sample_weights(True, 0.5, 1000, 9, DEV),
    )


def test_hist_build_matches_reference(hip, ref):
    g = torch.Generator().manual_seed(2)
    n, f, b, d = 30000, 40, 32, 2
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8).to(DEV)
    # channel contract: first d signed grads, rest non-negative hess/count
    gh = torch.cat(
        [torch.randn(n, d, generator=g), torch.rand(n, 2, generator=g)], dim=1
    ).to(DEV)
    rows = torch.randperm(n, generator=g)[: n - 100].to(torch.int32).to(DEV)
    # one launch with a single-chunk node, a multi-chunk node, an empty
    # node and a second multi-chunk node (staging slot != node id)
    offs = torch.tensor([0, 2000, 11000, 11000, n - 100])
    got = hip.hist_build(bins, gh, rows, offs, b, d)
    want = ref.hist_build(bins.cpu(), gh.cpu(), rows.cpu(), offs, b)
    assert torch.allclose(got.cpu(), want, atol=2e-2, rtol=1e-4)
    assert torch.equal(got[2].cpu(), torch.zeros(f, b, d + 2))

    import spark_ensemble_amd._hip_ops as m

    out = torch.empty_like(got)
    n_multi = m.hist_build(
        out, bins, gh, rows, offs, b, d, gh.abs().amax(dim=0).cpu(), False,
        torch.empty(0, dtype=torch.int32), 0,
    )
    assert n_multi == 2
    assert torch.equal(out, got)


def test_hist_build_all_nodes_empty(hip):
    g = torch.Generator().manual_seed(2)
    n, f, b, d = 3000, 40, 32, 2
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8).to(DEV)
    gh = torch.cat(
        [torch.randn(n, d, generator=g), torch.rand(n, 2, generator=g)], dim=1
    ).to(DEV)
    rows = torch.empty(0, dtype=torch.int32, device=DEV)
    got = hip.hist_build(bins, gh, rows, torch.tensor([0, 0, 0]), b, d)
    assert got.shape == (2, f, b, d + 2)
    assert torch.equal(got.cpu(), torch.zeros(2, f, b, d + 2))


def test_hist_build_256bins_multiclass(hip, ref):
    g = torch.Generator().manual_seed(3)
    n, f, b, d = 20000, 17, 256, 5
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8).to(DEV)
    gh = torch.cat(
        [torch.randn(n, d, generator=g), torch.rand(n, 2, generator=g)], dim=1
    ).to(DEV)
    rows = torch.arange(n, dtype=torch.int32).to(DEV)
    offs = torch.tensor([0, n])
    got = hip.hist_build(bins, gh, rows, offs, b, d)
    want = ref.hist_build(bins.cpu(), gh.cpu(), rows.cpu(), offs, b)
    assert torch.allclose(got.cpu(), want, atol=2e-2, rtol=1e-4)


def test_partition_rows_matches_reference(hip, ref):
    g = torch.Generator().manual_seed(4)
    n, f, b = 50000, 12, 32
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8).to(DEV)
    rows = torch.arange(n, dtype=torch.int32).to(DEV)
    offs = torch.tensor([0, 20000, n])
    feat = torch.tensor([3, -1], dtype=torch.int32)
    thr = torch.tensor([15, 0], dtype=torch.int32)
    new_rows, new_offs, lc = hip.partition_rows(bins, rows, offs, feat, thr)
    # same membership as reference (order within a side is unordered)
    rn, ro, rl = ref.partition_rows(bins.cpu(), rows.cpu(), offs, feat, thr)
    assert torch.equal(new_offs, ro)
    assert torch.equal(lc.cpu(), rl)
    for seg in range(4):
        a = new_rows[new_offs[seg] : new_offs[seg + 1]].cpu()
        bseg = rn[ro[seg] : ro[seg + 1]]
        assert torch.equal(a.sort().values, bseg.sort().values)


def test_tree_and_forest_predict_match_reference(hip, ref):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(10000, 8, generator=g).to(DEV)
    # grow a couple of real trees on CPU to get valid node arrays
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.models import DecisionTreeRegressor

    trees = []
    for s in range(3):
        y = torch.randn(10000, generator=g)
        m = DecisionTreeRegressor().setMaxDepth(6).setSeed(s).fit(
            TensorFrame(features=x.cpu(), label=y)
        )
        trees.append({k: v for k, v in m._tree.items()})
    t0 = {k: v.to(DEV) for k, v in trees[0].items()}
    got = hip.tree_predict(
        x, t0["feature"], t0["threshold"], t0["left_child"], t0["leaf_value"], 64
    )
    want = ref.tree_predict(
        x.cpu(), trees[0]["feature"], trees[0]["threshold"],
        trees[0]["left_child"], trees[0]["leaf_value"], 64,
    )
    assert torch.allclose(got.cpu(), want, atol=1e-6)

    w = torch.tensor([0.5, 1.0, 2.0])
    gotf = hip.forest_predict(x, [
        {k: v.to(DEV) for k, v in t.items()} for t in trees
    ], w.to(DEV))
    wantf = ref.forest_predict(x.cpu(), trees, w)
    assert torch.allclose(gotf.cpu(), wantf, atol=1e-4)


def test_grown_tree_gpu_matches_cpu():
    # the whole grower: same data, GPU kernels vs CPU reference path
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.models import DecisionTreeClassifier
    from spark_ensemble_amd.utils.io import synthetic_classification

    df_cpu = synthetic_classification(30000, 24, k=3, seed=21)
    df_gpu = df_cpu.to(DEV)
    m_cpu = DecisionTreeClassifier().setMaxDepth(6).fit(df_cpu)
    m_gpu = DecisionTreeClassifier().setMaxDepth(6).fit(df_gpu)
    p_cpu = m_cpu.transform(df_cpu)["prediction"]
    p_gpu = m_gpu.transform(df_gpu)["prediction"].cpu()
    # float-atomic ordering can flip a few near-tie splits; agreement must
    # still be near-total
    agree = float((p_cpu == p_gpu).float().mean())
    assert agree > 0.98, agree


@pytest.mark.parametrize(
    "est",
    ["bagging_clf", "boosting_clf", "gbm_clf", "gbm_logloss", "gbm_reg",
     "gbm_huber", "stacking_reg"],
)
def test_end_to_end_gpu_fits(est):
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.models import (
        DecisionTreeRegressor,
        LinearRegression,
    )
    from spark_ensemble_amd.utils.io import (
        synthetic_classification,
        synthetic_regression,
    )

    if est in ("gbm_reg", "gbm_huber", "stacking_reg"):
        df = synthetic_regression(50000, 32, seed=31, device=DEV)
        dft = synthetic_regression(20000, 32, seed=31, split=1, device=DEV)
    else:
        df = synthetic_classification(50000, 32, k=2, seed=31, device=DEV)
        dft = synthetic_classification(20000, 32, k=2, seed=31, split=1, device=DEV)

    if est == "bagging_clf":
        m = sea.BaggingClassifier().setNumBaseLearners(5).setSubsampleRatio(0.8).fit(df)
    elif est == "boosting_clf":
        m = sea.BoostingClassifier().setNumBaseLearners(5).fit(df)
    elif est == "gbm_clf":
        m = sea.GBMClassifier().setLoss("bernoulli").setNumBaseLearners(5).fit(df)
    elif est == "gbm_logloss":
        # vector (K-dim) L-BFGS-B line search path
        m = sea.GBMClassifier().setLoss("logloss").setNumBaseLearners(3).fit(df)
    elif est == "gbm_reg":
        m = sea.GBMRegressor().setNumBaseLearners(5).fit(df)
    elif est == "gbm_huber":
        # non-smooth loss -> Brent line search on the hess-less payload
        m = sea.GBMRegressor().setLoss("huber").setNumBaseLearners(5).fit(df)
    else:
        m = (
            sea.StackingRegressor()
            .setBaseLearners([DecisionTreeRegressor().setMaxDepth(5), LinearRegression()])
            .setStacker(LinearRegression())
            .setNumFolds(3)
            .fit(df)
        )
    if est in ("gbm_reg", "gbm_huber", "stacking_reg"):
        p = m.predict(dft["features"])
        ss = float(((p - dft["label"]) ** 2).mean())
        var = float(dft["label"].var())
        assert ss < var, "must beat predicting the mean"
    else:
        out = m.transform(dft)
        acc = float((out["prediction"] == dft["label"]).float().mean())
        assert acc > 0.6, acc


def test_gpu_losses_match_cpu():
    from spark_ensemble_amd.boosting.losses import get_classification_loss

    loss = get_classification_loss("logloss", 4)
    g = torch.Generator().manual_seed(7)
    y = torch.randint(0, 4, (5000,), generator=g).float()
    pred = torch.randn(5000, 4, generator=g)
    lab = loss.encode_label(y)
    l_cpu = loss.loss(lab, pred)
    grad_cpu = loss.gradient(lab, pred)
    l_gpu = loss.loss(lab.to(DEV), pred.to(DEV)).cpu()
    grad_gpu = loss.gradient(lab.to(DEV), pred.to(DEV)).cpu()
    assert torch.allclose(l_cpu, l_gpu, atol=1e-5)
    assert torch.allclose(grad_cpu, grad_gpu, atol=1e-5)


def test_grad_hess_kernel_matches_torch(hip):
    from spark_ensemble_amd.boosting.losses import (
        BernoulliLoss, ExponentialLoss, HuberLoss, LogCoshLoss, LogLoss,
        QuantileLoss, ScaledLogCoshLoss, SquaredLoss, AbsoluteLoss,
    )

    g = torch.Generator().manual_seed(11)
    n = 20000
    for loss in [SquaredLoss(), AbsoluteLoss(), LogCoshLoss(),
                 ScaledLogCoshLoss(0.3), HuberLoss(0.8), QuantileLoss(0.7),
                 ExponentialLoss(), BernoulliLoss(), LogLoss(4)]:
        if loss.name == "logloss":
            y = torch.randint(0, 4, (n,), generator=g).float()
        elif loss.name in ("exponential", "bernoulli"):
            y = torch.randint(0, 2, (n,), generator=g).float()
        else:
            y = torch.randn(n, generator=g)
        lab = loss.encode_label(y)
        pred = torch.randn(n, loss.dim, generator=g)
        want_g = loss.gradient(lab, pred)
        got_g, got_h = loss.grad_hess_fused(
            lab.to(DEV), pred.to(DEV), want_hess=loss.has_hessian
        )
        assert torch.allclose(got_g.cpu(), want_g, atol=1e-4), loss.name
        if loss.has_hessian:
            want_h = loss.hessian(lab, pred)
            assert torch.allclose(got_h.cpu(), want_h, atol=1e-4), loss.name


def test_line_search_eval_matches_torch(hip):
    from spark_ensemble_amd.boosting.line_search import _eval
    from spark_ensemble_amd.boosting.losses import BernoulliLoss, LogLoss

    g = torch.Generator().manual_seed(12)
    n = 40000
    for loss, D in [(BernoulliLoss(), 1), (LogLoss(3), 3)]:
        y = torch.randint(0, max(2, D), (n,), generator=g).float()
        lab = loss.encode_label(y)
        pred = torch.randn(n, D, generator=g)
        dr = torch.randn(n, D, generator=g)
        w = torch.rand(n, generator=g)
        coeff = torch.rand(D, generator=g) if D > 1 else 0.7
        want = _eval(loss, lab, pred, dr, w, coeff)
        got = _eval(
            loss, lab.to(DEV), pred.to(DEV), dr.to(DEV), w.to(DEV),
            coeff.to(DEV) if isinstance(coeff, torch.Tensor) else coeff,
        ).cpu()
        assert torch.allclose(got, want, rtol=2e-3, atol=2e-2), (loss.name, got, want)


@pytest.mark.parametrize("f,k,bias", [(256, 2, True), (1024, 2, True),
                                      (100, 3, False), (512, 4, True)])
def test_logreg_loss_grad_matches_reference(hip, ref, f, k, bias):
    g = torch.Generator().manual_seed(11)
    n = 20000
    x = torch.randn(n, f, generator=g).to(DEV)
    y = torch.randint(0, k, (n,), generator=g, dtype=torch.int32).to(DEV)
    w = torch.rand(n, generator=g).to(DEV)
    fp = f + (1 if bias else 0)
    wmat = (torch.randn(fp, k, generator=g) * 0.05).to(DEV)
    got = hip.logreg_loss_grad(x, y, w, wmat, bias)
    want = ref.logreg_loss_grad(x, y, w, wmat, bias)
    # loss and gradient sums over 20k rows: fp32 atomics, tolerate 1e-3 rel
    assert torch.allclose(got[0], want[0], rtol=1e-3, atol=1e-2)
    assert torch.allclose(got[1:], want[1:], rtol=1e-3, atol=5e-2), (
        (got[1:] - want[1:]).abs().max()
    )


def test_logistic_regression_gpu_fit():
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(30000, 64, k=2, seed=7, device=DEV)
    m = sea.LogisticRegression().setMaxIter(40).fit(df)
    out = m.transform(df)
    acc = float((out["prediction"] == df["label"]).float().mean())
    assert acc > 0.8, acc


@pytest.mark.parametrize("n,f,b,c,d", [(3, 40, 32, 4, 2), (8, 64, 256, 2, 1),
                                       (1, 256, 256, 3, 1)])
def test_split_argmax_matches_reference(hip, ref, n, f, b, c, d):
    # hist must be a REAL histogram (per-feature totals equal — the
    # hist_build invariant the kernel relies on: the reference scores the
    # parent from feature 0's totals, the kernel from each feature's own)
    g = torch.Generator().manual_seed(21)
    rows_n = 4000
    bins = torch.randint(0, b, (rows_n, f), generator=g, dtype=torch.uint8)
    gh = torch.cat(
        [torch.randn(rows_n, d, generator=g),
         torch.rand(rows_n, c - d, generator=g)], dim=1
    )
    seg = rows_n // n
    offs = torch.tensor([i * seg for i in range(n)] + [rows_n])
    rows = torch.arange(rows_n, dtype=torch.int32)
    hist = ref.hist_build(bins, gh, rows, offs, b).float()
    hist_gpu = hist.to(DEV)
    for mig, mcw in [(0.0, 0.0), (0.05, 0.3)]:
        got = hip.split_search(hist_gpu, 1e-6, mcw, 1.0, mig, d_dims=d)
        want = ref.split_search(hist, 1e-6, mcw, 1.0, mig, d_dims=d)
        gg, gf, gb, gls = [t.cpu() for t in got]
        wg, wf, wb, wls = want
        fin = torch.isfinite(wg)
        assert torch.equal(torch.isfinite(gg), fin)
        assert torch.allclose(gg[fin], wg[fin], rtol=1e-3, atol=1e-4)
        assert torch.equal(gf[fin], wf[fin]), (gf, wf, gg, wg)
        assert torch.equal(gb[fin], wb[fin])
        assert torch.allclose(gls[fin], wls[fin].float(), rtol=1e-4, atol=1e-4)


def test_hist_build_deterministic(hip):
    """instead of the reference's no-op race story, the
    rebuild pins determinism — fixed-point integer LDS accumulation makes
    hist_build bitwise-reproducible across runs (f32 atomics would not be)."""
    g = torch.Generator().manual_seed(33)
    n, f, b, d = 200000, 32, 256, 1
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8).to(DEV)
    gh = torch.cat(
        [torch.randn(n, d, generator=g), torch.rand(n, 1, generator=g)], dim=1
    ).to(DEV)
    rows = torch.randperm(n, generator=g).to(torch.int32).to(DEV)
    offs = torch.tensor([0, n // 3, n])
    h1 = hip.hist_build(bins, gh, rows, offs, b, d)
    h2 = hip.hist_build(bins, gh, rows, offs, b, d)
    assert torch.equal(h1, h2)


def test_tree_fit_deterministic():
    """Two identical fits on GPU produce identical predictions (tested at
    the estimator level: split decisions + leaf values reproduce)."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(100000, 24, k=2, seed=44, device=DEV)
    m1 = sea.GBMClassifier().setNumBaseLearners(3).setSeed(9).fit(df)
    m2 = sea.GBMClassifier().setNumBaseLearners(3).setSeed(9).fit(df)
    r1 = m1.transform(df)["rawPrediction"]
    r2 = m2.transform(df)["rawPrediction"]
    assert torch.equal(r1, r2)


def test_hist_build_wide_multiclass_chunked(hip, ref):
    """K > 7 one-hot channels exceed the kernel's 8-channel cap; dispatch
    chunks the signed channels and reassembles (letter-style 26-class
    trees on GPU go through this path)."""
    g = torch.Generator().manual_seed(51)
    n, f, b, d = 20000, 9, 32, 12
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8).to(DEV)
    gh = torch.cat(
        [torch.randn(n, d, generator=g), torch.rand(n, 1, generator=g)], dim=1
    ).to(DEV)
    rows = torch.arange(n, dtype=torch.int32).to(DEV)
    offs = torch.tensor([0, 8000, n])
    got = hip.hist_build(bins, gh, rows, offs, b, d)
    want = ref.hist_build(bins.cpu(), gh.cpu(), rows.cpu(), offs, b)
    assert got.shape == (2, f, b, d + 1)
    assert torch.allclose(got.cpu(), want, atol=2e-2, rtol=1e-3)


def test_wide_multiclass_tree_gpu():
    from spark_ensemble_amd.models import DecisionTreeClassifier
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(40000, 16, k=12, seed=8, device=DEV)
    m = DecisionTreeClassifier().setMaxDepth(6).fit(df)
    acc = float((m.transform(df)["prediction"] == df["label"]).float().mean())
    assert acc > 1.5 / 12, acc


def test_gpu_model_save_load_roundtrip(tmp_path):
    """Models fit on GPU must save/load (MLlib layout) and reproduce
    transform outputs exactly after reload."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(30000, 16, k=2, seed=17, device=DEV)
    m = sea.GBMClassifier().setLoss("bernoulli").setNumBaseLearners(4).fit(df)
    p = str(tmp_path / "m")
    m.save(p)
    m2 = sea.GBMClassificationModel.load(p)
    a = m.transform(df)["rawPrediction"].cpu()
    b = m2.transform(df)["rawPrediction"].cpu()
    assert torch.allclose(a, b, rtol=1e-6, atol=1e-7)

    bag = sea.BaggingRegressor().setNumBaseLearners(3).setSubspaceRatio(0.6).fit(
        synthetic_regression_gpu()
    )
    p2 = str(tmp_path / "bag")
    bag.save(p2)
    bag2 = sea.BaggingRegressionModel.load(p2)
    x = synthetic_regression_gpu()["features"]
    assert torch.allclose(bag.predict(x).cpu(), bag2.predict(x).cpu(),
                          rtol=1e-6, atol=1e-7)


def synthetic_regression_gpu():
    from spark_ensemble_amd.utils.io import synthetic_regression

    return synthetic_regression(20000, 12, seed=23, device=DEV)


def test_gpu_checkpoint_resume(tmp_path, monkeypatch):
    """Resume a CRASHED GBM fit on GPU: saved (CPU) stage models must
    replay cleanly against device tensors.  (A completed fit clears its
    own checkpoint, so the crash is injected mid-fit.)"""
    import os

    import spark_ensemble_amd as sea
    from spark_ensemble_amd.utils.instrumentation import Instrumentation
    from spark_ensemble_amd.utils.io import synthetic_regression

    df = synthetic_regression(50000, 16, seed=19, device=DEV)

    def mk(ck):
        e = sea.GBMRegressor().setNumBaseLearners(4).setSeed(4)
        if ck:
            e.setCheckpointInterval(2).setCheckpointDir(str(tmp_path / "gk"))
        return e

    m_full = mk(False).fit(df)

    class Crash(Exception):
        pass

    orig = Instrumentation.log_round

    def patched(self, i, **kw):
        orig(self, i, **kw)
        if i >= 2:
            raise Crash()

    monkeypatch.setattr(Instrumentation, "log_round", patched)
    with pytest.raises(Crash):
        mk(True).fit(df)
    monkeypatch.undo()
    assert os.path.exists(tmp_path / "gk" / "state.json")

    m_res = mk(True).fit(df)
    a = m_full.predict(df["features"])
    b = m_res.predict(df["features"])
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-5)
    assert not os.path.exists(tmp_path / "gk" / "state.json")


def _rand_complete_tree(depth, F, D, gen):
    """A random but VALID complete binary tree in flat node-array form
    (BFS order: node i's children at 2i+1, 2i+2)."""
    n_internal = 2 ** depth - 1
    n_nodes = 2 ** (depth + 1) - 1
    feature = torch.full((n_nodes,), -1, dtype=torch.int32)
    feature[:n_internal] = torch.randint(0, F, (n_internal,), generator=gen)
    threshold = torch.zeros(n_nodes)
    threshold[:n_internal] = torch.randn(n_internal, generator=gen)
    left = torch.full((n_nodes,), -1, dtype=torch.int32)
    left[:n_internal] = 2 * torch.arange(n_internal, dtype=torch.int32) + 1
    leaf = torch.randn(n_nodes, D, generator=gen)
    return {"feature": feature, "threshold": threshold,
            "left_child": left, "leaf_value": leaf}


@pytest.mark.parametrize("depth,T,D", [(9, 40, 1), (6, 30, 3)])
def test_forest_predict2_multigroup_matches_reference(hip, ref, depth, T, D):
    """The LDS-staged v2 serving kernel: deep trees spanning MULTIPLE
    16Ki-node LDS groups (depth 9 x 40 trees = 40,920 nodes = 3 groups)
    and the D > 1 global-leaf path must match the torch reference."""
    g = torch.Generator().manual_seed(77)
    F = 20
    x = torch.randn(30000, F, generator=g).to(DEV)
    trees = [_rand_complete_tree(depth, F, D, g) for _ in range(T)]
    w = torch.rand(T, generator=g) + 0.5
    got = hip.forest_predict(x, [
        {k: v.to(DEV) for k, v in t.items()} for t in trees
    ], w.to(DEV))
    want = ref.forest_predict(x.cpu(), trees, w)
    assert torch.allclose(got.cpu(), want, rtol=1e-4, atol=1e-4)


def test_hist_build_weighted_wide_multiclass(hip, ref):
    """weighted K >= 7 one-hot channels (2-channel
    nonneg tail) previously recursed forever in the C > 8 chunking."""
    g = torch.Generator().manual_seed(61)
    n, f, b, d = 15000, 9, 32, 9
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8).to(DEV)
    # d signed grads + hess + count (non-unit weights -> 2-wide tail)
    gh = torch.cat(
        [torch.randn(n, d, generator=g), torch.rand(n, 2, generator=g)], dim=1
    ).to(DEV)
    rows = torch.arange(n, dtype=torch.int32).to(DEV)
    offs = torch.tensor([0, 6000, n])
    got = hip.hist_build(bins, gh, rows, offs, b, d)
    want = ref.hist_build(bins.cpu(), gh.cpu(), rows.cpu(), offs, b)
    assert got.shape == (2, f, b, d + 2)
    assert torch.allclose(got.cpu(), want, atol=2e-2, rtol=1e-3)


def test_parallel_fits_match_sequential():
    """parallelism > 1 (per-thread HIP streams) must produce the same
    models as sequential fits (reference HasParallelism semantics: the
    thread pool changes scheduling, never results)."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.models import DecisionTreeRegressor, LinearRegression
    from spark_ensemble_amd.utils.io import synthetic_regression

    df = synthetic_regression(200000, 32, seed=41, device=DEV)
    x = df["features"]

    def bag(par):
        return (
            sea.BaggingRegressor()
            .setBaseLearner(DecisionTreeRegressor().setMaxDepth(6))
            .setNumBaseLearners(6)
            .setSubsampleRatio(0.8)
            .setReplacement(True)
            .setParallelism(par)
            .setSeed(5)
            .fit(df)
        )

    a = bag(1).predict(x)
    b = bag(4).predict(x)
    assert torch.equal(a, b)

    def stack(par):
        return (
            sea.StackingRegressor()
            .setBaseLearners([
                DecisionTreeRegressor().setMaxDepth(5),
                sea.GBMRegressor().setNumBaseLearners(3),
            ])
            .setStacker(LinearRegression())
            .setNumFolds(3)
            .setParallelism(par)
            .setSeed(2)
            .fit(df)
        )

    sa = stack(1).predict(x)
    sb = stack(4).predict(x)
    assert torch.allclose(sa, sb, rtol=1e-5, atol=1e-6)


def test_fused_multiclass_round_matches_sequential():
    """The fused K-tree GBM round (grow_forest) must reproduce the
    sequential per-class fits (same trees, same margins)."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(200000, 24, k=4, seed=33, device=DEV)

    m_fused = sea.GBMClassifier().setLoss("logloss").setNumBaseLearners(3) \
        .setSeed(9).fit(df)
    est_seq = sea.GBMClassifier().setLoss("logloss").setNumBaseLearners(3) \
        .setSeed(9)

    # force the sequential path by patching the eligibility method
    import spark_ensemble_amd.classification.gbm as gbm_mod
    orig = gbm_mod.GBMClassifier._can_fuse_round
    gbm_mod.GBMClassifier._can_fuse_round = lambda self, l, w, st: False
    try:
        m_seq = est_seq.fit(df)
    finally:
        gbm_mod.GBMClassifier._can_fuse_round = orig

    # exact tree-level parity is CPU-proven (test_forest_grower); on GPU
    # the fused round quantizes with different chunk sizes/scales than K
    # sequential fits (T*N vs N rows per launch), so near-tie splits can
    # legally flip.  Assert QUALITY equivalence: same accuracy and same
    # train loss to within a fraction of a percent.
    out_f = m_fused.transform(df)
    out_s = m_seq.transform(df)
    acc_f = float((out_f["prediction"] == df["label"]).float().mean())
    acc_s = float((out_s["prediction"] == df["label"]).float().mean())
    assert abs(acc_f - acc_s) < 0.015, (acc_f, acc_s)
    y = df["label"].long()
    nll_f = float(torch.nn.functional.nll_loss(
        out_f["probability"].clamp_min(1e-12).log(), y))
    nll_s = float(torch.nn.functional.nll_loss(
        out_s["probability"].clamp_min(1e-12).log(), y))
    assert abs(nll_f - nll_s) / max(nll_s, 1e-6) < 0.02, (nll_f, nll_s)
    # and the fused path must agree on the vast majority of rows
    agree = float((out_f["prediction"] == out_s["prediction"]).float().mean())
    assert agree > 0.95, agree


@pytest.mark.parametrize("voting", ["soft", "hard"])
def test_bagging_vote_packed_matches_loop(voting):
    """Classification bagging predictRaw: the packed forest path (leaf
    transforms: normalized probs / one-hot argmax) must exactly match the
    per-member loop."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(60000, 24, k=3, seed=29, device=DEV)
    bag = (
        sea.BaggingClassifier()
        .setNumBaseLearners(6)
        .setSubspaceRatio(0.6)
        .setSubsampleRatio(0.8)
        .setVotingStrategy(voting)
        .setSeed(4)
        .fit(df)
    )
    x = df["features"]
    fast = bag.predictRaw(x)

    # force the loop fallback by hiding the packed path
    from spark_ensemble_amd.ensemble import utils as eutils

    orig = eutils.packed_forest_vote
    eutils.packed_forest_vote = lambda *a, **k: None
    try:
        slow = bag.predictRaw(x)
    finally:
        eutils.packed_forest_vote = orig
    assert torch.allclose(fast, slow, rtol=1e-5, atol=1e-5), \
        float((fast - slow).abs().max())


@pytest.mark.parametrize("n,f", [(4096, 256), (1000, 37), (64, 64), (70, 5)])
def test_transpose_u8_matches_torch(hip, n, f):
    import spark_ensemble_amd._hip_ops as m

    g = torch.Generator().manual_seed(13)
    x = torch.randint(0, 256, (n, f), generator=g, dtype=torch.uint8).to(DEV)
    out = torch.empty(f, n, dtype=torch.uint8, device=DEV)
    m.transpose_u8(out, x)
    assert torch.equal(out, x.t().contiguous())


def test_letter_shape_26class_gbm_gpu():
    """Letter-shape 26-class logloss GBM: the fused K-tree round grows 26
    trees per boosting round level-synchronously on the HIP path and the
    model must clearly beat the class prior."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(60000, 16, k=26, seed=6, device=DEV)
    m = (
        sea.GBMClassifier()
        .setLoss("logloss")
        .setNumBaseLearners(2)
        .setLearningRate(0.5)
        .setSeed(3)
        .fit(df)
    )
    acc = float((m.transform(df)["prediction"] == df["label"]).float().mean())
    assert acc > 0.3, acc  # prior ~ 1/26


def test_weighted_wide_multiclass_tree_gpu():
    """End-to-end: a weighted 8-class gini tree (BoostingClassifier's
    reweighted rounds hit exactly this shape)."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(30000, 12, k=8, seed=13, device=DEV)
    m = sea.BoostingClassifier().setNumBaseLearners(3).fit(df)
    acc = float((m.transform(df)["prediction"] == df["label"]).float().mean())
    assert acc > 1.5 / 8, acc


@pytest.mark.gpu
def test_gather_ranges_kernel_matches_cat():
    from spark_ensemble_amd.ops import dispatch

    g = torch.Generator().manual_seed(3)
    src = torch.randint(0, 1 << 30, (300_000,), generator=g,
                        dtype=torch.int32).cuda()
    starts = torch.tensor([0, 1000, 250_000, 123, 299_999], dtype=torch.int64)
    lens = torch.tensor([1000, 0, 50_000, 77, 1], dtype=torch.int64)
    out = dispatch.gather_ranges(src, starts, lens)
    ref = torch.cat([src[int(s):int(s) + int(l)]
                     for s, l in zip(starts.tolist(), lens.tolist()) if l])
    assert torch.equal(out, ref)


@pytest.mark.gpu
def test_leaf_scatter_kernel_matches_eager():
    from spark_ensemble_amd.ops import dispatch

    g = torch.Generator().manual_seed(4)
    n, t_trees = 100_000, 3
    row_idx = torch.randperm(n, generator=g).to(torch.int32).cuda()
    tp = torch.zeros(n, t_trees, device="cuda")
    starts = torch.tensor([0, 40_000, 70_000], dtype=torch.int64)
    lens = torch.tensor([40_000, 30_000, 30_000], dtype=torch.int64)
    tree = torch.tensor([0, 2, 2], dtype=torch.int64)
    val = torch.tensor([1.5, -2.0, 3.0])
    dispatch.leaf_scatter(tp, row_idx, starts, lens, tree, val)
    ref = torch.zeros(n, t_trees, device="cuda")
    for s, l, tr, v in zip(starts.tolist(), lens.tolist(),
                           tree.tolist(), val.tolist()):
        ref[row_idx[s:s + l].long(), tr] = v
    assert torch.equal(tp, ref)


@pytest.mark.gpu
def test_newton_chain_matches_host_loop():
    """Device-chained Newton == the host safeguarded loop on the same
    bernoulli stage-weight problem."""
    from spark_ensemble_amd.boosting import line_search as ls
    from spark_ensemble_amd.boosting.losses import get_classification_loss

    g = torch.Generator().manual_seed(5)
    n = 200_000
    y = (torch.rand(n, generator=g) > 0.5).float() * 2 - 1
    pred = torch.randn(n, 1, generator=g) * 0.3
    direction = torch.randn(n, 1, generator=g) * 0.1 + y.unsqueeze(1) * 0.2
    w = torch.ones(n)
    loss = get_classification_loss("bernoulli", 2)
    ylab = loss.encode_label(((y > 0).float()))
    a_gpu = ls.optimize_weight_1d(
        loss, ylab.cuda(), pred.cuda(), direction.cuda(), w.cuda(),
        None, 100, 1e-6)
    # host loop on CPU tensors (same math path, f64 host arithmetic)
    a_cpu = ls.optimize_weight_1d(
        loss, ylab, pred, direction, w, None, 100, 1e-6)
    assert abs(a_gpu - a_cpu) < 5e-3, (a_gpu, a_cpu)


@pytest.mark.gpu
def test_partition_transposed_matches_rowmajor():
    """partition through the cached [F, N] transpose == row-major path."""
    from spark_ensemble_amd.ops import dispatch

    g = torch.Generator().manual_seed(6)
    n, f = 200_000, 32
    bins = torch.randint(0, 256, (n, f), generator=g,
                         dtype=torch.uint8).cuda()
    row_idx = torch.arange(n, dtype=torch.int32, device="cuda")
    offs = torch.tensor([0, n // 3, n], dtype=torch.int64)
    feat = torch.tensor([4, -1], dtype=torch.int32, device="cuda")
    thr = torch.tensor([100, 0], dtype=torch.int32, device="cuda")
    new_rows, offs2, lc = dispatch.partition_rows(
        bins, row_idx, offs, feat, thr)
    # reference decision on host
    b0 = bins[:n // 3, 4].cpu()
    left0 = set((b0 <= 100).nonzero(as_tuple=True)[0].tolist())
    got_left = set(new_rows[:int(lc[0])].cpu().tolist())
    assert got_left == left0
    # unsplit node (-1): everything goes left, order preserved
    assert int(lc[1]) == n - n // 3


@pytest.mark.gpu
def test_deep_tree_gbm_large():
    """Depth-12 GBM at 5M rows: per-level descriptor tables outgrow the
    pinned-staging minimum, exercising the slot-growth / reuse path that
    raced before the ping-pong fix (GPU memory fault postmortem in
    profiles/r02_summary.md)."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.models import DecisionTreeRegressor
    from spark_ensemble_amd.utils.io import synthetic_regression

    df = synthetic_regression(5_000_000, 64, seed=21, device="cuda:0")
    m = (sea.GBMRegressor().setNumBaseLearners(2)
         .setBaseLearner(DecisionTreeRegressor().setMaxDepth(12)
                         .setMaxBins(256))
         .fit(df))
    p = m.predict(df["features"])
    assert torch.isfinite(p).all()
    assert float(((p - df["label"]) ** 2).mean()) < float(df["label"].var())
