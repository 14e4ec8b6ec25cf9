"""Wide-multiclass (7 <= K <= 32) gini trees on the GPU: the label-indexed
histogram kernel and the wide split kernel against the torch reference,
estimator routing away from the loop grower, grown-tree parity and model
quality on the 26-class letter data."""

import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DATA = os.path.join(os.path.dirname(__file__), "..", "data")


@pytest.fixture(scope="module")
def hip():
    from spark_ensemble_amd.ops import dispatch

    assert dispatch.hip_available(), "HIP extension must be built in-tree"
    return dispatch


@pytest.fixture(scope="module")
def ref():
    from spark_ensemble_amd.ops import reference

    return reference


# ---------------------------------------------------------------------------
# hist_build_class
# ---------------------------------------------------------------------------


def _hist_inputs(n, f, b, k, t_trees, seed, weights):
    g = torch.Generator().manual_seed(seed)
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    label = torch.randint(0, k, (n,), generator=g).to(torch.uint8)
    if weights == "unit":
        w = torch.ones(n, t_trees)
    elif weights == "int":
        w = torch.randint(0, 9, (n, t_trees), generator=g).float()
    else:
        w = torch.rand(n, t_trees, generator=g)
    return bins, label, w, g


def _both(hip, ref, bins, label, w, rows, offs, col0, b, k, nn, **kw):
    want = ref.hist_build_class(bins, label, w, rows, offs, col0, b, k, nn)
    got = hip.hist_build_class(
        bins.to(DEV), label.to(DEV), w.to(DEV), rows.to(DEV), offs, col0, b,
        k, nn, float(w.max()), **kw
    )
    assert got.shape == want.shape
    return got.cpu(), want


def test_hist_class_permuted_rows_and_empty_node(hip, ref):
    n, f, b, k, nn = 30000, 40, 32, 9, 2
    bins, label, w, g = _hist_inputs(n, f, b, k, 1, 1, "int")
    rows = torch.randperm(n, generator=g)[: n - 100].to(torch.int32)
    offs = torch.tensor([0, 9000, 9000, n - 100], dtype=torch.int64)
    col0 = torch.zeros(3, dtype=torch.int32)
    got, want = _both(hip, ref, bins, label, w, rows, offs, col0, b, k, nn)
    assert torch.equal(got, want)
    assert torch.equal(got[1], torch.zeros(f, b, k + nn))  # the empty node
    # both bins sources give the same histogram
    got_rm, _ = _both(hip, ref, bins, label, w, rows, offs, col0, b, k, nn,
                      transposed=False)
    assert torch.equal(got_rm, want)


def test_hist_class_smallest_feature_group(hip, ref):
    # B = 256, K = 32: 64 KiB of LDS per feature -> feature groups of 2,
    # F = 5 is no multiple of it, and the group sits at the 160 KiB cap
    n, f, b, k, nn = 20000, 5, 256, 32, 2
    bins, label, w, g = _hist_inputs(n, f, b, k, 1, 2, "int")
    rows = torch.arange(n, dtype=torch.int32)
    offs = torch.tensor([0, 12000, n], dtype=torch.int64)
    col0 = torch.zeros(2, dtype=torch.int32)
    got, want = _both(hip, ref, bins, label, w, rows, offs, col0, b, k, nn)
    assert torch.equal(got, want)


def test_hist_class_letter_shape_unit_weights(hip, ref):
    n, f, b, k, nn = 15000, 16, 16, 26, 1
    bins, label, w, g = _hist_inputs(n, f, b, k, 1, 3, "unit")
    rows = torch.arange(n, dtype=torch.int32)
    offs = torch.tensor([0, n], dtype=torch.int64)
    col0 = torch.zeros(1, dtype=torch.int32)
    got, want = _both(hip, ref, bins, label, w, rows, offs, col0, b, k, nn,
                      identity_rows=True)
    assert torch.equal(got, want)
    # hess channel doubles as the row count
    assert float(got[0, 0, :, k].sum()) == n


def test_hist_class_multi_chunk_staging_path(hip, ref):
    n, f, b, k, nn = 30000, 8, 32, 9, 2
    bins, label, w, g = _hist_inputs(n, f, b, k, 1, 4, "int")
    rows = torch.randperm(n, generator=g)[:25000].to(torch.int32)
    offs = torch.tensor([0, 25000], dtype=torch.int64)
    col0 = torch.zeros(1, dtype=torch.int32)
    assert "SEA_HIST_OVERSUB" not in os.environ
    got, want = _both(hip, ref, bins, label, w, rows, offs, col0, b, k, nn)
    # the launch reports how many nodes were split into several chunks
    # (i64 staging atomics + decode pass)
    assert hip.last_hist_build_class_info["multi_chunk_nodes"] == 1
    assert torch.equal(got, want)


def test_hist_class_forest_weight_columns(hip, ref):
    n, f, b, k, nn, T = 12000, 10, 32, 26, 2, 3
    bins, label, w, g = _hist_inputs(n, f, b, k, T, 5, "int")
    rows = torch.randperm(n, generator=g).to(torch.int32)
    offs = torch.tensor([0, 3000, 7000, 7500, n], dtype=torch.int64)
    col0 = torch.tensor([0, 2, 1, 2], dtype=torch.int32)
    got, want = _both(hip, ref, bins, label, w, rows, offs, col0, b, k, nn)
    assert torch.equal(got, want)
    assert not torch.equal(got[1], got[3])


def test_hist_class_fractional_weights(hip, ref):
    n, f, b, k, nn = 20000, 12, 64, 26, 2
    bins, label, w, g = _hist_inputs(n, f, b, k, 2, 6, "frac")
    rows = torch.randperm(n, generator=g).to(torch.int32)
    offs = torch.tensor([0, 15000, n], dtype=torch.int64)
    col0 = torch.tensor([1, 0], dtype=torch.int32)
    got, want = _both(hip, ref, bins, label, w, rows, offs, col0, b, k, nn)
    assert torch.allclose(got, want, atol=2e-2, rtol=1e-3)
    assert torch.equal(got[..., k + 1], want[..., k + 1])  # counts are exact


def test_hist_class_deterministic(hip):
    n, f, b, k, nn = 30000, 8, 32, 26, 2
    bins, label, w, g = _hist_inputs(n, f, b, k, 1, 7, "frac")
    rows = torch.randperm(n, generator=g)[:25000].to(torch.int32)
    offs = torch.tensor([0, 25000], dtype=torch.int64)
    col0 = torch.zeros(1, dtype=torch.int32)
    args = (bins.to(DEV), label.to(DEV), w.to(DEV), rows.to(DEV), offs, col0,
            b, k, nn, 1.0)
    a = hip.hist_build_class(*args)
    assert hip.last_hist_build_class_info["multi_chunk_nodes"] == 1
    c = hip.hist_build_class(*args)
    assert torch.equal(a, c)


# ---------------------------------------------------------------------------
# wide split search, straight through the extension
# ---------------------------------------------------------------------------


def _gain64(hist, node, f, b, d, lam):
    h = hist[node, f].double()
    left = h[: b + 1].sum(dim=0)
    tot = h.sum(dim=0)
    right = tot - left

    def score(s):
        return float((s[:d] ** 2).sum() / (s[d] + lam))

    return score(left) + score(right) - score(tot)


@pytest.mark.parametrize("n,f,b,c,d", [(3, 40, 32, 9, 7), (4, 16, 16, 27, 26),
                                       (2, 5, 256, 34, 32),
                                       (2, 7, 100, 28, 26)])
def test_split_argmax_wide_matches_reference(hip, ref, n, f, b, c, d):
    import spark_ensemble_amd._hip_ops as ext

    nn = c - d
    g = torch.Generator().manual_seed(31)
    per = 1500
    rows_n = per * n + 300
    bins = torch.randint(0, b, (rows_n, f), generator=g, dtype=torch.uint8)
    # an extra node whose rows all sit in ONE bin per feature: no valid split
    bins[per * n:] = torch.randint(0, b, (f,), generator=g,
                                   dtype=torch.uint8)
    label = torch.randint(0, d, (rows_n,), generator=g).to(torch.uint8)
    w = (torch.ones(rows_n, 1) if nn == 1
         else torch.randint(1, 5, (rows_n, 1), generator=g).float())
    offs = torch.tensor([i * per for i in range(n + 1)] + [rows_n])
    rows = torch.arange(rows_n, dtype=torch.int32)
    hist = ref.hist_build_class(bins, label, w, rows, offs,
                                torch.zeros(n + 1, dtype=torch.int32), b, d,
                                nn)
    hist[:, 1] = 0.0  # one feature masked out, as the subspace mask does
    hist_gpu = hist.to(DEV).contiguous()
    n1 = n + 1
    lam = 1e-6
    for mig, mcw in [(0.0, 0.0), (0.05, 0.3)]:
        gain = torch.empty(n1, dtype=torch.float32, device=DEV)
        feat = torch.empty(n1, dtype=torch.int32, device=DEV)
        bin_ = torch.empty(n1, dtype=torch.int32, device=DEV)
        ls = torch.empty(n1, c, dtype=torch.float32, device=DEV)
        ext.split_argmax(gain, feat, bin_, ls, hist_gpu, d, lam, mcw, 1.0,
                         mig)
        gg, gf, gb, gls = gain.cpu(), feat.cpu(), bin_.cpu(), ls.cpu()
        wg, wf, wb, wls = ref.split_search(hist, lam, mcw, 1.0, mig, d_dims=d)
        fin = torch.isfinite(wg)
        assert torch.equal(torch.isfinite(gg), fin)
        assert bool(fin[:n].all()) and not bool(fin[n])
        assert torch.allclose(gg[fin], wg[fin], rtol=1e-3, atol=1e-4)
        # no-split contract
        assert int(gf[n]) == -1 and int(gb[n]) == -1
        assert torch.equal(gls[n], torch.zeros(c))
        cum = hist.double().cumsum(dim=2)
        for i in range(n):
            fi, bi = int(gf[i]), int(gb[i])
            assert fi != 1 and 0 <= fi < f and 0 <= bi < b - 1
            assert torch.allclose(gls[i].double(), cum[i, fi, bi], rtol=1e-4,
                                  atol=1e-4)
            # near-ties may pick another (feat, bin); its float64 gain must
            # still be the reference best within the gain tolerance
            chosen = _gain64(hist, i, fi, bi, d, lam)
            best = float(wg[i])
            assert abs(chosen - best) <= 1e-4 + 1e-3 * abs(best), (
                i, fi, bi, chosen, best)


# ---------------------------------------------------------------------------
# routing, parity, quality
# ---------------------------------------------------------------------------


@pytest.fixture(scope="module")
def letter_gpu():
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.utils.io import load_libsvm

    df = load_libsvm(os.path.join(DATA, "letter", "letter.svm"))
    n = df["features"].shape[0]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(5))
    cut = int(n * 0.75)

    def part(idx):
        return TensorFrame({
            "features": df["features"][idx].to(DEV),
            "label": (df["label"][idx] - 1.0).to(DEV),  # 1..26 -> 0..25
        })

    return part(perm[:cut]), part(perm[cut:])


def _acc(model, te):
    return float((model.transform(te)["prediction"] == te["label"])
                 .float().mean())


def _no_loop_grower(*a, **kw):
    raise AssertionError("_grow_tree_seq entered")


@pytest.fixture(scope="module")
def letter_models(letter_gpu):
    """Depth-6 tree and 8-member bag on letter, fitted with the loop
    grower disabled: both must route through the class mode."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.models import DecisionTreeClassifier, tree_grower

    tr, _ = letter_gpu
    mp = pytest.MonkeyPatch()
    mp.setattr(tree_grower, "_grow_tree_seq", _no_loop_grower)
    try:
        single = DecisionTreeClassifier().setMaxDepth(6).fit(tr)
        bag = (
            sea.BaggingClassifier()
            .setBaseLearner(DecisionTreeClassifier().setMaxDepth(6))
            .setNumBaseLearners(8)
            .setSubspaceRatio(0.8)
            .setReplacement(True)
            .setSeed(9)
            .fit(tr)
        )
    finally:
        mp.undo()
    return single, bag


def test_letter_fits_avoid_loop_grower(letter_models, letter_gpu):
    single, bag = letter_models
    tr, _ = letter_gpu
    assert single.numNodes > 31
    assert bag.numModels == 8
    assert _acc(single, tr) > 0.3  # 26 classes: prior is 0.04


def test_letter_bagging_beats_single_tree_class_mode(letter_models,
                                                     letter_gpu):
    single, bag = letter_models
    _, te = letter_gpu
    bag_acc, single_acc = _acc(bag, te), _acc(single, te)
    assert bag_acc > single_acc, (bag_acc, single_acc)


def test_k40_keeps_loop_grower(monkeypatch):
    from spark_ensemble_amd.models import DecisionTreeClassifier, tree_grower
    from spark_ensemble_amd.utils.io import synthetic_classification

    calls = []
    orig = tree_grower._grow_tree_seq

    def spy(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    monkeypatch.setattr(tree_grower, "_grow_tree_seq", spy)
    df = synthetic_classification(6000, 12, k=40, seed=3, device=DEV)
    model = DecisionTreeClassifier().setMaxDepth(4).fit(df)
    assert calls and model.numNodes >= 3


def test_class_mode_tree_matches_loop_grower_gpu(ref):
    from spark_ensemble_amd.models.tree_grower import (
        GrowParams, _grow_tree_seq, grow_forest,
    )
    from spark_ensemble_amd.ops import dispatch

    n, f, b, k = 15000, 16, 32, 26
    g = torch.Generator().manual_seed(41)
    x = torch.randn(n, f, generator=g)
    score = x[:, 0] + 0.7 * x[:, 1] - 0.5 * x[:, 2] * x[:, 3]
    score = score + 0.3 * torch.randn(n, generator=g)
    cuts = torch.quantile(score, torch.arange(1, k) / k)
    label = torch.bucketize(score, cuts).clamp_(0, k - 1)
    edges = ref.quantile_bins(x, b)
    bins = ref.bin_features(x, edges)
    x, edges, bins, label = (t.to(DEV) for t in (x, edges, bins, label))
    w = torch.ones(n, device=DEV)
    params = GrowParams(max_depth=6, max_bins=b)
    onehot = torch.zeros(n, k, device=DEV)
    onehot.scatter_(1, label.unsqueeze(1), 1.0)

    seq = _grow_tree_seq(bins, edges, onehot, w, params)
    cls = grow_forest(bins, edges, None, w, params, class_labels=label,
                      num_classes=k)[0]

    def pred(t):
        return dispatch.tree_predict(
            x, t["feature"], t["threshold"], t["left_child"],
            t["leaf_value"], 64).argmax(dim=1)

    agree = float((pred(seq) == pred(cls)).float().mean())
    assert agree > 0.98, agree
