"""Per-row feature contributions (path-dependent TreeSHAP): the reference
op against a brute-force Shapley oracle, the node covers the growers record,
and ``predictContrib`` of every tree-based model (docs/contributions.md)."""

import itertools
import math

import pytest
import torch

from spark_ensemble_amd import (
    BaggingClassifier,
    BaggingRegressor,
    GBMClassifier,
    GBMRegressor,
)
from spark_ensemble_amd.frame import TensorFrame
from spark_ensemble_amd.models import DecisionTreeClassifier, DecisionTreeRegressor
from spark_ensemble_amd.models.dummy import DummyRegressionModel
from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.ops import reference


# ---------------------------------------------------------------------------
# hand-built trees: spec = (value(s), cover) for a leaf,
# (feature, threshold, left_spec, right_spec) for a split
# ---------------------------------------------------------------------------


def build_tree(spec):
    feat, thr, left, leaf, cov = [], [], [], [], []

    def alloc():
        feat.append(-1); thr.append(0.0); left.append(-1)
        leaf.append(None); cov.append(0.0)
        return len(feat) - 1

    def fill(nid, sp):
        if len(sp) == 2:
            v, c = sp
            leaf[nid] = [float(u) for u in (v if isinstance(v, (list, tuple)) else [v])]
            cov[nid] = float(c)
            return cov[nid]
        f, t, ls, rs = sp
        l = alloc()
        r = alloc()
        assert r == l + 1
        feat[nid], thr[nid], left[nid] = f, float(t), l
        cov[nid] = fill(l, ls) + fill(r, rs)
        return cov[nid]

    fill(alloc(), spec)
    d = len(next(v for v in leaf if v is not None))
    return {
        "feature": torch.tensor(feat, dtype=torch.int32),
        "threshold": torch.tensor(thr, dtype=torch.float32),
        "left_child": torch.tensor(left, dtype=torch.int32),
        "leaf_value": torch.tensor(
            [v if v is not None else [0.0] * d for v in leaf],
            dtype=torch.float32),
        "node_weight": torch.tensor(cov, dtype=torch.float32),
    }


STUMP = (1, 0.5, (1.0, 4), (3.0, 6))
SINGLE_LEAF = (2.5, 7)
# root -> left -> left -> left -> left tests feature 0 three times
DEEP_REPEAT = (
    0, 0.5,
    (1, 0.0,
     (0, -0.5,
      (2, 0.25,
       (0, -1.0, (4.0, 3), (-2.0, 5)),
       (1.5, 2)),
      (0.5, 7)),
     (3, 0.75, (-1.0, 4), (2.0, 1))),
    (2, -0.25, (3.5, 6), (1, 1.0, (-0.5, 2), (6.0, 9))),
)
FOREST3 = [
    (0, 0.5, (1, -0.5, (1.0, 2), (2.0, 5)), (3, 0.0, (-1.0, 3), (4.0, 4))),
    (2, 0.0, (0.5, 6), (0, 0.5, (1, 0.5, (-3.0, 1), (2.5, 2)), (1.0, 8))),
    (4, 1.0, (9.0, 3), (-9.0, 3)),
]


# ---------------------------------------------------------------------------
# brute-force oracle: Shapley sum over all 2^F subsets of the value function
# E(x, S) evaluated recursively in float64 -- no path code involved
# ---------------------------------------------------------------------------


def _value(tree, x, in_s, nid=0):
    f = tree["f"][nid]
    if f < 0:
        return tree["v"][nid]
    l = tree["l"][nid]
    if in_s[f]:
        return _value(tree, x, in_s, l if x[f] <= tree["t"][nid] else l + 1)
    cl, cr = tree["c"][l], tree["c"][l + 1]
    el = _value(tree, x, in_s, l)
    er = _value(tree, x, in_s, l + 1)
    return [(cl * a + cr * b) / (cl + cr) for a, b in zip(el, er)]


def brute_force(x, trees, weights, planes, num_planes):
    x = x.double()
    n, nf = x.shape
    out = torch.zeros(n, num_planes, nf + 1, dtype=torch.float64)
    fact = [math.factorial(i) for i in range(nf + 1)]
    for tree, w, pl in zip(trees, weights, planes):
        t = {
            "f": tree["feature"].tolist(),
            "t": tree["threshold"].double().tolist(),
            "l": tree["left_child"].tolist(),
            "v": tree["leaf_value"].double().tolist(),
            "c": tree["node_weight"].double().tolist(),
        }
        d = len(t["v"][0])
        for r in range(n):
            xr = x[r].tolist()
            val = {}
            for bits in itertools.product((False, True), repeat=nf):
                val[bits] = _value(t, xr, bits)
            for k in range(d):
                out[r, pl + k, nf] += w * val[(False,) * nf][k]
            for i in range(nf):
                for bits, e0 in val.items():
                    if bits[i]:
                        continue
                    s = sum(bits)
                    wgt = fact[s] * fact[nf - s - 1] / fact[nf]
                    e1 = val[bits[:i] + (True,) + bits[i + 1:]]
                    for k in range(d):
                        out[r, pl + k, i] += w * wgt * (e1[k] - e0[k])
    return out


def _rows_on_thresholds(trees, nf, n_random, seed):
    """Random rows plus, for every split, a row sitting exactly on its
    threshold (x == thr goes left)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_random, nf, generator=g, dtype=torch.float64)
    extra = []
    for tree in trees:
        for f, t in zip(tree["feature"].tolist(), tree["threshold"].tolist()):
            if f >= 0:
                row = torch.randn(nf, generator=g, dtype=torch.float64)
                row[f] = t
                extra.append(row)
    return torch.cat([x, torch.stack(extra)]) if extra else x


def _assert_matches_brute(trees, weights, planes, num_planes, nf, seed):
    x = _rows_on_thresholds(trees, nf, 6, seed)
    got = reference.forest_contrib(x, trees, weights, planes, num_planes)
    assert got.dtype == torch.float64
    want = brute_force(x, trees, weights, planes, num_planes)
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"brute force: err={err:.3e} scale={scale:.3e}")
    assert err <= 1e-9 * scale
    return x, got


@pytest.mark.parametrize("spec,nf", [
    (STUMP, 3), (SINGLE_LEAF, 2), (DEEP_REPEAT, 4),
], ids=["stump", "single_leaf", "deep_repeat"])
def test_reference_matches_brute_force_single_tree(spec, nf):
    tree = build_tree(spec)
    x, got = _assert_matches_brute([tree], [1.0], [0], 1, nf, seed=3)
    if spec is SINGLE_LEAF:  # only bias
        assert bool((got[:, :, :nf] == 0).all())
        assert bool((got[:, 0, nf] == 2.5).all())
    if spec is DEEP_REPEAT:
        m = [len(e) for _, e in reference._tree_paths(tree)]
        assert max(m) == 3  # five splits, features {0, 1, 2}: 0 merged


def test_reference_matches_brute_force_forest_planes_weights():
    trees = [build_tree(s) for s in FOREST3]
    x, got = _assert_matches_brute(trees, [1.5, -0.5, 0.0], [0, 1, 0], 2, 5,
                                   seed=5)
    # the weight-0 tree (the only one on feature 4) contributes nothing
    assert bool((got[:, :, 4] == 0).all())
    # linear in the weights
    one = reference.forest_contrib(x, trees[:1], [1.0], [0], 2)
    two = reference.forest_contrib(x, trees[1:2], [1.0], [1], 2)
    assert torch.allclose(got, 1.5 * one - 0.5 * two, rtol=0, atol=1e-12)


def test_reference_matches_brute_force_vector_leaves():
    tree = build_tree(
        (0, 0.0, ([0.2, 0.8, 0.0], 3),
         (1, 0.5, ([1.0, 0.0, 0.0], 4), ([0.1, 0.3, 0.6], 2))))
    _assert_matches_brute([tree], [1.0], [0], 3, 3, seed=9)


def test_reference_matches_brute_force_fitted_tree():
    g = torch.Generator().manual_seed(21)
    x = torch.randn(300, 6, generator=g)
    y = x[:, 0] * 2 + (x[:, 1] > 0.3).float() - x[:, 2] * x[:, 3]
    model = DecisionTreeRegressor().setMaxDepth(4).fit(
        TensorFrame(features=x, label=y))
    tree = {k: v.cpu() for k, v in model._tree.items()}
    assert model.numNodes > 7
    xs, got = _assert_matches_brute([tree], [1.0], [0], 1, 6, seed=23)
    pred = model.predict(xs.float()).double()
    assert torch.allclose(got.sum(-1)[:, 0], pred, rtol=0, atol=1e-5)


def test_pack_keeps_degenerate_covers_off_the_kernel():
    """The kernel's fixed-point range and its factors assume what every
    grower emits: positive covers that add up.  Hand-made dicts that break
    this are packed for the reference op only."""
    cpu = torch.device("cpu")
    tree = build_tree(STUMP)
    pack = ops._pack_contrib([tree], [2.0], [0], 1, cpu)
    assert pack["native_ok"]
    # 2 * bound = 2 * 2.0 * 3.0 = 12 maps below 2^50, with a power of two
    assert 12 * pack["scale"] <= 2.0 ** 50 < 24 * pack["scale"]
    assert math.frexp(pack["scale"])[0] == 0.5
    for cov in ([10.0, 9.0, 9.0], [10.0, 0.0, 10.0]):
        bad = dict(tree, node_weight=torch.tensor(cov))
        assert not ops._pack_contrib([bad], [1.0], [0], 1, cpu)["native_ok"]
    # a path over CONTRIB_MAX_PATH unique features: nested right splits
    spec = (1.0, 1)
    for f in range(ops.CONTRIB_MAX_PATH + 1):
        spec = (f, 0.0, (float(f), 1), spec)
    long_tree = build_tree(spec)
    assert not ops._pack_contrib([long_tree], None, None, 1, cpu)["native_ok"]


# ---------------------------------------------------------------------------
# node covers recorded by the growers
# ---------------------------------------------------------------------------


def _check_covers(tree, total, rel=0.0):
    feat = tree["feature"].cpu().tolist()
    left = tree["left_child"].cpu().tolist()
    cov = tree["node_weight"].cpu()
    assert cov.dtype == torch.float32 and cov.numel() == len(feat)
    assert abs(float(cov[0]) - total) <= rel * total
    stack, seen = [0], 0
    while stack:
        nid = stack.pop()
        seen += 1
        assert float(cov[nid]) > 0
        if feat[nid] >= 0:
            l = left[nid]
            both = float(cov[l]) + float(cov[l + 1])
            # children are (left, parent - left) in f32
            assert abs(both - float(cov[nid])) <= 2.0 ** -22 * float(cov[nid])
            stack += [l, l + 1]
    assert seen == len(feat)


def _small_frames():
    g = torch.Generator().manual_seed(31)
    x = torch.randn(500, 5, generator=g)
    y = x[:, 0] - 2 * (x[:, 1] > 0).float() + 0.1 * torch.randn(500, generator=g)
    yc = ((x[:, 0] > 0).long() + (x[:, 2] > 0.5).long()).float()
    w = torch.rand(500, generator=g) + 0.5
    return x, y, yc, w


def test_grower_covers_tree_regressor():
    x, y, _, w = _small_frames()
    m = DecisionTreeRegressor().setMaxDepth(4).fit(TensorFrame(features=x, label=y))
    _check_covers(m._tree, 500.0)
    mw = DecisionTreeRegressor().setMaxDepth(4).setWeightCol("weight").fit(
        TensorFrame(features=x, label=y, weight=w))
    _check_covers(mw._tree, float(w.sum()), rel=1e-6)


def test_grower_covers_tree_classifier():
    x, _, yc, w = _small_frames()
    m = DecisionTreeClassifier().setMaxDepth(4).fit(
        TensorFrame(features=x, label=yc))
    assert m._tree["leaf_value"].shape[1] == 3
    _check_covers(m._tree, 500.0)
    mw = DecisionTreeClassifier().setMaxDepth(4).setWeightCol("weight").fit(
        TensorFrame(features=x, label=yc, weight=w))
    _check_covers(mw._tree, float(w.sum()), rel=1e-6)


def test_grower_covers_loop_grower_wide_leaves():
    """K = 8 classes exceed the arena grower's channel cap on the CPU: the
    loop grower records the covers."""
    x, _, _, w = _small_frames()
    yc = (torch.arange(500) % 8).float()
    m = DecisionTreeClassifier().setMaxDepth(3).fit(
        TensorFrame(features=x, label=yc))
    assert m._tree["leaf_value"].shape[1] == 8
    _check_covers(m._tree, 500.0)


def test_grower_covers_fit_tree_forest():
    from spark_ensemble_amd.models.tree import fit_tree_forest
    from spark_ensemble_amd.models.tree_grower import ensure_binned

    x, y, _, w = _small_frames()
    edges, bins = ensure_binned(None, x, 32)
    labels = torch.stack([y, -y, y * y], dim=1)
    learner = DecisionTreeRegressor().setMaxDepth(3)
    models, _ = fit_tree_forest(learner, edges, bins, labels,
                                torch.ones(500))
    for m in models:
        _check_covers(m._tree, 500.0)
    w2 = torch.stack([w, 2 * w, w + 1], dim=1)
    models, _ = fit_tree_forest(learner, edges, bins, labels, w2)
    for t, m in enumerate(models):
        _check_covers(m._tree, float(w2[:, t].sum()), rel=1e-6)


# ---------------------------------------------------------------------------
# predictContrib: local accuracy, exact zeros, constant bias
# ---------------------------------------------------------------------------


@pytest.fixture
def contrib_calls(monkeypatch):
    """Records the (trees, weights, planes, num_planes) of every
    forest_contrib call the models make."""
    calls = []
    real = ops.forest_contrib

    def spy(x, trees, weights=None, planes=None, num_planes=1, cache=None):
        calls.append((trees, weights, planes, num_planes))
        return real(x, trees, weights, planes, num_planes, cache=cache)

    monkeypatch.setattr(ops, "forest_contrib", spy)
    return calls


def _check_model_contrib(contrib, target, x, calls, extra_bias=0.0):
    """``contrib`` [N, P, F + 1] against ``target`` [N, P].  The tolerance
    is the float32 reference op's own deviation from its float64 run on the
    same inputs (per row, summed over the columns that the row sum adds up),
    times 4."""
    trees, weights, planes, num_planes = calls[-1]
    trees = [{k: v.cpu() for k, v in t.items()} for t in trees]
    xc = x.cpu()
    r32 = reference.forest_contrib(xc.float(), trees, weights, planes, num_planes)
    r64 = reference.forest_contrib(xc.double(), trees, weights, planes, num_planes)
    tol = 4.0 * float((r32.double() - r64).abs().sum(-1).max())
    nf = x.shape[1]
    err = float((contrib.sum(-1).cpu().double() - target.cpu().double()).abs().max())
    print(f"local accuracy: err={err:.3e} tol={tol:.3e}")
    assert contrib.shape == (x.shape[0], num_planes, nf + 1)
    assert err <= tol
    # features no tree splits on get exactly 0.0
    used = set()
    for t in trees:
        used |= {f for f in t["feature"].tolist() if f >= 0}
    unused = [f for f in range(nf) if f not in used]
    if unused:
        assert bool((contrib[:, :, unused] == 0).all())
    # the bias does not depend on the row
    assert bool((contrib[:, :, nf] == contrib[:1, :, nf]).all())
    # and the float64 reference agrees with it
    assert torch.allclose(contrib[0, :, nf].cpu().double() - extra_bias,
                          r64[0, :, nf], rtol=1e-5, atol=1e-6)
    return used


def test_contrib_tree_regressor(reg_frame, reg_frame_test, contrib_calls):
    m = DecisionTreeRegressor().setMaxDepth(5).fit(reg_frame)
    x = reg_frame_test["features"][:256]
    c = m.predictContrib(x)
    assert c.shape == (256, 21)
    _check_model_contrib(c.unsqueeze(1), m.predict(x).unsqueeze(1), x,
                         contrib_calls)


def test_contrib_tree_classifier(clf_frame, clf_frame_test, contrib_calls):
    m = DecisionTreeClassifier().setMaxDepth(5).fit(clf_frame)
    x = clf_frame_test["features"][:256]
    c = m.predictContrib(x)
    _check_model_contrib(c, m.predictRaw(x), x, contrib_calls)


def test_contrib_gbm_regressor(reg_frame, reg_frame_test, contrib_calls):
    m = GBMRegressor().setNumBaseLearners(8).fit(reg_frame)
    x = reg_frame_test["features"][:256]
    c = m.predictContrib(x)
    assert c.shape == (256, 21)
    const = float(m._init._constant)
    _check_model_contrib(c.unsqueeze(1), m.predict(x).unsqueeze(1), x,
                         contrib_calls, extra_bias=const)
    # an init that is itself a tree joins the forest with weight 1
    init_tree = DecisionTreeRegressor().setMaxDepth(2).fit(reg_frame)
    m2 = GBMRegressor().setNumBaseLearners(3).fit(reg_frame)
    m2._init = init_tree
    c2 = m2.predictContrib(x)
    assert len(contrib_calls[-1][0]) == 4
    _check_model_contrib(c2.unsqueeze(1), m2.predict(x).unsqueeze(1), x,
                         contrib_calls)
    m2._init = object()
    with pytest.raises(ValueError, match="init"):
        m2.predictContrib(x)


def test_contrib_gbm_classifier(clf_frame, clf_frame_test, bin_frame,
                                bin_frame_test, contrib_calls):
    m = GBMClassifier().setNumBaseLearners(4).fit(clf_frame)
    x = clf_frame_test["features"][:256]
    c = m.predictContrib(x)
    assert c.shape == (256, m._dim, 21) and m._dim == 3
    _check_model_contrib(c, m._margins(x.float()), x, contrib_calls,
                         extra_bias=m._init._raw[:3].double())
    assert torch.equal(m._margins(x.float()), m.predictRaw(x))
    # binary: one plane, predictRaw = (-s, s)
    b = GBMClassifier().setLoss("bernoulli").setNumBaseLearners(4).fit(bin_frame)
    xb = bin_frame_test["features"][:256]
    cb = b.predictContrib(xb)
    assert cb.shape == (256, 1, 21)
    _check_model_contrib(cb, b._margins(xb.float()), xb, contrib_calls,
                         extra_bias=b._init._raw[:1].double())
    assert torch.equal(b.predictRaw(xb)[:, 1], b._margins(xb.float())[:, 0])


def test_contrib_bagging_regressor_subspaced(reg_frame, reg_frame_test,
                                             contrib_calls):
    m = (
        BaggingRegressor()
        .setBaseLearner(DecisionTreeRegressor().setMaxDepth(3))
        .setNumBaseLearners(4)
        .setSubsampleRatio(0.8)
        .setSubspaceRatio(0.4)
        .fit(reg_frame)
    )
    x = reg_frame_test["features"][:256]
    c = m.predictContrib(x)
    assert c.shape == (256, 21)
    used = _check_model_contrib(c.unsqueeze(1), m.predict(x).unsqueeze(1), x,
                                contrib_calls)
    # contributions are reported in ORIGINAL feature ids: the columns in
    # use are the members' local split features mapped through their
    # subspaces (and at least one member does not see feature 0..k as 0..k)
    want = set()
    for mem, sub in zip(m._models, m._subspaces):
        assert sub.numel() < 20
        want |= {int(sub[f]) for f in mem._tree["feature"].tolist() if f >= 0}
    assert used == want
    local = set()
    for mem in m._models:
        local |= {f for f in mem._tree["feature"].tolist() if f >= 0}
    assert local != want
    nz = {f for f in range(20) if bool((c[:, f] != 0).any())}
    assert nz and nz <= want


@pytest.mark.parametrize("voting", ["soft", "hard"])
def test_contrib_bagging_classifier(clf_frame, clf_frame_test, contrib_calls,
                                    voting):
    m = (
        BaggingClassifier()
        .setBaseLearner(DecisionTreeClassifier().setMaxDepth(4))
        .setNumBaseLearners(4)
        .setSubsampleRatio(0.8)
        .setSubspaceRatio(0.7)
        .setVotingStrategy(voting)
        .fit(clf_frame)
    )
    x = clf_frame_test["features"][:256]
    c = m.predictContrib(x)
    assert c.shape == (256, 3, 21)
    _check_model_contrib(c, m.predictRaw(x), x, contrib_calls)


# ---------------------------------------------------------------------------
# persistence and errors
# ---------------------------------------------------------------------------


def test_contrib_save_load_roundtrip(tmp_path):
    from spark_ensemble_amd import GBMRegressionModel

    x, y, _, _ = _small_frames()
    m = GBMRegressor().setNumBaseLearners(3).fit(TensorFrame(features=x, label=y))
    want = m.predictContrib(x[:64])
    p = str(tmp_path / "gbm")
    m.save(p)
    loaded = GBMRegressionModel.load(p)
    assert "node_weight" in loaded._models[0]._tree
    assert torch.equal(loaded.predictContrib(x[:64]), want)


def test_contrib_without_covers_raises():
    x, y, _, _ = _small_frames()
    m = DecisionTreeRegressor().setMaxDepth(3).fit(TensorFrame(features=x, label=y))
    m._tree = {k: v for k, v in m._tree.items() if k != "node_weight"}
    with pytest.raises(ValueError, match="node_weight"):
        m.predictContrib(x[:8])


def test_contrib_non_tree_member_raises():
    x, y, _, _ = _small_frames()
    m = (
        BaggingRegressor()
        .setBaseLearner(DecisionTreeRegressor().setMaxDepth(2))
        .setNumBaseLearners(3)
        .fit(TensorFrame(features=x, label=y))
    )
    dummy = DummyRegressionModel()
    dummy._constant = 1.0
    m._models = [m._models[0], dummy, m._models[2]]
    with pytest.raises(ValueError, match="DummyRegressionModel"):
        m.predictContrib(x[:8])
