"""The fused tree-level path against the composed ops it replaces.

``SEA_LEVEL_FUSED=0`` keeps the level loop on the ops it had before
(assemble + ``split_search`` + cat, device-side left counts); that run is the
oracle.  The fused
kernels do the same f32 operations in the same order, so every comparison is
``torch.equal``: there are no tolerances."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from spark_ensemble_amd.ops import dispatch

    assert dispatch.hip_available(), "HIP extension must be built in-tree"
    return dispatch


def _d_of(c):
    return 1 if c <= 3 else c - 2


def _rand_hist(g, n, f, b, c):
    """Signed gradient channels, non-negative hess / count channels."""
    d = _d_of(c)
    h = torch.randn(n, f, b, c, generator=g)
    h[..., d:] = torch.randint(0, 21, (n, f, b, c - d), generator=g).float()
    return h


def _level_case(g, f, b, c, built_nodes, derived, n_prev):
    """``built_nodes``: active indices that are built (their rows in ``built``
    follow that order); ``derived``: {active index: parent row}.  A parent is
    its two children's sum, so the derived counts stay non-negative."""
    n = len(built_nodes) + len(derived)
    built = _rand_hist(g, len(built_nodes), f, b, c)
    brow = {j: i for i, j in enumerate(built_nodes)}
    table = torch.full((n, 3), -1, dtype=torch.int32)
    for j, i in brow.items():
        table[j, 0] = i
    parent = _rand_hist(g, n_prev, f, b, c) if n_prev else None
    for j, p in derived.items():
        parent[p] = built[brow[j ^ 1]] + _rand_hist(g, 1, f, b, c)[0]
        table[j, 1] = p
        table[j, 2] = brow[j ^ 1]
    return built, parent, table


def _both(hip, monkeypatch, built, parent, table, **kw):
    """(fused, composed) outputs on the GPU."""
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("SEA_LEVEL_FUSED", flag)
        b = built.to(DEV).clone()
        p = parent.to(DEV) if parent is not None else None
        level, pack, feat, bin_ = hip.level_split(b, p, table, **kw)
        torch.cuda.synchronize()
        outs.append((level, pack, feat, bin_, b))
    return outs


def _assert_same(outs, n, c):
    (lv, pk, ft, bn, _), (lv0, pk0, ft0, bn0, _) = outs
    assert torch.equal(lv, lv0)
    gain, gain0 = pk[:n], pk0[:n]
    assert torch.equal(gain, gain0)
    assert torch.equal(pk[n:2 * n], pk0[n:2 * n])          # feat as f32
    assert torch.equal(pk[2 * n:3 * n], pk0[2 * n:3 * n])  # bin as f32
    assert torch.equal(pk[3 * n:], pk0[3 * n:])            # left_stats
    assert pk.numel() == n * (3 + c)
    assert ft.dtype == torch.int32 and bn.dtype == torch.int32
    assert torch.equal(ft, ft0) and torch.equal(bn, bn0)
    assert torch.equal(ft.float(), pk[n:2 * n])
    assert torch.equal(bn.float(), pk[2 * n:3 * n])


SIX = dict(built_nodes=[0, 3, 4], derived={1: 1, 2: 3, 5: 4}, n_prev=5)


@pytest.mark.parametrize("c", [2, 3, 8])
@pytest.mark.parametrize("b", [2, 3, 64, 65, 255, 256])
@pytest.mark.parametrize("f", [1, 5, 64])
def test_level_split_mixed_level(hip, monkeypatch, f, b, c):
    """6 active nodes, 3 built and 3 derived, parents {1, 3, 4} of an
    uncompacted 5-row previous level."""
    g = torch.Generator().manual_seed(1000 * f + 10 * b + c)
    built, parent, table = _level_case(g, f, b, c, **SIX)
    outs = _both(hip, monkeypatch, built, parent, table, d_dims=_d_of(c))
    _assert_same(outs, 6, c)
    assert bool(torch.isfinite(outs[0][1][:6]).any())


@pytest.mark.parametrize("c", [2, 3, 8])
def test_level_split_all_built(hip, monkeypatch, c):
    g = torch.Generator().manual_seed(7)
    built, parent, table = _level_case(g, 5, 65, c, [0, 1, 2, 3], {}, 2)
    outs = _both(hip, monkeypatch, built, parent, table, d_dims=_d_of(c))
    _assert_same(outs, 4, c)
    assert torch.equal(outs[0][0], built.to(DEV))


@pytest.mark.parametrize("n", [1, 3])
def test_level_split_root_aliases_built(hip, monkeypatch, n):
    """At the root (no parent, identity table) ``level`` is ``built`` itself,
    unchanged; n = 1 is also the one-node case."""
    g = torch.Generator().manual_seed(8)
    built, _, table = _level_case(g, 5, 65, 3, list(range(n)), {}, 0)
    outs = _both(hip, monkeypatch, built, None, table, d_dims=1)
    _assert_same(outs, n, 3)
    level, _, _, _, b_in = outs[0]
    assert level.data_ptr() == b_in.data_ptr()
    assert torch.equal(level, built.to(DEV))


def test_level_split_zero_row_node(hip, monkeypatch):
    """An all-zero histogram (a node without rows): gain -inf, feat -1."""
    g = torch.Generator().manual_seed(9)
    built, parent, table = _level_case(g, 5, 65, 2, **SIX)
    built[1] = 0.0   # node 3 is built in row 1
    parent[3] = 0.0  # node 2 = parent 3 - built row 1: an empty pair
    outs = _both(hip, monkeypatch, built, parent, table, d_dims=1)
    _assert_same(outs, 6, 2)
    _, pk, ft, bn, _ = outs[0]
    for j in (2, 3):
        assert pk[j].item() == float("-inf")
        assert ft[j].item() == -1 and bn[j].item() == -1
    assert not bool(outs[0][0][2].any()) and not bool(outs[0][0][3].any())


def test_level_split_tie_rule(hip, monkeypatch):
    """Two identical feature columns: the packed atomicMax decides alike."""
    g = torch.Generator().manual_seed(10)
    built, parent, table = _level_case(g, 5, 65, 3, **SIX)
    built[:, 4] = built[:, 1]
    parent[:, 4] = parent[:, 1]
    outs = _both(hip, monkeypatch, built, parent, table, d_dims=1)
    _assert_same(outs, 6, 3)


@pytest.mark.parametrize("c", [2, 3])
def test_level_split_min_instances(hip, monkeypatch, c):
    """Some nodes refuse to split: their counts cannot fill two children."""
    g = torch.Generator().manual_seed(11)
    built, parent, table = _level_case(g, 5, 65, c, **SIX)
    built[0, ..., c - 1] = built[0, ..., c - 1].clamp(max=2.0)
    totals = built[..., c - 1].sum(dim=2)[:, 0]
    mi = float(totals.min() * 0.75)      # node 0 holds < 2 * mi rows
    outs = _both(hip, monkeypatch, built, parent, table, d_dims=1,
                 min_instances=mi)
    _assert_same(outs, 6, c)
    gains = outs[0][1][:6]
    assert bool(torch.isinf(gains).any()) and bool(torch.isfinite(gains).any())


def test_level_split_min_info_gain(hip, monkeypatch):
    g = torch.Generator().manual_seed(12)
    built, parent, table = _level_case(g, 5, 65, 3, **SIX)
    outs = _both(hip, monkeypatch, built, parent, table, d_dims=1,
                 min_info_gain=1e30)
    _assert_same(outs, 6, 3)
    assert bool(torch.isinf(outs[0][1][:6]).all())
    assert bool((outs[0][2] == -1).all())


@pytest.mark.parametrize("bad", ["built_row", "parent_row", "sibling_row",
                                 "sibling_not_built"])
def test_level_split_bad_table_raises(hip, monkeypatch, bad):
    """Checked on the host, before any launch."""
    monkeypatch.setenv("SEA_LEVEL_FUSED", "1")
    g = torch.Generator().manual_seed(13)
    built, parent, table = _level_case(g, 5, 65, 3, **SIX)
    if bad == "built_row":
        table[0, 0] = 3
    elif bad == "parent_row":
        table[1, 1] = 5
    elif bad == "sibling_row":
        table[1, 2] = 3
    else:
        table[0] = torch.tensor([-1, 0, 0])  # 0 and 1 are both derived
    with pytest.raises(RuntimeError, match="level_split"):
        hip.level_split(built.to(DEV), parent.to(DEV), table, d_dims=1)
    torch.cuda.synchronize()


def test_level_split_shape_mismatch_raises(hip, monkeypatch):
    monkeypatch.setenv("SEA_LEVEL_FUSED", "1")
    g = torch.Generator().manual_seed(14)
    built, parent, table = _level_case(g, 5, 65, 3, **SIX)
    with pytest.raises(RuntimeError, match="level_split"):
        hip.level_split(built.to(DEV), parent[:, :, :64].contiguous().to(DEV),
                        table, d_dims=1)


# --------------------------------------------------------------------------
# partition: left counts from the cursor table
# --------------------------------------------------------------------------


def test_partition_cursor_counts(hip, monkeypatch):
    """Four nodes: one longer than a partition chunk (8192 rows), one empty,
    one unsplit (feat = -1)."""
    from spark_ensemble_amd.ops import reference

    g = torch.Generator().manual_seed(20)
    n, f = 20000, 6
    bins = torch.randint(0, 32, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g).to(torch.int32)
    offs = torch.tensor([0, 9000, 9000, 12000, 20000])
    feat = torch.tensor([1, 2, -1, 0], dtype=torch.int32)
    thr = torch.tensor([15, 3, -1, 7], dtype=torch.int32)
    bins_d, rows_d = bins.to(DEV), rows.to(DEV)
    res = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("SEA_LEVEL_FUSED", flag)
        res[flag] = hip.partition_rows(bins_d, rows_d, offs, feat.to(DEV),
                                       thr.to(DEV))
    ref_rows, ref_offs, ref_lc = reference.partition_rows(bins, rows, offs,
                                                          feat, thr)
    for flag in ("1", "0"):
        new_rows, new_offs, lc = res[flag]
        assert torch.equal(lc, ref_lc.to(torch.int64))
        assert torch.equal(new_offs, ref_offs.to(torch.int64))
        nr = new_rows.cpu()
        for i in range(8):
            s, e = int(new_offs[i]), int(new_offs[i + 1])
            assert torch.equal(nr[s:e].sort().values,
                               ref_rows[s:e].sort().values)
    assert torch.equal(res["1"][2], res["0"][2])
    assert torch.equal(res["1"][1], res["0"][1])


# --------------------------------------------------------------------------
# the whole grower
# --------------------------------------------------------------------------

TREE_KEYS = ("feature", "threshold", "left_child", "leaf_value",
             "node_weight", "feature_importance")


def _forest_inputs(n, f, t, unit_hess, seed):
    g = torch.Generator().manual_seed(seed)
    b = 16
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    edges = torch.rand(f, b - 1, generator=g).sort(dim=1).values
    grads = torch.randn(n, t, generator=g)
    hess = (torch.ones(n) if unit_hess
            else torch.rand(n, generator=g) + 0.5)
    return bins.to(DEV), edges.to(DEV), grads.to(DEV), hess.to(DEV), b


def _grow(monkeypatch, flag, inputs, depth, min_inst, unit_hess, with_tp):
    from spark_ensemble_amd.models.tree_grower import GrowParams, grow_forest

    monkeypatch.setenv("SEA_LEVEL_FUSED", flag)
    bins, edges, grads, hess, b = inputs
    params = GrowParams(max_depth=depth, max_bins=b,
                        min_instances_per_node=min_inst)
    tp = [] if with_tp else None
    trees = grow_forest(bins, edges, grads, hess, params,
                        hess_is_count=unit_hess, train_pred_out=tp)
    torch.cuda.synchronize()
    return trees, (tp[0] if with_tp else None)


def _assert_forests_equal(a, b):
    (trees_a, tp_a), (trees_b, tp_b) = a, b
    assert len(trees_a) == len(trees_b)
    for ta, tb in zip(trees_a, trees_b):
        for k in TREE_KEYS:
            assert torch.equal(ta[k], tb[k]), k
    assert (tp_a is None) == (tp_b is None)
    if tp_a is not None:
        assert torch.equal(tp_a, tp_b)


@pytest.mark.parametrize("with_tp", [True, False])
@pytest.mark.parametrize("min_inst", [1, 250])
@pytest.mark.parametrize("unit_hess", [True, False])
@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("depth", [1, 3])
def test_grow_forest(hip, monkeypatch, depth, t, unit_hess, min_inst, with_tp):
    """N = 3000, F = 6, with and without captured training predictions.  With
    min_inst = 250 a last-level node of depth 3 (four of them share the 3000
    rows) needs 500 rows to split."""
    inputs = _forest_inputs(3000, 6, t, unit_hess, seed=30 + depth + t)
    runs = [_grow(monkeypatch, flag, inputs, depth, min_inst, unit_hess,
                  with_tp) for flag in ("1", "0")]
    _assert_forests_equal(*runs)
    n_nodes = sum(int(tr["feature"].numel()) for tr in runs[0][0])
    assert n_nodes > t  # something split
    if min_inst > 1 and depth == 3:
        assert n_nodes < t * 15  # and something at the bottom did not


@pytest.mark.parametrize("loss,k", [("bernoulli", 2), ("logloss", 3)])
def test_gbm_end_to_end(hip, monkeypatch, loss, k):
    """5 rounds of depth-4 trees on 20 000 x 32, fused on against off: stage
    weights, every tree array and the raw predictions are equal."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.models import DecisionTreeRegressor
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(20000, 32, k=k, seed=50, device=DEV)
    models = []
    for flag in ("1", "0"):
        monkeypatch.setenv("SEA_LEVEL_FUSED", flag)
        est = (sea.GBMClassifier()
               .setBaseLearner(DecisionTreeRegressor().setMaxDepth(4))
               .setLoss(loss).setNumBaseLearners(5).setSeed(3))
        fit_df = TensorFrame(features=df["features"], label=df["label"])
        models.append(est.fit(fit_df))
        torch.cuda.synchronize()
    on, off = models
    assert torch.equal(torch.tensor(on._weights), torch.tensor(off._weights))
    trees_on = [m._tree for ms in on._models for m in ms]
    trees_off = [m._tree for ms in off._models for m in ms]
    assert len(trees_on) == len(trees_off) == 5 * (1 if k == 2 else k)
    for ta, tb in zip(trees_on, trees_off):
        for key in ("feature", "threshold", "left_child", "leaf_value"):
            assert torch.equal(ta[key], tb[key]), key
    x = df["features"]
    assert torch.equal(on.predictRaw(x), off.predictRaw(x))
