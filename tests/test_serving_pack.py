"""CPU tests of the serving path's host side: ``dispatch._pack_forest``
(packed u64 nodes, LDS group plan, u8 rank transform) walked by a
pure-torch emulation of the packed kernel and compared EXACTLY with a
float64 oracle walk, for the raw and the rank-transformed (binned) rows.
No GPU needed; tests/test_serving_gpu.py runs the same forests through
the kernels."""

import pytest
import torch

from spark_ensemble_amd.ops import dispatch

import serving_util as su

CPU = torch.device("cpu")
BUDGET = dispatch._FP2_GROUP_NODES


def _check_both_walks(x, trees, w, want_binned=True):
    pack = dispatch._pack_forest(trees, w, CPU)
    assert pack["v2"]
    su.check_groups(pack, trees)
    want = su.oracle(x, trees, w)
    got = su.emulate_packed_walk(x, pack, binned=False)
    bad = int((got != want).any(dim=1).sum())
    assert torch.equal(got, want), f"raw walk: {bad} rows differ"
    assert bool(pack.get("binned_ok")) == want_binned
    if want_binned:
        got_b = su.emulate_packed_walk(x, pack, binned=True)
        bad = int((got_b != want).any(dim=1).sum())
        assert torch.equal(got_b, want), f"binned walk: {bad} rows differ"
    return pack


@pytest.mark.parametrize("D", [1, 3])
def test_unbalanced_forest_with_root_only_trees(D):
    g = torch.Generator().manual_seed(100 + D)
    F = 7
    mk = lambda: su.rand_tree(6, F, D, g, su.INT_POOL, p_stop=0.3)  # noqa: E731
    trees = ([su.leaf_tree(D, 5.0)] + [mk() for _ in range(6)]
             + [su.leaf_tree(D, -9.0)] + [mk() for _ in range(6)]
             + [su.leaf_tree(D, 64.0)])
    sizes = {t["feature"].numel() for t in trees}
    assert len(sizes) > 3, "the trees must differ in shape"
    w = su.rand_weights(len(trees), g)
    x = su.special_x(3000, F, su.INT_POOL, g)
    _check_both_walks(x, trees, w)


@pytest.mark.parametrize("seed", range(8))
def test_specials_pool_thresholds(seed):
    """Thresholds from [-inf .. 3.4e38, +inf].  A feature with fewer
    distinct thresholds than the widest one gets a padded edge row; the
    pad must not sit below any threshold (a 3e38 pad under a 3.4e38 or
    +inf threshold left the row unsorted and misrouted binned rows)."""
    g = torch.Generator().manual_seed(seed)
    F = 7
    trees = [su.rand_tree(3, F, 1, g, su.SPECIALS_POOL, p_stop=0.1)
             for _ in range(3)]
    w = su.rand_weights(3, g)
    x = su.special_x(3000, F, su.SPECIALS_POOL, g)
    pack = dispatch._pack_forest(trees, w, CPU)
    counts = pack["bin_offs"][1:] - pack["bin_offs"][:-1]
    assert bool((counts < pack["bin_maxcnt"]).any()), \
        "no padded feature row: the case does not exercise the padding"
    edges = dispatch._binned_edges(pack, F)
    assert bool((edges[:, 1:] >= edges[:, :-1]).all()), "edge row unsorted"
    _check_both_walks(x, trees, w)


def _one_feature_forest(n_thr, g):
    """Complete depth-8 tree (255 splits) on feature 0 with 255 distinct
    thresholds, plus a stump per further threshold."""
    vals = (torch.randperm(n_thr, generator=g) - n_thr // 2).float()
    t0 = su.complete_tree(8, 1, 1, g, [0.0])
    t0["threshold"][:255] = vals[:255]
    trees = [t0]
    for v in vals[255:]:
        s = su.complete_tree(1, 1, 1, g, [float(v)])
        trees.append(s)
    return trees, vals


def test_255_distinct_thresholds_keep_the_rank_transform():
    g = torch.Generator().manual_seed(5)
    trees, vals = _one_feature_forest(255, g)
    w = su.rand_weights(len(trees), g)
    x = su.special_x(2000, 3, vals, g)  # more columns than the forest uses
    pack = _check_both_walks(x, trees, w)
    assert pack["bin_maxcnt"] == 255 and pack["bin_fmax"] == 1
    inner = trees[0]["feature"] >= 0
    ranks = (pack["node64b"] >> 32)[: inner.numel()][inner]
    assert sorted(ranks.tolist()) == list(range(255))
    # NaN rows take rank 255, the one u8 value above every threshold rank
    xb = su.lower_bound_bins(x, dispatch._binned_edges(pack, 3))
    assert bool((xb[:, 0][x[:, 0].isnan()] == 255).all())
    assert bool(x[:, 0].isnan().any())


def test_256_distinct_thresholds_turn_the_rank_transform_off():
    g = torch.Generator().manual_seed(6)
    trees, vals = _one_feature_forest(256, g)
    w = su.rand_weights(len(trees), g)
    x = su.special_x(2000, 3, vals, g)
    pack = _check_both_walks(x, trees, w, want_binned=False)
    assert "binned_ok" not in pack and "node64b" not in pack


def test_nan_threshold_keeps_the_raw_walk():
    """``x <= NaN`` is false for every x: all rows go right.  A NaN cannot
    sit in a sorted edge row, so the rank transform must stay off."""
    g = torch.Generator().manual_seed(4)
    pool = torch.cat([su.INT_POOL, torch.tensor([float("nan")])])
    trees = [su.rand_tree(4, 5, 1, g, pool, p_stop=0.1) for _ in range(6)]
    assert any(bool(t["threshold"].isnan().any()) for t in trees)
    w = su.rand_weights(6, g)
    x = su.special_x(2000, 5, su.INT_POOL, g)
    _check_both_walks(x, trees, w, want_binned=False)


def test_group_plan_exact_fill():
    g = torch.Generator().manual_seed(7)
    assert BUDGET - 19 * 1023 == 915
    trees = su.exact_fill_forest(5, 1, g, su.INT_POOL, tail=3)
    w = su.rand_weights(len(trees), g)
    x = su.special_x(600, 5, su.INT_POOL, g)
    pack = _check_both_walks(x, trees, w)
    groups = pack["groups_t"].tolist()
    assert len(groups) == 2
    assert groups[0] == [0, 20, 0, BUDGET]
    assert groups[1][:3] == [20, 3, BUDGET]
    assert pack["max_nodes"] == BUDGET


def test_group_plan_overflow_by_one_node():
    """Tree sizes are odd, so a 20-tree group ends on an even count: 20350
    nodes, and the next (3-node) tree would make 20353 = budget + 1."""
    g = torch.Generator().manual_seed(8)
    trees = [su.complete_tree(9, 5, 1, g, su.INT_POOL) for _ in range(19)]
    trees.append(su.sized_tree(913, 5, 1, g, su.INT_POOL))
    trees.append(su.complete_tree(1, 5, 1, g, su.INT_POOL))
    trees.append(su.leaf_tree(1, 3.0))
    assert sum(t["feature"].numel() for t in trees[:21]) == BUDGET + 1
    w = su.rand_weights(len(trees), g)
    x = su.special_x(600, 5, su.INT_POOL, g)
    pack = _check_both_walks(x, trees, w)
    assert pack["groups_t"].tolist() == [[0, 20, 0, BUDGET - 2],
                                         [20, 2, BUDGET - 2, 4]]


def test_oversized_tree_and_wide_output_fall_back_to_v1():
    g = torch.Generator().manual_seed(9)
    big = su.sized_tree(BUDGET + 1, 5, 1, g, su.INT_POOL)
    pack = dispatch._pack_forest([su.leaf_tree(), big], None, CPU)
    assert pack["v2"] is False and "node64" not in pack
    fits = su.sized_tree(BUDGET - 1, 5, 1, g, su.INT_POOL)
    pack = dispatch._pack_forest([su.leaf_tree(), fits], None, CPU)
    assert pack["v2"] is True
    assert su.check_groups(pack, [su.leaf_tree(), fits]) == [[0, 2, 0, BUDGET]]
    wide = [su.rand_tree(3, 5, 9, g, su.INT_POOL)]
    assert dispatch._pack_forest(wide, None, CPU)["v2"] is False
    ok = [su.rand_tree(3, 5, 8, g, su.INT_POOL)]
    assert dispatch._pack_forest(ok, None, CPU)["v2"] is True


@pytest.mark.parametrize("max_bins", [4, 16, 256])
def test_quantile_edges_keep_bin_and_threshold_routing_equal(max_bins):
    """Columns with many NaNs: the cut points stay sorted and NaN-free, so
    a split at any bin routes every value (ties, neighbours, +-inf, NaN)
    the same way by bin and by threshold."""
    g = torch.Generator().manual_seed(21)
    xfit = su.nan_columns(g)
    edges = dispatch.quantile_bins(xfit, max_bins)
    assert edges.shape == (4, max_bins - 1)
    x = torch.cat([xfit, su.special_x(500, 4, edges, g)])
    su.check_bin_split_invariant(x, edges, dispatch.bin_features(x, edges))


@pytest.mark.parametrize("kind", su.ROUTING_DATASETS)
def test_train_and_serve_route_alike_cpu(kind):
    x, tree = su.fit_routing_tree(kind)
    assert tree["feature"].numel() > 7
    if kind == "nan_inf":
        inner = tree["feature"] >= 0
        assert bool(torch.isinf(tree["threshold"][inner]).any()), \
            "the dataset is meant to produce a +inf threshold"
    idt = su.id_tree(tree)
    ids = dispatch.tree_predict(x, idt["feature"], idt["threshold"],
                                idt["left_child"], idt["leaf_value"], 64)
    su.check_routing(ids[:, 0], x, tree, f"{kind} tree_predict")
    pack = dispatch._pack_forest([idt], None, CPU)
    assert pack["v2"] and pack.get("binned_ok")
    for binned in (False, True):
        ids = su.emulate_packed_walk(x, pack, binned)[:, 0]
        su.check_routing(ids, x, tree, f"{kind} packed binned={binned}")
