"""GPU tests (MI355X) of the forest serving path: ``bin_features`` and
every walk mode of ``forest_predict`` (raw / binned / binned_t / the v1
fallback / ``tree_predict``) against a float64 oracle walk.  Routing is
discrete and the forests of tests/serving_util.py sum exactly in f32, so
every comparison is ``torch.equal``."""

import functools

import pytest
import torch

from spark_ensemble_amd.ops import dispatch

import serving_util as su

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = ("raw", "binned", "binned_t")
N_ROWS = 5000
EXTRA = 5  # surplus x columns of the wide variants


@pytest.fixture(scope="module", autouse=True)
def hip():
    assert dispatch.hip_available(), "HIP extension must be built in-tree"
    return dispatch


@pytest.fixture(autouse=True)
def _no_mode_env(monkeypatch):
    monkeypatch.delenv("SEA_SERVE_MODE", raising=False)
    monkeypatch.delenv("SEA_SERVE_RAW", raising=False)


# ---- a. bin_features --------------------------------------------------------

BIN_SHAPES = [(1, 16, 1), (255, 16, 255), (257, 32, 63), (1000, 48, 255),
              (300, 17, 31), (300, 15, 7), (70, 5, 1)]


def _edge_rows(F, nedges, g):
    """Row f is, by f % 4: strictly increasing / all equal (a constant
    feature) / increasing with a +inf-padded tail / increasing with a NaN
    tail (the sorted sample of a column with many NaNs; quantile_bins
    itself turns such a tail into +inf)."""
    e = (torch.rand(F, nedges, generator=g) + 0.01).cumsum(1) - 0.1 * nedges
    tail = nedges // 2
    for f in range(F):
        if f % 4 == 1:
            e[f] = float(f)
        elif f % 4 == 2:
            e[f, tail:] = float("inf")
        elif f % 4 == 3:
            e[f, tail:] = float("nan")
    return e.contiguous()


def _assert_definition(got, x, edges):
    """bin == number of edges strictly below x; NaN x -> nedges.  Only
    for edge rows without a NaN."""
    ok = ~edges.isnan().any(dim=1)
    nedges = edges.shape[1]
    want = (edges.double()[None, :, :] < x.double()[:, :, None]).sum(2)
    want = torch.where(x.isnan(), torch.full_like(want, nedges), want)
    assert torch.equal(got.long()[:, ok], want[:, ok])


@pytest.mark.parametrize("n,F,nedges", BIN_SHAPES)
def test_bin_features_exact(n, F, nedges):
    g = torch.Generator().manual_seed(n * 1000 + F)
    edges = _edge_rows(F, nedges, g)
    x = su.special_x(n, F, edges, g)
    want = torch.searchsorted(edges, x.T.contiguous(), right=False).T
    got = dispatch.bin_features(x.to(DEV), edges.to(DEV))
    assert got.dtype == torch.uint8 and got.shape == (n, F)
    got = got.cpu()
    assert torch.equal(got.long(), want)
    _assert_definition(got, x, edges)


def test_bin_features_row_loop_strides():
    """F = 2048 gives 128 feature groups, which caps the grid at
    16384 / 128 = 128 row blocks of 256 rows = 32768 rows per pass, so
    the last 257 rows are reached only through the row-stride loop.  The
    reference of this one case is torch.searchsorted ON THE DEVICE (the
    same library call, 67M cells) to keep the test within seconds."""
    n, F, nedges = 32768 + 257, 2048, 15
    g = torch.Generator().manual_seed(12)
    edges = _edge_rows(F, nedges, g)
    cand = su.special_candidates(F, edges).to(DEV)
    gd = torch.Generator(device=DEV).manual_seed(13)
    idx = torch.randint(0, cand.shape[1], (F, n), generator=gd, device=DEV)
    xt = cand.gather(1, idx)  # [F, n]
    x = xt.T.contiguous()
    del idx
    edges_d = edges.to(DEV)
    got = dispatch.bin_features(x, edges_d)
    want = torch.searchsorted(edges_d, xt, right=False).T
    assert torch.equal(got.long(), want)
    # the strided tail rows, once more from the definition on the CPU
    tail = slice(32768, n)
    _assert_definition(got[tail].cpu(), x[tail].cpu(), edges)


@pytest.mark.parametrize("max_bins", [16, 256])
def test_quantile_edges_keep_bin_and_threshold_routing_equal(max_bins):
    """Device twin of the CPU test: cut points of NaN-heavy columns, the
    kernel's bins, and  bin <= t  <=>  x <= edges[t]  for every cut."""
    g = torch.Generator().manual_seed(21)
    xfit = su.nan_columns(g)
    edges = dispatch.quantile_bins(xfit.to(DEV), max_bins)
    x = torch.cat([xfit, su.special_x(500, 4, edges.cpu(), g)])
    bins = dispatch.bin_features(x.to(DEV), edges)
    su.check_bin_split_invariant(x, edges, bins)


# ---- b. every walk mode is exact -------------------------------------------

WIDE_POOL = torch.arange(-100, 100, dtype=torch.float32)  # 200 values


def _forest(name):
    """(trees, weights, F, pool) of one named forest."""
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    ip = su.INT_POOL
    if name in ("unbalanced_d1", "unbalanced_d3", "unbalanced_d8"):
        D = int(name[-1])
        F = 32 if D == 3 else 20
        trees = [su.rand_tree(6, F, D, g, ip, p_stop=0.25) for _ in range(30)]
        pool = ip
    elif name == "multigroup_binned":
        # 40 x 1023 nodes: groups of 19 / 19 / 2 trees, 19437 nodes =
        # 152 KiB of LDS (> 64 KiB: the hipFuncSetAttribute branch); at
        # most 200 distinct thresholds per feature keep the u8 ranks
        F, pool = 32, WIDE_POOL
        trees = [su.complete_tree(9, F, 1, g, pool) for _ in range(40)]
    elif name == "exact_fill":
        F, pool = 20, ip
        trees = su.exact_fill_forest(F, 1, g, pool, tail=3)
    elif name == "root_only_at_group_edges":
        # leaf | 19 x 1023 + 913 | leaf  fill group 1 exactly; group 2
        # starts and ends with a root-only tree
        F, pool, D = 20, ip, 3
        trees = ([su.leaf_tree(D, 3.0)]
                 + [su.complete_tree(9, F, D, g, pool) for _ in range(19)]
                 + [su.sized_tree(913, F, D, g, pool), su.leaf_tree(D, -7.0),
                    su.leaf_tree(D, 11.0)]
                 + [su.rand_tree(5, F, D, g, pool, p_stop=0.2)
                    for _ in range(4)]
                 + [su.leaf_tree(D, -64.0)])
    elif name == "single_tree":
        F, pool = 20, ip
        trees = [su.rand_tree(6, F, 1, g, pool, p_stop=0.2)]
    elif name.startswith("specials_seed"):
        # the forests of test_serving_pack.test_specials_pool_thresholds;
        # seeds 2 and 7 misrouted binned rows under the 3e38 edge pad
        g = torch.Generator().manual_seed(int(name[len("specials_seed"):]))
        F, pool = 7, su.SPECIALS_POOL
        trees = [su.rand_tree(3, F, 1, g, pool, p_stop=0.1) for _ in range(3)]
    else:
        raise KeyError(name)
    assert len(trees) <= 64
    return trees, su.rand_weights(len(trees), g), F, pool, g


FORESTS = ("unbalanced_d1", "unbalanced_d3", "unbalanced_d8",
           "multigroup_binned", "exact_fill", "root_only_at_group_edges",
           "single_tree", "specials_seed2", "specials_seed7")


@functools.lru_cache(maxsize=None)
def _case(name):
    """Forest, its three x variants and their oracles — built once and
    shared by every mode; nothing here is modified afterwards."""
    trees, w, F, pool, g = _forest(name)
    x = su.special_x(N_ROWS, F, pool, g)
    xw = su.special_x(N_ROWS, F + EXTRA, pool, g)
    want = {
        "plain": su.oracle(x, trees, w),
        # more columns than the forest's highest used feature
        "wide": su.oracle(xw, trees, w),
        # a column-sliced, non-contiguous view
        "view": su.oracle(xw[:, 2:2 + F], trees, w),
    }
    xd, xwd = x.to(DEV), xw.to(DEV)
    xs = {"plain": xd, "wide": xwd, "view": xwd[:, 2:2 + F]}
    assert not xs["view"].is_contiguous()
    return su.to_dev(trees, DEV), w.to(DEV), xs, want


def _serve(name, variant, mode, monkeypatch):
    trees, w, xs, _ = _case(name)
    monkeypatch.setenv("SEA_SERVE_MODE", mode)
    cache = {}
    got = dispatch.forest_predict(xs[variant], trees, w, cache=cache)
    pack = cache["pack"]
    # the mode is honoured only with the rank transform available
    assert pack["v2"] and pack.get("binned_ok")
    assert pack["bin_fmax"] <= xs[variant].shape[1]
    return got, pack


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", FORESTS)
def test_walk_mode_exact(name, mode, monkeypatch):
    want = _case(name)[3]
    for variant in ("plain", "wide", "view"):
        got, pack = _serve(name, variant, mode, monkeypatch)
        assert got.dtype == torch.float32
        bad = int((got.double().cpu() != want[variant]).any(dim=1).sum())
        assert torch.equal(got.double().cpu(), want[variant]), \
            f"{name} {mode} {variant}: {bad} of {N_ROWS} rows differ"
    if name == "multigroup_binned":
        assert pack["groups_t"].shape[0] == 3
        assert pack["max_nodes"] * 8 > 65536
    if name == "exact_fill":
        assert pack["groups_t"].tolist()[0] == [
            0, 20, 0, dispatch._FP2_GROUP_NODES]
    if name == "root_only_at_group_edges":
        assert [g[:2] for g in pack["groups_t"].tolist()] == [[0, 22], [22, 6]]


@pytest.mark.parametrize("name", FORESTS)
def test_walk_modes_bit_identical(name, monkeypatch):
    outs = [_serve(name, "plain", mode, monkeypatch)[0] for mode in MODES]
    assert not bool(outs[0].isnan().any())
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], outs[2])


# ---- c. v1 fallback and the single-tree kernel -----------------------------

def _serve_v1(trees, w, F, pool, g):
    x = su.special_x(N_ROWS, F, pool, g)
    cache = {}
    got = dispatch.forest_predict(x.to(DEV), su.to_dev(trees, DEV),
                                  w.to(DEV), cache=cache)
    assert cache["pack"]["v2"] is False
    assert torch.equal(got.double().cpu(), su.oracle(x, trees, w))


def test_v1_fallback_wide_output():
    g = torch.Generator().manual_seed(41)
    trees = [su.rand_tree(6, 20, 9, g, su.INT_POOL, p_stop=0.25)
             for _ in range(12)]
    trees.insert(5, su.leaf_tree(9, 4.0))
    _serve_v1(trees, su.rand_weights(len(trees), g), 20, su.INT_POOL, g)


def test_v1_fallback_tree_over_the_group_budget():
    g = torch.Generator().manual_seed(42)
    trees = [su.complete_tree(14, 20, 1, g, WIDE_POOL)]
    assert trees[0]["feature"].numel() == 32767 > dispatch._FP2_GROUP_NODES
    _serve_v1(trees, su.rand_weights(1, g), 20, WIDE_POOL, g)


@pytest.mark.parametrize("shape", ["unbalanced", "root_only"])
@pytest.mark.parametrize("D", [1, 3])
def test_tree_predict_exact(shape, D):
    g = torch.Generator().manual_seed(43 + D)
    F = 20
    tree = (su.rand_tree(7, F, D, g, su.INT_POOL, p_stop=0.3)
            if shape == "unbalanced" else su.leaf_tree(D, -13.0))
    x = su.special_x(N_ROWS, F, su.INT_POOL, g)
    got = dispatch.tree_predict(
        x.to(DEV), tree["feature"].to(DEV), tree["threshold"].to(DEV),
        tree["left_child"].to(DEV), tree["leaf_value"].to(DEV), 64)
    assert got.shape == (N_ROWS, D)
    assert torch.equal(got.double().cpu(), su.oracle(x, [tree]))


# ---- d. auto-selection ------------------------------------------------------

def test_auto_selected_mode_is_exact_and_stable():
    """2^20 rows with no mode forced: the three walks are timed once, the
    winner is remembered in the pack, and the answer is exact either way.
    The rows are a 2^14-row block of special values tiled 64 times, so
    the oracle walks the block once."""
    g = torch.Generator().manual_seed(44)
    F, block, reps = 16, 1 << 14, 64
    trees = [su.rand_tree(5, F, 1, g, su.INT_POOL, p_stop=0.15)
             for _ in range(8)]
    w = su.rand_weights(8, g)
    xb = su.special_x(block, F, su.INT_POOL, g)
    want = su.oracle(xb, trees, w).repeat(reps, 1)
    x = xb.to(DEV).repeat(reps, 1)
    assert x.shape[0] == 1 << 20
    cache = {}
    td, wd = su.to_dev(trees, DEV), w.to(DEV)
    first = dispatch.forest_predict(x, td, wd, cache=cache)
    assert cache["pack"].get("binned_ok")
    assert cache["pack"]["mode"] in dispatch._SERVE_MODES
    assert torch.equal(first.double().cpu(), want)
    second = dispatch.forest_predict(x, td, wd, cache=cache)
    assert torch.equal(first, second)


# ---- e. a row goes the same way in training and in serving -----------------

@pytest.mark.parametrize("kind", su.ROUTING_DATASETS)
def test_train_and_serve_route_alike(kind, monkeypatch):
    x, tree = su.fit_routing_tree(kind, DEV)
    assert x.is_cuda and tree["feature"].numel() > 7
    idt = su.id_tree(tree)
    idt_d = su.to_dev([idt], DEV)[0]
    ids = dispatch.tree_predict(x, idt_d["feature"], idt_d["threshold"],
                                idt_d["left_child"], idt_d["leaf_value"], 64)
    su.check_routing(ids[:, 0], x, tree, f"{kind} tree_predict")
    for mode in MODES:
        monkeypatch.setenv("SEA_SERVE_MODE", mode)
        cache = {}
        ids = dispatch.forest_predict(x, [idt_d], None, cache=cache)
        assert cache["pack"]["v2"] and cache["pack"].get("binned_ok")
        su.check_routing(ids[:, 0], x, tree, f"{kind} {mode}")


# ---- f. empty batch ---------------------------------------------------------

def _is_empty(t, shape, dtype):
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_cuda


def test_empty_batch_returns_empty_results():
    g = torch.Generator().manual_seed(45)
    F = 20
    x0 = torch.empty(0, F, device=DEV)
    edges = _edge_rows(F, 15, g).to(DEV)
    _is_empty(dispatch.bin_features(x0, edges), (0, F), torch.uint8)
    for D in (1, 3):
        tree = su.to_dev([su.rand_tree(4, F, D, g, su.INT_POOL)], DEV)[0]
        got = dispatch.tree_predict(
            x0, tree["feature"], tree["threshold"], tree["left_child"],
            tree["leaf_value"], 64)
        _is_empty(got, (0, D), torch.float32)
        got = dispatch.forest_predict(x0, [tree, tree], None, cache={})
        _is_empty(got, (0, D), torch.float32)
    wide = su.to_dev([su.rand_tree(3, F, 9, g, su.INT_POOL)], DEV)  # v1
    _is_empty(dispatch.forest_predict(x0, wide), (0, 9), torch.float32)
