"""Device-planned tree levels (SEA_LEVEL_CHAIN): ``level_plan_kernel``
against the host planner word for word, the histogram kernels launched from
its table on a grid sized by the planner's bound against the host-planned
launch, and whole fits with the knob on against off."""

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
def ext():
    import spark_ensemble_amd._hip_ops as m

    return m


# --------------------------------------------------------------------------
# planner equality
# --------------------------------------------------------------------------


def _pairs(lens, extra):
    """A partitioned arena given by numbers only: built child i has lens[i]
    rows and its sibling extra[i]; even children are left ones.  Returns the
    host ``child`` table, the cursor table and the arena size."""
    child, cursors, at = [], [], 0
    for i, (ln, ex) in enumerate(zip(lens, extra)):
        right = i % 2
        ps, pe = at, at + ln + ex
        le = pe - ln if right else ps + ln
        child.append([i, right, 3 * (i % 5), ps, pe])
        cursors.append([le, le])
        at = pe
    return (torch.tensor(child, dtype=torch.int32).reshape(-1, 5),
            torch.tensor(cursors, dtype=torch.int32).reshape(-1, 2), at)


def _check_plan(hip, ext, lens, extra=None, f=256, b=256, d=1, nn=1,
                gh_max=None):
    c = d + nn
    extra = [0] * len(lens) if extra is None else extra
    gh_max = torch.full((c,), 8.0) if gh_max is None else gh_max
    child, cursors, arena = _pairs(lens, extra)
    n = len(lens)
    table, seg = hip.level_plan(cursors.to(DEV), child, gh_max, arena, arena,
                                16 + c, f, b, d, c)
    tab, seg = table.cpu(), seg.cpu()

    fg, _, n_groups, lds_bytes = ext._hist_geometry(f, b, d, nn)
    b_off = torch.zeros(n + 1, dtype=torch.int64)
    b_off[1:] = torch.tensor(lens, dtype=torch.int64).cumsum(0)
    no_col0 = torch.tensor([], dtype=torch.int32)
    args = (b_off, no_col0, int(b_off[-1]), 1, lds_bytes, n_groups)
    chunk_rows, chunks, multi = ext._hist_plan(*args)
    first, count = ext._hist_plan_slots(*args)
    bound, _ = ext._hist_chunk_bound(arena, n, lds_bytes, n_groups)
    assert tab.numel() == 2 * c + 5 * bound + 4 * n

    n_chunks, n_slots = int(tab[c]), int(tab[c + 1])
    assert n_chunks == chunks.shape[0] <= bound
    assert n_slots == multi.numel()
    assert torch.equal(tab[c + 2:2 * c], torch.zeros(c - 2, dtype=torch.int32))
    # scales by bit pattern
    want_scales = ext._hist_scales(chunk_rows, gh_max)
    assert torch.equal(tab[:c], want_scales.view(torch.int32))
    recs = tab[2 * c:2 * c + 5 * n_chunks].view(-1, 5)
    assert torch.equal(recs, chunks)
    slots = tab[2 * c + 5 * n_chunks:2 * c + 5 * n_chunks + 4 * n_slots]
    slabs = count.cumsum(0) - count
    want_slots = torch.stack([multi, first, count, slabs.to(torch.int32)],
                             dim=1) if n_slots else slots.view(-1, 4)
    assert torch.equal(slots.view(-1, 4), want_slots)
    # the ranges to gather: compact offsets, source starts, col0
    assert torch.equal(seg[:n + 1], b_off)
    starts = [int(cursors[i, 0]) if child[i, 1] else int(child[i, 3])
              for i in range(n)]
    assert seg[n + 1:2 * n + 1].tolist() == starts
    assert torch.equal(seg[2 * n + 1:], child[:, 2].to(torch.int64))
    return chunk_rows, n_chunks, n_slots


@pytest.mark.parametrize("rows,want", [(0, (1, 0)), (1, (1, 0)),
                                       (4096, (1, 0)), (4097, (2, 1))])
def test_single_node_around_the_floor(hip, ext, rows, want):
    """4097 rows: just over chunk_rows, one slot of two records."""
    chunk_rows, n_chunks, n_slots = _check_plan(hip, ext, [rows], [rows])
    assert chunk_rows == 4096 and (n_chunks, n_slots) == want


@pytest.mark.parametrize("f", [64, 256])  # 1 and 4 feature groups
def test_128_mixed_nodes(hip, ext, f):
    g = torch.Generator().manual_seed(3)
    pool = torch.tensor([0, 0, 1, 37, 4096, 4097, 9000, 70000, 250000])
    lens = pool[torch.randint(0, len(pool), (128,), generator=g)].tolist()
    extra = pool[torch.randint(0, len(pool), (128,), generator=g)].tolist()
    _, n_chunks, n_slots = _check_plan(hip, ext, lens, extra, f=f)
    assert n_chunks > 128 and 0 < n_slots < 128


def test_more_nodes_than_threads_and_three_channels(hip, ext):
    """700 children: three tiles of the planner's block, the carries between
    them; C = 3 moves the header."""
    g = torch.Generator().manual_seed(4)
    lens = torch.randint(0, 12000, (700,), generator=g).tolist()
    _check_plan(hip, ext, lens, lens[::-1], f=64, d=1, nn=2)


@pytest.mark.parametrize("bad", [0.0, float("inf"), float("nan")])
def test_scale_fallback(hip, ext, bad):
    _check_plan(hip, ext, [5000, 100], gh_max=torch.tensor([bad, 2.5]))


def test_rows_past_the_chunk_cap(hip, ext):
    """Offsets only, no data behind them: 4 x 30M built rows over 64 target
    chunks want 1.9M-row chunks, which the 2^20 cap cuts."""
    chunk_rows, n_chunks, n_slots = _check_plan(
        hip, ext, [30_000_000] * 4, [20_000_000] * 4)
    assert chunk_rows == 2 ** 20 and n_slots == 4 and n_chunks > 64 + 4


# --------------------------------------------------------------------------
# bounded-grid kernels
# --------------------------------------------------------------------------


def _chain_vs_host(hip, n, f, d, nn, sizes, seed):
    """Nodes of ``sizes`` rows are pairs of siblings; the smaller-indexed
    rule does not matter here, so built children alternate left / right.
    The device-planned build of the built children must equal the
    host-planned one bit for bit."""
    c = d + nn
    g = torch.Generator().manual_seed(seed)
    b = 256
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    gh = torch.cat([torch.randn(n, d, generator=g),
                    torch.rand(n, nn, generator=g)], dim=1)
    gh = torch.cat([gh, gh * 0.5], dim=1).contiguous()  # two trees' columns
    rows = torch.randperm(n, generator=g)[:sum(sizes)].to(torch.int32)
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    child, cursors, starts, lens, col0 = [], [], [], [], []
    for k in range(len(sizes) // 2):
        ps, le, pe = offs[2 * k], offs[2 * k + 1], offs[2 * k + 2]
        right = k % 2
        child.append([k, right, c * (k % 2), ps, pe])
        cursors.append([le, le])
        starts.append(le if right else ps)
        lens.append(pe - le if right else le - ps)
        col0.append(c * (k % 2))
    child = torch.tensor(child, dtype=torch.int32)
    gh_max = gh.abs().amax(dim=0)[:c]
    bins_d, gh_d, rows_d = bins.to(DEV), gh.to(DEV), rows.to(DEV)

    got = hip.level_chain_hist(
        bins_d, gh_d, rows_d, torch.tensor(cursors, dtype=torch.int32).to(DEV),
        child, gh_max, offs[-1], b, d, c)
    again = hip.level_chain_hist(
        bins_d, gh_d, rows_d, torch.tensor(cursors, dtype=torch.int32).to(DEV),
        child, gh_max, offs[-1], b, d, c)

    starts_t, lens_t = torch.tensor(starts), torch.tensor(lens)
    rows_b, gh_b = hip.gather_ranges_gh(rows_d, gh_d, starts_t, lens_t,
                                        torch.tensor(col0), c)
    b_off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    b_off[1:] = lens_t.cumsum(0)
    want = hip.hist_build_forest(
        bins_d, gh_b, rows_b, b_off,
        torch.zeros(len(lens), dtype=torch.int32), b, c, gh_max, d_dims=d,
        gh_by_position=True)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(again, got)
    assert float(want.abs().sum()) > 0
    return lens


def test_one_cell_single_chunk_and_slab_nodes(hip):
    # C = 2, F = 64: FG = 64, one group; built children of 0, 3000, 9000 (3
    # chunks, slabs) and 20000 rows next to single-chunk ones
    lens = _chain_vs_host(
        hip, 60000, 64, 1, 1,
        [3000, 500, 700, 9000, 0, 4000, 1000, 20000, 4097, 10, 2, 4096], 61)
    assert lens == [3000, 9000, 0, 20000, 4097, 4096]


def test_two_cells_staged_atomics(hip):
    # C = 3 (hessian and count): FG = 32, two groups, staged atomics
    _chain_vs_host(hip, 40000, 64, 1, 2,
                   [100, 12000, 5000, 1, 9000, 300, 0, 4097], 62)


def test_300k_rows_above_the_floor(hip):
    # F = 256: four groups, 64 target chunks; 317k built rows put chunk_rows
    # at 4954, off its floor
    _chain_vs_host(hip, 330000, 256, 1, 1,
                   [150000, 7000, 3000, 100000, 50000, 2000, 1000, 17000], 63)


# --------------------------------------------------------------------------
# whole fits
# --------------------------------------------------------------------------

TREE_KEYS = ("feature", "threshold", "left_child", "leaf_value",
             "node_weight", "feature_importance")


def _chained_levels():
    from spark_ensemble_amd.models import tree_grower

    return tree_grower.level_chain_stats["levels"]


@pytest.mark.parametrize("loss,k", [("bernoulli", 2), ("logloss", 3)])
def test_gbm_fit_chain_on_equals_off(hip, monkeypatch, loss, k):
    """4 rounds of depth-4 trees on 20 000 x 16; logloss K = 3 grows a forest
    of T = 3 trees per round.  Tree for tree, stage weight for stage weight."""
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.frame import TensorFrame
    from spark_ensemble_amd.models import DecisionTreeRegressor
    from spark_ensemble_amd.utils.io import synthetic_classification

    df = synthetic_classification(20000, 16, k=k, seed=51, device=DEV)
    models, chained = [], []
    for flag in ("1", "0"):
        monkeypatch.setenv("SEA_LEVEL_CHAIN", flag)
        before = _chained_levels()
        est = (sea.GBMClassifier()
               .setBaseLearner(DecisionTreeRegressor().setMaxDepth(4))
               .setLoss(loss).setNumBaseLearners(4).setSeed(3))
        models.append(est.fit(TensorFrame(features=df["features"],
                                          label=df["label"])))
        torch.cuda.synchronize()
        chained.append(_chained_levels() - before)
    assert chained[0] > 0 and chained[1] == 0
    on, off = models
    assert torch.equal(torch.tensor(on._weights), torch.tensor(off._weights))
    trees_on = [m._tree for ms in on._models for m in ms]
    trees_off = [m._tree for ms in off._models for m in ms]
    assert len(trees_on) == len(trees_off) == 4 * (1 if k == 2 else k)
    for ta, tb in zip(trees_on, trees_off):
        for key in TREE_KEYS:
            assert torch.equal(ta[key], tb[key]), key
    x = df["features"]
    assert torch.equal(on.predictRaw(x), off.predictRaw(x))


def _grow(monkeypatch, flag, depth, min_inst, masks=None, t=2):
    from spark_ensemble_amd.models.tree_grower import GrowParams, grow_forest

    monkeypatch.setenv("SEA_LEVEL_CHAIN", flag)
    g = torch.Generator().manual_seed(70)
    n, f, b = 6000, 8, 16
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    edges = torch.rand(f, b - 1, generator=g).sort(dim=1).values
    grads = torch.randn(n, t, generator=g)
    hess = torch.rand(n, generator=g) + 0.5
    before = _chained_levels()
    tp = []
    trees = grow_forest(
        bins.to(DEV), edges.to(DEV), grads.to(DEV), hess.to(DEV),
        GrowParams(max_depth=depth, max_bins=b,
                   min_instances_per_node=min_inst),
        hess_is_count=False, train_pred_out=tp,
        feature_masks=None if masks is None else masks.to(DEV))
    torch.cuda.synchronize()
    return trees, tp[0], _chained_levels() - before


def _assert_same(a, b):
    for ta, tb in zip(a[0], b[0]):
        for key in TREE_KEYS:
            assert torch.equal(ta[key], tb[key]), key
    assert torch.equal(a[1], b[1])


def test_nodes_that_stop_splitting_take_the_host_level(hip, monkeypatch):
    """Depth 6 on 6000 rows with 400 rows needed per child: the first levels
    split everywhere and chain, then some nodes stop and those levels are
    planned on the host; both knob settings give the same forest."""
    on = _grow(monkeypatch, "1", 6, 400)
    off = _grow(monkeypatch, "0", 6, 400)
    _assert_same(on, off)
    n_nodes = [int(tr["feature"].numel()) for tr in on[0]]
    assert all(3 < n < 2 ** 7 - 1 for n in n_nodes)  # split, but not fully
    # levels 0..4 could chain (the last level's children are leaves)
    assert 0 < on[2] < 5 and off[2] == 0


def test_full_tree_chains_every_inner_level(hip, monkeypatch):
    on = _grow(monkeypatch, "1", 4, 1)
    off = _grow(monkeypatch, "0", 4, 1)
    _assert_same(on, off)
    assert on[2] == 3 and off[2] == 0  # after levels 0, 1 and 2


def test_feature_masks_do_not_chain(hip, monkeypatch):
    masks = torch.ones(2, 8)
    masks[0, 3] = 0
    _, _, chained = _grow(monkeypatch, "1", 4, 1, masks=masks)
    assert chained == 0
