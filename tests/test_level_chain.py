"""Device-planned tree levels (SEA_LEVEL_CHAIN), the parts that need no
device: the bound that sizes the histogram grid of a level whose node sizes
are not yet known, and the knob."""

import os
import random

import pytest
import torch


@pytest.fixture(scope="module")
def ext():
    assert "SEA_HIST_OVERSUB" not in os.environ, "policy values assume the default"
    return pytest.importorskip("spark_ensemble_amd._hip_ops")


def test_record_count_never_exceeds_the_bound(ext):
    """The grid of a device-planned level is max(target_chunks, ceil(R /
    2^20)) + n_nodes blocks, R the rows of the split parents.  However those
    rows fall to the built children (any subset of them, any sizes), the
    planner emits no more records.  Sizes are drawn around the 4096 floor,
    around one target's worth of chunks and past the 2^20 cap."""
    rng = random.Random(11)
    geoms = [(131072, 1), (131072, 4), (65536, 3), (8192, 2)]
    pools = [
        [0, 0, 1, 4095, 4096, 4097, 8193, 70000],
        [0, 1, 4097, 300000, 1 << 20, (1 << 20) + 1, 3 << 20],
        [0, 50_000_000, 90_000_000, 200_000_000],
    ]
    for trial in range(300):
        lds_bytes, n_groups = rng.choice(geoms)
        pool = pools[trial % 3]
        n_nodes = rng.randint(1, 6 if trial % 3 == 2 else 40)
        sizes = [rng.choice(pool) for _ in range(n_nodes)]
        if sum(sizes) >= 2 ** 31:
            continue
        # the parents hold the built rows and their siblings' rows
        rows_bound = sum(sizes) + rng.choice([0, 1, 4096, sum(sizes)])
        if rows_bound >= 2 ** 31:
            rows_bound = sum(sizes)
        offs = [0]
        for s in sizes:
            offs.append(offs[-1] + s)
        chunk_rows, chunks, multi = ext._hist_plan(
            torch.tensor(offs, dtype=torch.int64),
            torch.tensor([], dtype=torch.int32), max(offs), 1, lds_bytes,
            n_groups)
        bound, target = ext._hist_chunk_bound(rows_bound, n_nodes, lds_bytes,
                                              n_groups)
        assert bound == max(target, -(-rows_bound // 2 ** 20)) + n_nodes
        assert chunks.shape[0] <= bound, (sizes, rows_bound, lds_bytes, n_groups)
        assert multi.numel() <= min(n_nodes, rows_bound // 4096,
                                    bound - n_nodes)


def test_bound_is_tight_enough_to_matter(ext):
    """63 nodes one row over the 4096 floor and an empty one, 64 target
    chunks: two records each and one, 127 of a bound of 128, so the
    '+ n_nodes' term is needed."""
    n_nodes = 64
    offs = [i * 4097 for i in range(n_nodes)] + [63 * 4097]
    chunk_rows, chunks, _ = ext._hist_plan(
        torch.tensor(offs, dtype=torch.int64),
        torch.tensor([], dtype=torch.int32), offs[-1], 1, 131072, 4)
    bound, target = ext._hist_chunk_bound(offs[-1], n_nodes, 131072, 4)
    assert target == 64 and chunk_rows == 4096
    assert chunks.shape[0] == 2 * 63 + 1 == bound - 1


def test_host_scales_match_the_formula(ext):
    """2^30 / (chunk_rows * max_abs) in double, rounded once to float; a
    non-positive or non-finite maximum counts as 1."""
    ma = torch.tensor([0.0, float("inf"), float("nan"), -2.0, 1e-30, 3.5])
    got = ext._hist_scales(5000, ma)
    want = []
    for v in ma.double().tolist():
        if not (v > 0.0) or v == float("inf"):
            v = 1.0
        want.append(min(2.0 ** 30 / (5000.0 * v), 2.0 ** 30 / v))
    assert torch.equal(got, torch.tensor(want, dtype=torch.float64).float())


def test_knob_is_read_at_every_call(monkeypatch):
    from spark_ensemble_amd.ops import dispatch

    monkeypatch.delenv("SEA_LEVEL_CHAIN", raising=False)
    assert dispatch.level_chain_enabled()
    monkeypatch.setenv("SEA_LEVEL_CHAIN", "0")
    assert not dispatch.level_chain_enabled()
    monkeypatch.setenv("SEA_LEVEL_CHAIN", "1")
    assert dispatch.level_chain_enabled()


def test_cpu_fit_does_not_chain():
    """Without a GPU the grower keeps the host-planned level."""
    from spark_ensemble_amd.models import tree_grower
    from spark_ensemble_amd.models.tree_grower import GrowParams, grow_forest

    g = torch.Generator().manual_seed(5)
    bins = torch.randint(0, 16, (600, 4), generator=g, dtype=torch.uint8)
    edges = torch.rand(4, 15, generator=g).sort(dim=1).values
    before = tree_grower.level_chain_stats["levels"]
    trees = grow_forest(bins, edges, torch.randn(600, 2, generator=g),
                        torch.ones(600), GrowParams(max_depth=3, max_bins=16),
                        hess_is_count=True)
    assert int(trees[0]["feature"].numel()) > 1
    assert tree_grower.level_chain_stats["levels"] == before
