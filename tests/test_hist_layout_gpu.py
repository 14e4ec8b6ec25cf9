"""hist_build's two LDS layouts (bin-major lane-rotated for full feature
groups, feature-major for the byte-wise fallback) against an exact sum.

The fixed point is made exact: integer-valued gh in [-8, 8] (non-negative
channels in [0, 8]), ``max_abs`` passed as 8.0 per channel and few enough
rows that the planner's ``chunk_rows`` sits at its 4096 floor, so the scale
is 2^30 / (4096 * 8) = 2^15 and every addend, chunk sum (< 2^30), staging
sum and decoded float is exact.  The comparison is therefore ``torch.equal``
against a float64 CPU sum (and against ``reference.hist_build``, whose f32
sums of these integers stay far below 2^24 and are exact too)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def hip():
    from spark_ensemble_amd.ops import dispatch

    assert dispatch.hip_available(), "HIP extension must be built in-tree"
    return dispatch


def _int_gh(g, n, d, nn, lim=8):
    return torch.cat(
        [
            torch.randint(-lim, lim + 1, (n, d), generator=g),
            torch.randint(0, lim + 1, (n, nn), generator=g),
        ],
        dim=1,
    ).float()


def _sum64(bins, gh, rows, offs, b, col0=None, c=None):
    """float64 per-(node, feature, bin) sums on the CPU."""
    f = bins.shape[1]
    c = gh.shape[1] if c is None else c
    n_nodes = len(offs) - 1
    out = torch.zeros(n_nodes, f * b, c, dtype=torch.float64)
    fb = torch.arange(f) * b
    for nd in range(n_nodes):
        r = rows[offs[nd]:offs[nd + 1]].long()
        c0 = 0 if col0 is None else col0[nd]
        flat = (bins[r].long() + fb).reshape(-1)
        vals = gh[r, c0:c0 + c].double().unsqueeze(1).expand(-1, f, -1)
        out[nd].index_add_(0, flat, vals.reshape(-1, c))
    return out.view(n_nodes, f, b, c)


def _check(hip, bins, gh, rows, offs, b, d, fg, n_multi, col0=None, c=None):
    """Run the kernel twice; assert the plan (4096-row chunks, ``n_multi``
    staged nodes for the expected FG) and exact, repeatable sums."""
    import spark_ensemble_amd._hip_ops as m
    from spark_ensemble_amd.ops import reference

    f = bins.shape[1]
    c = gh.shape[1] if c is None else c
    cells = max(d, c - d)
    col0_t = torch.tensor([] if col0 is None else col0, dtype=torch.int32)
    chunk_rows, _, multi = m._hist_plan(
        torch.tensor(offs, dtype=torch.int64), col0_t, rows.numel(),
        gh.shape[1] - c + 1, fg * b * cells * 8, -(-f // fg),
    )
    assert chunk_rows == 4096
    assert multi.numel() == n_multi

    max_abs = torch.full((c,), 8.0)
    offs_t = torch.tensor(offs)
    args = (bins.to(DEV), gh.to(DEV), rows.to(DEV), offs_t)
    if col0 is None:
        run = lambda: hip.hist_build(*args, b, d, max_abs)
    else:
        run = lambda: hip.hist_build_forest(*args, col0_t, b, c, max_abs, d)
    got = run()
    again = run()
    want = _sum64(bins, gh, rows, offs, b, col0, c)
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.cpu().double(), want)
    assert torch.equal(again, got)
    if col0 is None:
        assert torch.equal(
            got.cpu(), reference.hist_build(bins, gh, rows, offs_t, b)
        )
    return got


def test_fg64_one_node_three_chunks(hip):
    # <1,1>, FG=64, 128 KiB: 9000 shuffled rows as one node, staging path
    g = torch.Generator().manual_seed(11)
    n, f, b = 9500, 64, 256
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g)[:9000].to(torch.int32)
    _check(hip, bins, _int_gh(g, n, 1, 1), rows, [0, 9000], b, 1, 64, 1)


def test_fg64_two_groups_empty_tiny_and_multichunk_nodes(hip):
    g = torch.Generator().manual_seed(12)
    n, f, b = 5100, 128, 256
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g)[:5018].to(torch.int32)
    got = _check(hip, bins, _int_gh(g, n, 1, 1), rows,
                 [0, 0, 1, 18, 5018], b, 1, 64, 1)
    assert torch.equal(got[0].cpu(), torch.zeros(f, b, 2))


def test_fg32_two_planes(hip):
    # D=1 with hess and count: CELLS=2, FG=32, two planes, two groups
    g = torch.Generator().manual_seed(13)
    n, f, b = 9000, 64, 256
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g).to(torch.int32)
    _check(hip, bins, _int_gh(g, n, 1, 2), rows,
           [0, 3000, 3000, 9000], b, 1, 32, 1)


def test_fg16_five_planes(hip):
    # D=5 with hess and count: CELLS=5, FG=16, five planes, two groups
    g = torch.Generator().manual_seed(14)
    n, f, b = 7000, 32, 256
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g).to(torch.int32)
    _check(hip, bins, _int_gh(g, n, 5, 2), rows,
           [0, 1500, 7000], b, 5, 16, 1)


def test_fg16_row_width_not_power_of_two(hip):
    # F=48, B=32: FG=16 in 4 KiB of LDS, three groups, many blocks per CU
    g = torch.Generator().manual_seed(15)
    n, f, b = 10000, 48, 32
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g)[:9537].to(torch.int32)
    _check(hip, bins, _int_gh(g, n, 1, 1), rows,
           [0, 4500, 4537, 9537], b, 1, 16, 2)


def test_fallback_keeps_feature_major(hip):
    # F=40: FG=16 does not divide the row, byte-wise path, ragged last group
    g = torch.Generator().manual_seed(16)
    n, f, b = 10000, 40, 32
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g)[:9537].to(torch.int32)
    _check(hip, bins, _int_gh(g, n, 2, 1), rows,
           [0, 4500, 4537, 9537], b, 2, 16, 2)


@pytest.mark.parametrize("pattern", ["bin0", "bin255", "alternate"])
def test_fg64_adversarial_bins(hip, pattern):
    # 4096 rows in one chunk, every lane of a wave on one address per
    # feature; 4096 * 7 * 2^15 < 2^30 keeps the field headroom
    g = torch.Generator().manual_seed(17)
    n, f, b = 4096, 64, 256
    if pattern == "bin0":
        bins = torch.zeros(n, f, dtype=torch.uint8)
    elif pattern == "bin255":
        bins = torch.full((n, f), 255, dtype=torch.uint8)
    else:
        bins = ((torch.arange(n) % 2) * 255).to(torch.uint8)
        bins = bins.unsqueeze(1).expand(n, f).contiguous()
    rows = torch.arange(n, dtype=torch.int32)
    _check(hip, bins, _int_gh(g, n, 1, 1, lim=7), rows, [0, n], b, 1, 64, 0)


def test_fg64_forest_column_groups(hip):
    # two trees' channel groups side by side in gh; node_col0 = 0 and C
    g = torch.Generator().manual_seed(18)
    n, f, b, c = 6000, 64, 256, 2
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    gh = torch.cat([_int_gh(g, n, 1, 1), _int_gh(g, n, 1, 1)], dim=1)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    # tree 0: nodes of 1000 and 5000 rows; tree 1: the same rows split 4100
    # (two chunks) / 1900
    rows = torch.cat([perm, perm])
    _check(hip, bins, gh, rows, [0, 1000, 6000, 10100, 12000], b, 1, 64, 2,
           col0=[0, 0, c, c], c=c)
