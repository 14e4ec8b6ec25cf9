"""hist_build's flushes (slab copy + int64 reduction for multi-chunk nodes
and wide stores for single-chunk nodes in the one-cell kernel, staged
atomics in the wider kernels and the byte-wise fallback) and the
position-indexed gh of ``gather_ranges_gh``, against an exact sum.

The exactness recipe is that of test_hist_layout_gpu.py: integer-valued gh
in [-8, 8] (non-negative channels in [0, 8]), ``max_abs`` = 8 and few enough
rows that ``chunk_rows`` sits at its 4096 floor, so the scale is 2^15 and
every addend, chunk sum, slot sum and decoded float is exact.  Every case
compares with ``torch.equal`` against a float64 CPU sum and runs twice."""

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


def _plan(bins, gh, rows, offs, b, d, fg, c, col0):
    import spark_ensemble_amd._hip_ops as m

    f = bins.shape[1]
    cells = max(d, c - d)
    col0_t = torch.tensor([] if col0 is None else col0, dtype=torch.int32)
    chunk_rows, _, multi = m._hist_plan(
        torch.tensor(offs, dtype=torch.int64), col0_t, rows.numel(),
        gh.shape[1] - c + 1, fg * b * cells * 8, -(-f // fg),
    )
    assert chunk_rows == 4096
    return multi.numel()


def _run(hip, bins, gh, rows, offs, b, d, c, col0, by_position):
    """Both forms through hist_build_forest; run twice, return the first."""
    n_nodes = len(offs) - 1
    offs_t = torch.tensor(offs)
    max_abs = torch.full((c,), 8.0)
    col0_t = torch.tensor([0] * n_nodes if col0 is None else col0,
                          dtype=torch.int32)
    bins_d, gh_d, rows_d = bins.to(DEV), gh.to(DEV), rows.to(DEV)
    if by_position:
        rows_b, gh_b = hip.gather_ranges_gh(
            rows_d, gh_d, offs_t[:-1], offs_t[1:] - offs_t[:-1], col0_t, c)
        assert torch.equal(rows_b, rows_d)
        assert gh_b.shape == (rows.numel(), c)
        zero = torch.zeros(n_nodes, dtype=torch.int32)
        run = lambda: hip.hist_build_forest(  # noqa: E731
            bins_d, gh_b, rows_b, offs_t, zero, b, c, max_abs, d,
            gh_by_position=True)
    else:
        run = lambda: hip.hist_build_forest(  # noqa: E731
            bins_d, gh_d, rows_d, offs_t, col0_t, b, c, max_abs, d)
    got = run()
    again = run()
    assert torch.equal(again, got)
    return got


def _check(hip, bins, gh, rows, offs, b, d, fg, n_multi, col0=None, c=None,
           forms=(True,)):
    c = gh.shape[1] if c is None else c
    assert _plan(bins, gh, rows, offs, b, d, fg, c, col0) == n_multi
    want = _sum64(bins, gh, rows, offs, b, col0, c)
    outs = []
    for by_position in forms:
        got = _run(hip, bins, gh, rows, offs, b, d, c, col0, by_position)
        assert got.dtype == torch.float32 and got.shape == want.shape
        assert torch.equal(got.cpu().double(), want), by_position
        outs.append(got)
    for o in outs[1:]:
        assert torch.equal(o, outs[0])
    return outs[0]


def test_fg64_empty_tiny_two_and_three_chunk_nodes(hip):
    # <1,1>, FG=64, two groups: an empty node, 1 row, 17 rows, 2 chunks and
    # 3 chunks (the smallest sum over more than two slabs); both gh forms
    g = torch.Generator().manual_seed(21)
    n, f, b = 14100, 128, 256
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g)[:14018].to(torch.int32)
    got = _check(hip, bins, _int_gh(g, n, 1, 1), rows,
                 [0, 0, 1, 18, 5018, 14018], b, 1, 64, 2, forms=(True, False))
    assert torch.equal(got[0].cpu(), torch.zeros(f, b, 2))


def test_fg32_two_planes_compact_gh(hip):
    # <1,2>: CELLS=2, FG=32; two cells keep the staged atomics and the
    # 8 x 8 tile, here fed by the compact gh
    g = torch.Generator().manual_seed(22)
    n, f, b = 9000, 64, 256
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g).to(torch.int32)
    _check(hip, bins, _int_gh(g, n, 1, 2), rows,
           [0, 3000, 3000, 9000], b, 1, 32, 1)


def test_fg16_five_planes_keeps_old_tile(hip):
    # D=5 NN=2: CELLS=5, FG=16, C=7 keeps the 8 x 8 single-chunk tile
    g = torch.Generator().manual_seed(23)
    n, f, b = 7000, 32, 256
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g).to(torch.int32)
    _check(hip, bins, _int_gh(g, n, 5, 2), rows,
           [0, 1500, 7000], b, 5, 16, 1)


def test_fallback_keeps_staged_atomics(hip):
    # F=40, B=32: FG=16 does not divide the row, byte-wise path
    g = torch.Generator().manual_seed(24)
    n, f, b = 10000, 40, 32
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    rows = torch.randperm(n, generator=g)[:9537].to(torch.int32)
    _check(hip, bins, _int_gh(g, n, 2, 1), rows,
           [0, 4500, 4537, 9537], b, 2, 16, 2, forms=(True, False))


def test_forest_compact_gather_matches_row_indexed(hip):
    # two trees' channel groups in a [N, 2C] gh; the compact [M, C] gather
    # (col0 = 0 in the chunk records) must reproduce node_col0 = [0, 0, C, C]
    g = torch.Generator().manual_seed(25)
    n, f, b, c = 6000, 64, 256, 2
    bins = torch.randint(0, b, (n, f), generator=g, dtype=torch.uint8)
    gh = torch.cat([_int_gh(g, n, 1, 1), _int_gh(g, n, 1, 1)], dim=1)
    perm = torch.randperm(n, generator=g).to(torch.int32)
    rows = torch.cat([perm, perm])
    _check(hip, bins, gh, rows, [0, 1000, 6000, 10100, 12000], b, 1, 64, 2,
           col0=[0, 0, c, c], c=c, forms=(True, False))


def test_fg64_all_rows_in_last_bin(hip):
    # 4096 rows, every bin 255: one chunk, the wide-store path at the last
    # bin pair of the tile; 4096 * 7 * 2^15 < 2^30 keeps the field headroom
    g = torch.Generator().manual_seed(26)
    n, f, b = 4096, 64, 256
    bins = torch.full((n, f), 255, dtype=torch.uint8)
    rows = torch.arange(n, dtype=torch.int32)
    _check(hip, bins, _int_gh(g, n, 1, 1, lim=7), rows, [0, n], b, 1, 64, 0,
           forms=(True, False))


def test_gather_ranges_gh_alone(hip):
    # ranges of length 0 and 1, one crossing a 1024-row boundary of the
    # output (positions 601 .. 2100), distinct column groups
    g = torch.Generator().manual_seed(27)
    n, c = 5000, 2
    gh = torch.randn(n, 3 * c, generator=g)
    src = torch.randperm(n, generator=g).to(torch.int32)
    starts = torch.tensor([40, 7, 3000, 100, 900])
    lens = torch.tensor([600, 0, 1, 1500, 0])
    col0 = torch.tensor([0, c, 2 * c, c, 0])
    rows, gh_b = hip.gather_ranges_gh(src.to(DEV), gh.to(DEV), starts, lens,
                                      col0, c)
    want_rows = torch.cat([src[s:s + l] for s, l in zip(starts, lens)])
    want_gh = torch.cat([gh[src[s:s + l].long(), c0:c0 + c]
                         for s, l, c0 in zip(starts, lens, col0)])
    assert rows.dtype == torch.int32 and torch.equal(rows.cpu(), want_rows)
    assert torch.equal(gh_b.cpu(), want_gh)
    assert torch.equal(
        rows, hip.gather_ranges(src.to(DEV), starts, lens))
    # the CPU form agrees
    rows_c, gh_c = hip.gather_ranges_gh(src, gh, starts, lens, col0, c)
    assert torch.equal(rows_c, want_rows) and torch.equal(gh_c, want_gh)
