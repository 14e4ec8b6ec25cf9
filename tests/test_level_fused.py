"""CPU side of the fused level path: without a GPU ``ops.level_split``
composes the existing ops, and that composition is the branch of
``_finish_level_split`` the grower ran before; the host-side pieces
(table checks, cursor-table left counts) run on CPU tensors as well."""

import pytest
import torch

from spark_ensemble_amd.models.tree_grower import _finish_level_split
from spark_ensemble_amd.ops import dispatch as ops

F, B, C = 5, 17, 3
ARGS = dict(lam=1e-6, min_child_weight=0.0, min_instances=1.0,
            min_info_gain=0.0, d_dims=1)


def _hist(g, n):
    h = torch.randn(n, F, B, C, generator=g)
    h[..., 1:] = torch.randint(0, 21, (n, F, B, C - 1), generator=g).float()
    return h


def _unpack(pack, n):
    return (pack[:n], pack[n:2 * n], pack[2 * n:3 * n],
            pack[3 * n:].reshape(n, C))


def test_level_split_fallback_matches_old_branch():
    """6 nodes, built {0, 3, 4}, derived {1, 2, 5} from parents {1, 3, 4} of
    a 5-row previous level: the old branch works on the compacted parents."""
    g = torch.Generator().manual_seed(1)
    built = _hist(g, 3)
    parent = _hist(g, 5)
    for row, sib in ((1, 0), (3, 1), (4, 2)):
        parent[row] = built[sib] + _hist(g, 1)[0]
    table = torch.tensor([[0, -1, -1], [-1, 1, 0], [-1, 3, 1], [1, -1, -1],
                          [2, -1, -1], [-1, 4, 2]], dtype=torch.int32)
    level, pack, feat, bin_ = ops.level_split(built, parent, table, **ARGS)

    kept = parent[torch.tensor([1, 3, 4])]  # what index_select left behind
    hists, gain, ft, b, ls = _finish_level_split(
        built.clone(), torch.tensor([0, 3, 4]), kept, torch.tensor([1, 2, 5]),
        torch.tensor([0, 3, 4]), torch.tensor([0, 1, 2]), 6, (F, B, C),
        torch.device("cpu"), None, ARGS,
    )
    assert torch.equal(level, hists)
    g_p, f_p, b_p, ls_p = _unpack(pack, 6)
    assert torch.equal(g_p, gain)
    assert torch.equal(f_p, ft.float()) and torch.equal(b_p, b.float())
    assert torch.equal(ls_p, ls)
    assert feat.dtype == torch.int32 and torch.equal(feat.long(), ft)
    assert bin_.dtype == torch.int32 and torch.equal(bin_.long(), b)


def test_level_split_fallback_root():
    g = torch.Generator().manual_seed(2)
    built = _hist(g, 2)
    table = torch.tensor([[0, -1, -1], [1, -1, -1]], dtype=torch.int32)
    level, pack, feat, bin_ = ops.level_split(built, None, table, **ARGS)
    hists, gain, ft, b, ls = _finish_level_split(
        built, None, None, None, None, None, 2, (F, B, C),
        torch.device("cpu"), None, ARGS,
    )
    assert level is built and hists is built
    g_p, f_p, b_p, ls_p = _unpack(pack, 2)
    assert torch.equal(g_p, gain) and torch.equal(ls_p, ls)
    assert torch.equal(feat.long(), ft) and torch.equal(bin_.long(), b)


@pytest.mark.parametrize("row", [
    [3, -1, -1],   # built_row out of range
    [-1, 5, 0],    # parent_row out of range
    [-1, 1, 3],    # sibling_built_row out of range
    [-1, 1, 1],    # sibling row 1 is not node 1's row
])
def test_level_split_fallback_bad_table(row):
    g = torch.Generator().manual_seed(3)
    built, parent = _hist(g, 3), _hist(g, 5)
    table = torch.tensor([row, [0, -1, -1]], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="level_split"):
        ops.level_split(built, parent, table, **ARGS)


def test_partition_finish_from_cursor_table():
    """partition_rows_finish on a pinned-style cursor table [n, 2]: left =
    lcur - segment start, same return values as with plain left counts."""
    offs = torch.tensor([0, 10, 10, 25])
    lc = torch.tensor([4, 0, 15], dtype=torch.int32)
    cursors = torch.stack([offs[:-1].to(torch.int32) + lc,
                           offs[1:].to(torch.int32)], dim=1)

    class _Done:
        def synchronize(self):
            pass

    rows = torch.arange(25, dtype=torch.int32)
    a = ops.partition_rows_finish(rows, (cursors, _Done()), offs)
    b = ops.partition_rows_finish(rows, (lc, _Done()), offs)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[1].tolist() == [0, 4, 10, 10, 10, 25, 25]
