"""Staging slots of the histogram chunk plan (csrc/hist_plan.h) through the
``_hist_plan_slots`` debug binding: for each slot, the first record and the
record count name exactly the consecutive records of its node.  No test here
touches a device."""

import os

import pytest
import torch


@pytest.fixture(scope="module")
def ext():
    assert "SEA_HIST_OVERSUB" not in os.environ, "policy values assume the default"
    return pytest.importorskip("spark_ensemble_amd._hip_ops")


def _slots(ext, offs, lds_bytes=131072, n_groups=4):
    """(chunk records, slot -> node, slot -> first record, slot -> count)."""
    offs_t = torch.tensor(offs, dtype=torch.int64)
    col0_t = torch.tensor([], dtype=torch.int32)
    args = (offs_t, col0_t, max(offs), 1, lds_bytes, n_groups)
    chunk_rows, chunks, multi = ext._hist_plan(*args)
    first, count = ext._hist_plan_slots(*args)
    assert first.dtype == torch.int32 and count.dtype == torch.int32
    assert first.numel() == multi.numel() == count.numel()
    return chunk_rows, chunks.tolist(), multi.tolist(), first.tolist(), count.tolist()


def _assert_slots_name_their_records(chunks, multi, first, count):
    for slot, (node, f0, n) in enumerate(zip(multi, first, count)):
        named = list(range(f0, f0 + n))
        of_node = [i for i, rec in enumerate(chunks) if rec[0] == node]
        assert named == of_node
        assert n >= 2
        assert all(chunks[i][3] == slot for i in named)
    # every record with a slot is named by it
    staged = [i for i, rec in enumerate(chunks) if rec[3] >= 0]
    assert staged == [i for f0, n in zip(first, count) for i in range(f0, f0 + n)]


def test_no_multi_chunk_node(ext):
    chunk_rows, chunks, multi, first, count = _slots(ext, [0, 0, 100, 4196, 4200])
    assert chunk_rows == 4096
    assert multi == [] and first == [] and count == []
    assert all(rec[3] == -1 for rec in chunks)


def test_all_nodes_multi_chunk(ext):
    chunk_rows, chunks, multi, first, count = _slots(
        ext, [0, 4097, 4097 + 8192, 4097 + 8192 + 8193])
    assert chunk_rows == 4096
    assert multi == [0, 1, 2]
    assert first == [0, 2, 4] and count == [2, 2, 3]
    _assert_slots_name_their_records(chunks, multi, first, count)


def test_empty_node_between_two_multi_chunk_nodes(ext):
    chunk_rows, chunks, multi, first, count = _slots(
        ext, [0, 9000, 9000, 9000 + 5000])
    assert chunk_rows == 4096
    assert multi == [0, 2]
    # node 0: records 0..2, the empty node's own record 3, node 2: 4..5
    assert first == [0, 4] and count == [3, 2]
    assert chunks[3][:4] == [1, 9000, 0, -1]
    _assert_slots_name_their_records(chunks, multi, first, count)


def test_large_level_chunk_rows_above_floor(ext):
    # 1M rows over 64 target chunks: chunk_rows 15625, nodes of 1 / 2 / many
    # chunks mixed
    offs = [0, 15625, 15625 + 15626, 500000, 500000, 1000000]
    chunk_rows, chunks, multi, first, count = _slots(ext, offs)
    assert chunk_rows == 15625
    assert multi == [1, 2, 4]
    _assert_slots_name_their_records(chunks, multi, first, count)
    assert sum(count) + 2 == len(chunks)
