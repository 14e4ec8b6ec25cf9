"""Host-side chunk plan of the histogram kernels (csrc/hist_plan.h) through
the ``_hist_plan`` debug binding, and the staleness rule of the extension
build.  No test here touches a device."""

import os
import random
import sys

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ext():
    assert "SEA_HIST_OVERSUB" not in os.environ, "policy values assume the default"
    return pytest.importorskip("spark_ensemble_amd._hip_ops")


def _plan(ext, offs, col0=None, row_bound=None, col_bound=1, lds_bytes=8192,
          n_groups=3):
    offs_t = torch.tensor(offs, dtype=torch.int64)
    col0_t = torch.tensor([] if col0 is None else col0, dtype=torch.int32)
    if row_bound is None:
        row_bound = max(offs)
    chunk_rows, chunks, multi = ext._hist_plan(
        offs_t, col0_t, row_bound, col_bound, lds_bytes, n_groups
    )
    return chunk_rows, chunks.tolist(), multi.tolist()


def _expected_chunk_rows(total_rows, lds_bytes, n_groups):
    """The host arithmetic of plan_hist_chunks, SEA_HIST_OVERSUB unset."""
    blocks_per_cu = max(1, 163840 // max(1, lds_bytes))
    resident = 256 * blocks_per_cu
    oversub = 1.0 if blocks_per_cu == 1 else 1.5
    target = max(1, int(resident * oversub) // max(1, n_groups))
    return min(max(4096, -(-total_rows // target)), 1 << 20)


def test_random_tables_are_tiled_exactly(ext):
    rng = random.Random(7)
    for trial in range(40):
        n_nodes = rng.randint(1, 12)
        sizes = [rng.choice([0, 0, 1, 37, 4095, 4096, 4097, 9000, 50000])
                 for _ in range(n_nodes)]
        base = rng.choice([0, 5])
        offs = [base]
        for s in sizes:
            offs.append(offs[-1] + s)
        col0 = [rng.randint(0, 6) for _ in range(n_nodes)]
        lds_bytes = rng.choice([8192, 65536, 131072])
        n_groups = rng.choice([1, 3, 4])
        chunk_rows, chunks, multi = _plan(
            ext, offs, col0, col_bound=7, lds_bytes=lds_bytes,
            n_groups=n_groups,
        )
        assert chunk_rows == _expected_chunk_rows(sum(sizes), lds_bytes, n_groups)
        assert 4096 <= chunk_rows <= 2 ** 20
        want_multi = [nd for nd in range(n_nodes) if sizes[nd] > chunk_rows]
        assert multi == want_multi  # dense slots 0..n_multi-1 in node order
        # records come grouped by node, in node order
        assert [r[0] for r in chunks] == sorted(r[0] for r in chunks)
        for nd in range(n_nodes):
            recs = [r for r in chunks if r[0] == nd]
            assert recs, "every node gets at least one record"
            pos = offs[nd]
            for node, start, length, slot, c0 in recs:
                assert start == pos and 0 <= length <= chunk_rows
                assert c0 == col0[nd]
                pos += length
            assert pos == offs[nd + 1]
            if sizes[nd] == 0:
                assert len(recs) == 1 and recs[0][2] == 0 and recs[0][3] == -1
            else:
                assert all(r[2] > 0 for r in recs)
            if nd in want_multi:
                assert len(recs) > 1
                assert all(r[3] == want_multi.index(nd) for r in recs)
                assert multi[recs[0][3]] == nd
            else:
                assert len(recs) == 1 and recs[0][3] == -1


def test_null_col0_means_zero(ext):
    _, chunks, _ = _plan(ext, [0, 10, 10, 5000])
    assert [r[4] for r in chunks] == [0] * len(chunks)


@pytest.mark.parametrize(
    "lds_bytes, n_groups, offs, chunk_rows, multi",
    [
        # 20 blocks/CU -> 5120 resident x 1.5 / 3 groups = 2560 chunks;
        # 29900 rows / 2560 is under the 4096 floor
        (8192, 3, [0, 2000, 11000, 11000, 29900], 4096, [1, 3]),
        # 2 blocks/CU -> 512 x 1.5 = 768 chunks; 200000 / 768 = 261 -> floor
        (65536, 1, [0, 66666, 200000], 4096, [0, 1]),
        # 1 block/CU -> oversubscription 1.0: 256 / 4 groups = 64 chunks
        (131072, 4, [0, 10_000_000], 156250, [0]),
    ],
)
def test_policy_values(ext, lds_bytes, n_groups, offs, chunk_rows, multi):
    got_rows, chunks, got_multi = _plan(
        ext, offs, lds_bytes=lds_bytes, n_groups=n_groups
    )
    assert got_rows == chunk_rows
    assert got_rows == _expected_chunk_rows(offs[-1] - offs[0], lds_bytes, n_groups)
    assert got_multi == multi
    assert max(r[2] for r in chunks) <= chunk_rows


def test_chunk_cap(ext):
    # 1 block/CU, 1 group: 2^31 - 1 rows / 256 chunks is over the 2^20 cap
    chunk_rows, chunks, multi = _plan(
        ext, [0, 2 ** 31 - 1], lds_bytes=131072, n_groups=1
    )
    assert chunk_rows == 2 ** 20 and multi == [0]
    assert len(chunks) == 2048 and chunks[-1][2] == 2 ** 20 - 1


@pytest.mark.parametrize(
    "offs, col0, row_bound, col_bound",
    [
        ([0, 100, 50], None, 100, 1),        # decreasing pair
        ([0, 100, 201], None, 200, 1),       # end > row_bound
        ([-1, 100], None, 100, 1),           # negative start
        ([0, 100], [3], 100, 3),             # col0 == col_bound
        ([0, 100], [-1], 100, 3),            # col0 < 0
        ([0, 100], None, 100, 0),            # implicit col0 = 0 out of range
        ([0, 2 ** 31], None, 2 ** 32, 1),    # does not fit the int32 table
    ],
)
def test_rejects_bad_tables(ext, offs, col0, row_bound, col_bound):
    with pytest.raises(ValueError):
        _plan(ext, offs, col0, row_bound=row_bound, col_bound=col_bound)


def test_header_newer_than_output_forces_rebuild(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        from build_ext import is_stale
    finally:
        sys.path.pop(0)
    src = tmp_path / "ops.hip"
    hdr = tmp_path / "common.h"
    out = tmp_path / "_hip_ops.so"
    src.write_text("")
    hdr.write_text("")
    deps = [str(src), str(hdr)]
    assert is_stale(str(out), deps)  # missing output
    out.write_text("")
    os.utime(src, (1000, 1000))
    os.utime(hdr, (1000, 1000))
    os.utime(out, (2000, 2000))
    assert not is_stale(str(out), deps)
    os.utime(hdr, (3000, 3000))
    assert is_stale(str(out), deps)  # header edited after the build
    os.utime(hdr, (1000, 1000))
    os.utime(src, (3000, 3000))
    assert is_stale(str(out), deps)
