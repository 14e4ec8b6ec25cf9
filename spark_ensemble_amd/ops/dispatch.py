"""Op dispatch: HIP/CDNA4 kernels on GPU, torch reference on CPU.

Policy: on a GPU box the hand-written gfx950 extension (built in-tree from
csrc/ into spark_ensemble_amd/_hip_ops.so) is REQUIRED for the designated
native ops — a missing extension raises instead of silently falling back to
eager torch, so a passing GPU test run always means the HIP path ran.  Set
SEA_ALLOW_EAGER=1 to override for debugging only.
"""

from __future__ import annotations

import math
import os
from typing import Optional

import torch

from . import reference

_hip = None
_hip_error: Optional[str] = None


def _load_hip():
    global _hip, _hip_error
    if _hip is not None or _hip_error is not None:
        return _hip
    try:
        from . import hip_ext

        _hip = hip_ext.load()
    except Exception as e:  # noqa: BLE001
        _hip_error = f"{type(e).__name__}: {e}"
        _hip = None
    return _hip


def hip_available() -> bool:
    return _load_hip() is not None


def _require_hip(op_name: str):
    m = _load_hip()
    if m is None:
        if os.environ.get("SEA_ALLOW_EAGER") == "1":
            return None
        raise RuntimeError(
            f"HIP extension required for {op_name} on GPU but not available "
            f"({_hip_error}). Build it with `python setup.py build_ext --inplace` "
            f"or set SEA_ALLOW_EAGER=1 to run the slow eager fallback."
        )
    return m


# ---------------------------------------------------------------------------


def sample_weights(replacement, ratio, n, seed, device=None, base_weight=None, rank=0):
    dev = torch.device(device) if device is not None else torch.device("cpu")
    if dev.type == "cuda":
        m = _require_hip("sample_weights")
        if m is not None:
            w = torch.empty(n, dtype=torch.float32, device=dev)
            m.sample_weights(w, bool(replacement), float(ratio), int(seed), int(rank))
            if base_weight is not None:
                w *= base_weight
            return w
    return reference.sample_weights(replacement, ratio, n, seed, device, base_weight, rank)


def quantile_bins(x, max_bins=256, sample_rows=262_144, seed=17):
    # sort-based; torch sort is fine on both devices (one-time cost per fit)
    return reference.quantile_bins(x, max_bins, sample_rows, seed)


def bin_features(x, edges):
    if x.is_cuda:
        m = _require_hip("bin_features")
        if m is not None:
            out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
            if x.shape[0] == 0:
                return out  # a 0-block grid is not a valid launch
            m.bin_features(out, x.contiguous(), edges.contiguous())
            return out
    return reference.bin_features(x, edges)


def hist_build(bins, gh, row_idx, node_offsets, num_bins, d_dims=-1, max_abs=None, identity_rows=False):
    """Per-(node, feature, bin) channel sums.

    Channel contract (tree_grower.py): gh[:, :d_dims] are SIGNED gradient
    channels, gh[:, d_dims:] are NON-NEGATIVE hess/count channels — the
    gfx950 kernel accumulates in packed fixed-point u64 LDS cells
    (ds_add_u64 is ~13x faster than ds_add_f32 on gfx950, see
    profiles/r01_hist_probe.md).  ``max_abs`` (host [C] tensor of per-channel
    abs maxima) sizes the quantization; pass it from the caller to avoid a
    device sync per level — when None it is computed here (one sync).
    """
    if bins.is_cuda:
        m = _require_hip("hist_build")
        if m is not None:
            n_nodes = node_offsets.numel() - 1
            C = gh.shape[1]
            if max_abs is None:
                max_abs = gh.abs().amax(dim=0).cpu()
            if C > 8:
                # wide one-hot targets (K-class gini trees, K > 7): the
                # kernel caps at 8 channels, so re-layout gh ONCE into
                # contiguous per-chunk groups [g_s..g_{s+w-1}, tail...]
                # (tail = hess/count duplicated per chunk, <= 2 cols) and
                # launch one kernel per chunk with a column offset — no
                # per-chunk gh copies (r01 chunking index_select'ed the
                # whole gh every chunk).  Chunk width is 8 - len(tail) so
                # every launch is within the channel cap.
                D = d_dims if d_dims > 0 else C - 1
                tail = list(range(D, C))
                step = 8 - len(tail)
                assert 1 <= step <= 7, f"hist_build tail too wide: {len(tail)}"
                spans = []  # (col0_in_wide, w)
                cols: list = []
                for s in range(0, D, step):
                    w = min(step, D - s)
                    spans.append((len(cols), w))
                    cols.extend(range(s, s + w))
                    cols.extend(tail)
                idx = torch.tensor(cols, device=gh.device)
                gh_wide = gh.index_select(1, idx).contiguous()  # once
                ma_wide = max_abs[torch.tensor(cols)]
                parts = []
                for ci, (c0, w) in enumerate(spans):
                    cc = w + len(tail)
                    part = hist_build_forest(
                        bins, gh_wide, row_idx, node_offsets,
                        torch.full((n_nodes,), c0, dtype=torch.int32),
                        num_bins, cc, ma_wide[c0:c0 + cc], d_dims=w,
                    )
                    parts.append(part[..., :w])
                    if ci == len(spans) - 1:
                        parts.append(part[..., w:])  # tail once
                return torch.cat(parts, dim=-1)
            return _hist_build_launch(
                m, bins, gh, row_idx, node_offsets, _EMPTY_I32, num_bins, C,
                max_abs, d_dims, identity_rows,
            )
    return reference.hist_build(bins, gh, row_idx, node_offsets, num_bins)


_EMPTY_I32 = torch.empty(0, dtype=torch.int32)
_EMPTY_U8 = torch.empty(0, dtype=torch.uint8)


def _hist_build_launch(m, bins, gh, row_idx, node_offsets, node_col0,
                       num_bins, c_per_node, max_abs, d_dims, identity_rows,
                       gh_by_position=False):
    """Allocate ``out`` and run the native hist_build.  Every node's slice
    is fully written by the kernel's flush or the staging reduction
    (zero-row nodes included), so ``out`` needs no zero fill."""
    out = torch.empty(
        node_offsets.numel() - 1, bins.shape[1], num_bins, c_per_node,
        dtype=torch.float32, device=bins.device,
    )
    m.hist_build(
        out, bins, gh.contiguous(), row_idx.to(torch.int32),
        node_offsets.to(torch.int64).cpu().contiguous(), int(num_bins),
        int(d_dims), max_abs.to(torch.float32), bool(identity_rows),
        node_col0, int(c_per_node), bool(gh_by_position),
    )
    return out


def hist_build_forest(bins, gh, row_idx, node_offsets, node_col0, num_bins,
                      c_per_node, max_abs, d_dims=1, gh_by_position=False,
                      identity_rows=False):
    """Forest histogram build: gh is [N, CH] with contiguous per-node
    channel groups; node_col0[n] selects the base column node n
    accumulates (tree fusion: owning_tree * C; wide-gini chunking: the
    chunk's column offset).  One launch covers every active node of every
    tree in the level (the MI355X form of the reference's parallel
    per-class futures, GBMClassifier.scala:377-411).  ``max_abs`` is
    slot-wise ([c_per_node]): max over the corresponding column of every
    group.  ``gh_by_position``: gh is the compact ``[len(row_idx), CH]``
    matrix of ``gather_ranges_gh`` and entry i of row_idx reads gh row i.
    ``identity_rows``: row_idx is ``arange(N)`` (the root of a lone tree over
    every row) and the GPU kernel does not read it."""
    if bins.is_cuda:
        m = _require_hip("hist_build")
        if m is not None:
            return _hist_build_launch(
                m, bins, gh, row_idx, node_offsets,
                node_col0.to(torch.int32).cpu().contiguous(), num_bins,
                c_per_node, max_abs, d_dims, bool(identity_rows),
                gh_by_position,
            )
    if gh_by_position:
        # the reference indexes gh by row: bins gathered, rows = positions
        pos = torch.arange(row_idx.numel(), device=row_idx.device)
        return reference.hist_build_forest(
            bins.index_select(0, row_idx.long()), gh, pos, node_offsets,
            node_col0, num_bins, c_per_node
        )
    return reference.hist_build_forest(
        bins, gh, row_idx, node_offsets, node_col0, num_bins, c_per_node
    )


# what the last GPU hist_build_class launch did (tests assert the
# multi-chunk staging path was taken without guessing the chunk policy)
last_hist_build_class_info: dict = {}


def hist_build_class(bins, label, weight, row_idx, node_offsets, node_col0,
                     num_bins, num_classes, nn, w_max=None,
                     identity_rows=False, transposed=None):
    """Label-indexed histograms for K-class gini trees (2 <= K <= 32).

    ``label`` [N] u8, ``weight`` [N, T] f32 >= 0 (one column per fused
    tree), host ``node_offsets`` / ``node_col0`` (per-node weight column).
    Output [n_nodes, F, B, K + nn] in the grower's layout (classes, hess,
    count when nn == 2).  The gfx950 kernel spends ONE ds_add_u64 per
    (row, feature) and quantises with a power-of-two scale sized by the
    host scalar ``w_max`` (computed here, with one sync, when None), so
    integer-valued weights histogram exactly.  ``transposed`` picks the
    bins source: the cached [F, N] transpose (default, see
    profiles/wide_class.md) or the row-major matrix.
    """
    if bins.is_cuda:
        m = _require_hip("hist_build_class")
        if m is not None:
            n_nodes = node_offsets.numel() - 1
            F = bins.shape[1]
            C = int(num_classes) + int(nn)
            if w_max is None:
                w_max = float(weight.max()) if weight.numel() else 1.0
            if transposed is None:
                transposed = os.environ.get("SEA_CLASS_HIST_SRC") != "rowmajor"
            bt = _bins_transposed(bins) if transposed else _EMPTY_U8
            # every node's slice is fully written by the flush or the
            # decode pass (zero-row nodes included) — no zero fill
            out = torch.empty(n_nodes, F, num_bins, C, dtype=torch.float32,
                              device=bins.device)
            n_multi = m.hist_build_class(
                out, bins, bt, label, weight.contiguous(),
                row_idx.to(torch.int32),
                node_offsets.to(torch.int64).cpu().contiguous(),
                node_col0.to(torch.int32).cpu().contiguous(),
                int(num_bins), int(num_classes), int(nn), float(w_max),
                bool(identity_rows),
            )
            last_hist_build_class_info["multi_chunk_nodes"] = int(n_multi)
            return out
    return reference.hist_build_class(
        bins, label, weight, row_idx, node_offsets, node_col0, num_bins,
        num_classes, nn,
    )


SPLIT_WIDE_MAX_C = 34  # K <= 32 one-hot channels + hess + count


def split_search(hist, lam=1e-6, min_child_weight=0.0, min_instances=1.0, min_info_gain=0.0, d_dims=-1):
    if hist.is_cuda:
        c_chk = hist.shape[3]
        if c_chk > SPLIT_WIDE_MAX_C:
            # beyond the wide kernel's channel cap (K > 32 gini trees):
            # eager torch path (runs on GPU)
            return reference.split_search(
                hist, lam, min_child_weight, min_instances, min_info_gain,
                d_dims,
            )
        m = _require_hip("split_argmax")
        if m is not None:
            n, f, b, c = hist.shape
            gain = torch.empty(n, dtype=torch.float32, device=hist.device)
            feat = torch.empty(n, dtype=torch.int32, device=hist.device)
            bin_ = torch.empty(n, dtype=torch.int32, device=hist.device)
            left_stats = torch.empty(n, c, dtype=torch.float32, device=hist.device)
            m.split_argmax(
                gain, feat, bin_, left_stats, hist.contiguous(),
                int(d_dims), float(lam), float(min_child_weight),
                float(min_instances), float(min_info_gain),
            )
            return gain, feat.long(), bin_.long(), left_stats
    return reference.split_search(hist, lam, min_child_weight, min_instances, min_info_gain, d_dims)


def level_fused_enabled() -> bool:
    """``SEA_LEVEL_FUSED=0`` keeps the tree level loop on the composed ops
    (assemble + split_search + pack, device-side left counts); read at every
    call."""
    return os.environ.get("SEA_LEVEL_FUSED", "1") != "0"


def _check_level_table(table, n_built, n_prev):
    """The checks of the native level_split, for the composed path."""
    tb = table.tolist()
    n = len(tb)
    for j, (br, pr, sr) in enumerate(tb):
        if br >= 0:
            if br >= n_built:
                raise RuntimeError(f"level_split: built_row {br} of node {j} "
                                   "out of range")
            continue
        if br != -1:
            raise RuntimeError(f"level_split: built_row of node {j} is {br}")
        if not 0 <= pr < n_prev:
            raise RuntimeError(f"level_split: parent_row {pr} of node {j} "
                               "out of range")
        if not 0 <= sr < n_built:
            raise RuntimeError(f"level_split: sibling_built_row {sr} of node "
                               f"{j} out of range")
        if (j ^ 1) >= n or tb[j ^ 1][0] != sr:
            raise RuntimeError(f"level_split: the sibling of derived node {j} "
                               f"is not the built node in row {sr}")


def level_split(built, parent, table, lam=1e-6, min_child_weight=0.0,
                min_instances=1.0, min_info_gain=0.0, d_dims=-1):
    """Split search of one tree level straight off its sources.

    ``built`` [n_built, F, B, C] holds the histograms built at this level,
    ``parent`` [n_prev, F, B, C] the previous level's full tensor (None or
    empty at the root), ``table`` a host int32 [n, 3] of (built_row,
    parent_row, sibling_built_row) per active node: node j scans
    ``built[built_row]`` when built_row >= 0, else ``parent[parent_row] -
    built[sibling_built_row]``; its sibling is node j ^ 1.

    Returns (level, pack, feat, bin): ``level`` [n, F, B, C] is the full level
    tensor (``built`` itself at a root whose table is the identity), ``pack``
    the f32 [n * (3 + C)] buffer (gain[n], feat[n], bin[n], left_stats[n, C])
    meant for one copy to the host, feat / bin int32 device tensors for
    ``partition_rows_async``.

    GPU: one scan kernel + one decode kernel (C <= 8).  Without a GPU, or with
    ``SEA_LEVEL_FUSED=0``, the same result is composed from index copies, a
    subtraction, ``split_search`` and a cat.
    """
    table = table.to(torch.int32).cpu().contiguous()
    n = table.shape[0]
    n_built, F, B, C = built.shape
    root = parent is None or parent.numel() == 0
    n_prev = 0 if root else parent.shape[0]
    if not root and tuple(parent.shape[1:]) != (F, B, C):
        raise RuntimeError("level_split: parent and built disagree in F, B, C")
    identity = n == n_built and bool(
        (table[:, 0] == torch.arange(n, dtype=torch.int32)).all())
    args = (float(lam), float(min_child_weight), float(min_instances),
            float(min_info_gain))
    if built.is_cuda and C <= 8 and level_fused_enabled():
        m = _require_hip("level_split")
        if m is not None:
            dev = built.device
            built = built.contiguous()
            level = built if root and identity else torch.empty(
                n, F, B, C, dtype=torch.float32, device=dev)
            pack = torch.empty(n * (3 + C), dtype=torch.float32, device=dev)
            feat = torch.empty(n, dtype=torch.int32, device=dev)
            bin_ = torch.empty(n, dtype=torch.int32, device=dev)
            m.level_split(
                level, pack, feat, bin_, built,
                built.new_empty(0) if root else parent.contiguous(), table,
                int(d_dims), *args,
            )
            return level, pack, feat, bin_
    _check_level_table(table, n_built, n_prev)
    dev = built.device
    if root and identity:
        level = built
    else:
        tb = table.long()
        b_nodes = (tb[:, 0] >= 0).nonzero(as_tuple=True)[0]
        d_nodes = (tb[:, 0] < 0).nonzero(as_tuple=True)[0]
        level = torch.empty(n, F, B, C, dtype=torch.float32, device=dev)
        if b_nodes.numel():
            level[b_nodes.to(dev)] = built[tb[b_nodes, 0].to(dev)]
        if d_nodes.numel():
            level[d_nodes.to(dev)] = (
                parent[tb[d_nodes, 1].to(dev)] - built[tb[d_nodes, 2].to(dev)]
            )
    g, ft, b, ls = split_search(level, *args, d_dims=d_dims)
    pack = torch.cat([g, ft.to(torch.float32), b.to(torch.float32),
                      ls.reshape(-1)])
    return level, pack, ft.to(torch.int32), b.to(torch.int32)


def partition_rows(bins, row_idx, node_offsets, feat, thr):
    if bins.is_cuda:
        m = _require_hip("partition_rows")
        if m is not None:
            new_rows, lc_dev, offs_cpu = partition_rows_async(
                bins, row_idx, node_offsets, feat, thr
            )
            return partition_rows_finish(new_rows, lc_dev, offs_cpu)
    return reference.partition_rows(bins, row_idx, node_offsets, feat, thr)


_BT_CACHE: list = []  # [(weakref(bins), bins_t)] — at most 2 entries


def _bins_transposed(bins):
    """[F, N] transpose of the binned matrix, cached by OBJECT identity
    (the grower reuses one bins tensor across all rounds of a fit).  The
    partition kernel reads it instead of the row-major matrix: a node's
    rows are locally dense, so a 64-B line yields many useful bytes
    instead of one.  One transpose_u8 pass (~0.7 ms at 10M x 256)
    amortizes over every level of every round."""
    import weakref

    m = _load_hip()
    if m is None or not bins.is_cuda:
        return None
    # prune entries whose bins tensor died FIRST: a stale entry pins a
    # multi-GB transpose (25.6 GB at the 100M x 256 capacity point)
    _BT_CACHE[:] = [(w, b) for (w, b) in _BT_CACHE if w() is not None]
    for wr, bt in _BT_CACHE:
        if wr() is bins:
            return bt
    n, f = bins.shape
    bt = torch.empty(f, n, dtype=torch.uint8, device=bins.device)
    m.transpose_u8(bt, bins)
    _BT_CACHE.insert(0, (weakref.ref(bins), bt))
    del _BT_CACHE[1:]
    return bt


def partition_rows_async(bins, row_idx, node_offsets, feat, thr):
    """Launch the partition kernel WITHOUT syncing (feat/thr may be live
    device tensors straight from split_argmax); call
    :func:`partition_rows_finish` after the caller's own device sync."""
    import time as _time

    _prof = os.environ.get("SEA_GROW_PROF") == "1"
    _t0 = _time.perf_counter() if _prof else 0.0
    m = _require_hip("partition_rows")
    n = node_offsets.numel() - 1
    offs_cpu = node_offsets.to(torch.int64).cpu()
    row_idx = row_idx.to(torch.int32)
    new_rows = torch.empty_like(row_idx)
    f32 = feat.to(torch.int32).to(bins.device)
    t32 = thr.to(torch.int32).to(bins.device)
    bt = _bins_transposed(bins)
    if level_fused_enabled():
        # the cursor table itself goes to the host (left = lcur - segment
        # start, subtracted in partition_rows_finish): no zero fill, no
        # segment-start upload, no device subtract; int32 feat / thr straight
        # from level_split pass the two casts above untouched
        cursors = m.partition_rows_cursors(
            new_rows, bins, bt if bt is not None else _EMPTY_U8,
            row_idx.contiguous(), offs_cpu, f32.contiguous(),
            t32.contiguous(),
        )
        cur_h = torch.empty(n, 2, dtype=torch.int32, pin_memory=True)
        cur_h.copy_(cursors, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return new_rows, (cur_h, ev), offs_cpu
    left_counts = torch.zeros(n, dtype=torch.int32, device=bins.device)
    if _prof:
        _t1 = _time.perf_counter()
    m.partition_rows(
        new_rows,
        left_counts,
        bins,
        bt if bt is not None else _EMPTY_U8,
        row_idx,
        offs_cpu,
        f32,
        t32,
    )
    # prefetch the left counts: non-blocking D2H + event, so finish()
    # wakes the host the moment the kernel ends (a blocking .cpu() there
    # costs an extra stream round trip after the partition)
    lc_h = torch.empty(left_counts.numel(), dtype=torch.int32,
                       pin_memory=True)
    lc_h.copy_(left_counts, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    if _prof:
        _t2 = _time.perf_counter()
        print(f"[part prof] prep={(_t1-_t0)*1000:.2f} native={(_t2-_t1)*1000:.2f}")
    return new_rows, (lc_h, ev), offs_cpu


def gather_ranges(src, starts, lens):
    """Concatenation of ``src[starts_i : starts_i + lens_i)`` ranges.

    src is an int32 device row arena; starts/lens are SMALL cpu int64
    tensors (one entry per active node).  GPU: one kernel pass (binary
    search over the L2-resident prefix table) instead of torch's
    repeat_interleave + cumsum + arange + gather chain.  CPU: slice cat.
    """
    if src.is_cuda:
        m = _require_hip("gather_ranges")
        if m is not None:
            out = torch.empty(int(lens.sum()), dtype=torch.int32,
                              device=src.device)
            m.gather_ranges(out, src, starts.to(torch.int64),
                            lens.to(torch.int64))
            return out
    st, ln = starts.tolist(), lens.tolist()
    segs = [src[s:s + l] for s, l in zip(st, ln) if l > 0]
    if not segs:
        return torch.empty(0, dtype=src.dtype, device=src.device)
    return segs[0].clone() if len(segs) == 1 else torch.cat(segs)


def gather_ranges_gh(src, gh, starts, lens, col0, c_per_node):
    """``gather_ranges`` that brings the gradients along: returns the
    gathered rows and the compact ``[M, c_per_node]`` matrix whose row i is
    ``gh[rows[i], col0_j : col0_j + c_per_node]`` for the range j that
    position i belongs to.  One gather per built row, in the pass that
    already writes the rows; ``hist_build_forest(..., gh_by_position=True)``
    then streams it.  starts/lens/col0 are small cpu tensors."""
    C = int(c_per_node)
    if src.is_cuda:
        m = _require_hip("gather_ranges_gh")
        if m is not None:
            total = int(lens.sum())
            out = torch.empty(total, dtype=torch.int32, device=src.device)
            gh_out = torch.empty(total, C, dtype=torch.float32,
                                 device=src.device)
            m.gather_ranges_gh(out, gh_out, src, gh.contiguous(),
                               starts.to(torch.int64), lens.to(torch.int64),
                               col0.to(torch.int64))
            return out, gh_out
    rows = gather_ranges(src, starts, lens)
    segs = [
        gh[src[s:s + l].long(), c0:c0 + C]
        for s, l, c0 in zip(starts.tolist(), lens.tolist(), col0.tolist())
        if l > 0
    ]
    if not segs:
        return rows, gh.new_empty(0, C)
    return rows, torch.cat(segs)


def leaf_scatter(tp, row_idx, starts, lens, tree, val):
    """tp[row_idx[starts_i : starts_i+lens_i], tree_i] = val_i for every
    segment i — the train-pred leaf capture, fused into one kernel on GPU
    (no device-side index lists are materialized at all)."""
    if tp.is_cuda:
        m = _require_hip("leaf_scatter")
        if m is not None:
            m.leaf_scatter(tp, row_idx, starts.to(torch.int64),
                           lens.to(torch.int64), tree.to(torch.int64),
                           val.to(torch.float32))
            return
    st, ln = starts.tolist(), lens.tolist()
    tl, vl = tree.tolist(), val.tolist()
    for s, l, t, v in zip(st, ln, tl, vl):
        if l > 0:
            tp[row_idx[s:s + l].long(), int(t)] = float(v)


def partition_rows_finish(new_rows, left_counts, offs_cpu):
    n = offs_cpu.numel() - 1
    if isinstance(left_counts, tuple):
        lc_h, ev = left_counts
        ev.synchronize()
        if lc_h.dim() == 2:  # the cursor table: left = lcur - segment start
            lc = lc_h[:, 0].to(torch.int64) - offs_cpu[:-1]
        else:
            lc = lc_h.to(torch.int64)
    else:
        lc = left_counts.cpu().to(torch.int64)
    sizes = torch.empty(2 * n, dtype=torch.int64)
    seg = offs_cpu[1:] - offs_cpu[:-1]
    sizes[0::2] = lc
    sizes[1::2] = seg - lc
    new_offs = torch.cat([torch.zeros(1, dtype=torch.int64), sizes.cumsum(0)])
    return new_rows, new_offs, lc


def tree_predict(x, feature, threshold, left_child, leaf_value, max_depth):
    if x.is_cuda:
        m = _require_hip("tree_predict")
        if m is not None:
            N = x.shape[0]
            D = leaf_value.shape[1]
            out = torch.empty(N, D, dtype=torch.float32, device=x.device)
            if N == 0:
                return out
            m.tree_predict(
                out,
                x.contiguous(),
                feature.to(torch.int32).to(x.device),
                threshold.to(torch.float32).to(x.device),
                left_child.to(torch.int32).to(x.device),
                leaf_value.to(torch.float32).to(x.device).contiguous(),
            )
            return out
    return reference.tree_predict(x, feature, threshold, left_child, leaf_value, max_depth)


def forest_predict(x, trees, weights=None, max_depth=64, cache=None):
    """Packed-forest ensemble inference.

    ``cache``: an optional caller-owned dict; the packed node arena is
    stored there under key "pack" so repeated transform calls on the same
    (immutable, post-fit) tree list skip the per-call packing.
    """
    if x.is_cuda and trees:
        m = _require_hip("forest_predict")
        if m is not None:
            if x.shape[0] == 0:
                return torch.zeros(0, trees[0]["leaf_value"].shape[1],
                                   dtype=torch.float32, device=x.device)
            pack = cache.get("pack") if cache is not None else None
            if pack is None or pack["T"] != len(trees) or pack["dev"] != x.device:
                pack = _pack_forest(trees, weights, x.device)
                if cache is not None:
                    cache["pack"] = pack
            return _forest_predict_packed(m, x, pack)
    return reference.forest_predict(x, trees, weights, max_depth)


_FP2_GROUP_NODES = 20352  # ~159 KiB of packed 8-B nodes per LDS group (160 KiB LDS/CU)


def _pack_forest(trees, weights, dev):
    """Pack a tree list into the arena tensors both kernel paths consume.
    Done once per (model, device) — callers cache the result."""
    # per-tree moves BEFORE the cat: a resumed ensemble mixes CPU-loaded
    # checkpoint stages with device-fitted ones
    feats = torch.cat([t["feature"].to(dev, torch.int32) for t in trees])
    thrs = torch.cat([t["threshold"].to(dev, torch.float32) for t in trees])
    lefts = torch.cat([t["left_child"].to(dev, torch.int32) for t in trees])
    leaves = torch.cat(
        [t["leaf_value"].to(dev, torch.float32) for t in trees]
    ).contiguous()
    sizes = [t["feature"].numel() for t in trees]
    sizes_t = torch.tensor(sizes, dtype=torch.int64)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), sizes_t.cumsum(0)])[:-1]
    offsets32 = offsets.to(torch.int32).to(dev)
    D = trees[0]["leaf_value"].shape[1]
    T = len(trees)
    if weights is None:
        w = torch.ones(T, dtype=torch.float32, device=dev)
    else:
        w = weights.to(torch.float32).to(dev)

    pack = {
        "T": T, "D": D, "dev": dev, "feats": feats, "thrs": thrs,
        "lefts": lefts, "leaves": leaves, "offsets32": offsets32, "w": w,
        "v2": False,
    }
    fits_v2 = D <= 8 and max(sizes) <= _FP2_GROUP_NODES
    if not fits_v2:
        return pack

    # ---- v2: pack (feat s16 | left s16 | payload f32-bits) into one u64
    # per node; for D == 1 a leaf's payload IS its weighted leaf value so
    # the kernel never touches the leaf tensor (csrc forest_predict2)
    if D == 1:
        tree_id = torch.repeat_interleave(
            torch.arange(T, device=dev), sizes_t.to(dev)
        )
        payload = torch.where(feats < 0, w[tree_id] * leaves[:, 0], thrs)
    else:
        payload = thrs
    node64 = (
        (feats.to(torch.int64) & 0xFFFF)
        | ((lefts.to(torch.int64) & 0xFFFF) << 16)
        | ((payload.view(torch.int32).to(torch.int64) & 0xFFFFFFFF) << 32)
    ).contiguous()

    # greedy contiguous tree groups under the LDS node budget
    groups = []
    off_list = offsets.tolist()
    first = 0
    acc = 0
    max_nodes = 0
    for t in range(T):
        if acc + sizes[t] > _FP2_GROUP_NODES and acc > 0:
            groups.append([first, t - first, off_list[first], acc])
            max_nodes = max(max_nodes, acc)
            first, acc = t, 0
        acc += sizes[t]
    groups.append([first, T - first, off_list[first], acc])
    max_nodes = max(max_nodes, acc)
    pack.update(
        v2=True,
        node64=node64,
        groups_t=torch.tensor(groups, dtype=torch.int32, device=dev),
        max_nodes=max_nodes,
    )
    _pack_forest_binned(pack, feats, thrs, payload)
    return pack


def _pack_forest_binned(pack, feats, thrs, payload):
    """Rank-transform serving structures (EXACT): collect each feature's
    sorted unique threshold set; a node's threshold becomes its RANK in
    that set, and at predict time every row is rank-transformed once via
    the bin_features kernel (lower_bound against the +inf-padded set),
    after which  x <= thr  <=>  rank(x) <= rank(thr)  on u8 bins for every
    f32 x, +-inf included; a NaN x ranks above every threshold and goes
    right — rows shrink 4x for the divergent walk gathers.  Disabled when
    any feature carries > 255 distinct thresholds (u8 overflow)."""
    dev = pack["dev"]
    mask = feats >= 0
    m_cnt = int(mask.sum())
    if m_cnt == 0:
        return
    f_int = feats[mask].long()
    t_val = thrs[mask]
    if bool(torch.isnan(t_val).any()):
        # x <= NaN is false for every x; a NaN has no place in a sorted
        # edge row, so such a forest keeps the raw walk
        return
    f_max = int(f_int.max()) + 1
    # sort by (feature, threshold)
    order = torch.argsort(t_val)
    f_s, t_s = f_int[order], t_val[order]
    order2 = torch.argsort(f_s, stable=True)
    p = order[order2]
    f_s, t_s = f_s[order2], t_s[order2]
    keep = torch.ones_like(f_s, dtype=torch.bool)
    keep[1:] = (f_s[1:] != f_s[:-1]) | (t_s[1:] != t_s[:-1])
    uidx = keep.long().cumsum(0) - 1
    fu, tu = f_s[keep], t_s[keep]
    counts = torch.bincount(fu, minlength=f_max)
    maxcnt = int(counts.max())
    if maxcnt > 255:
        return
    offs = torch.zeros(f_max + 1, dtype=torch.long, device=dev)
    offs[1:] = counts.cumsum(0)
    rank_sorted = uidx - offs[f_s]
    rank_node = torch.empty(m_cnt, dtype=torch.long, device=dev)
    rank_node[p] = rank_sorted
    rank_full = torch.zeros(feats.numel(), dtype=torch.int64, device=dev)
    rank_full[mask] = rank_node
    payload_bits = torch.where(
        mask,
        rank_full,
        payload.view(torch.int32).to(torch.int64) & 0xFFFFFFFF,
    )
    node64b = (
        (feats.to(torch.int64) & 0xFFFF)
        | ((pack["lefts"].to(torch.int64) & 0xFFFF) << 16)
        | (payload_bits << 32)
    ).contiguous()
    pack.update(
        binned_ok=True, node64b=node64b, bin_fu=fu, bin_tu=tu,
        bin_offs=offs, bin_maxcnt=max(maxcnt, 1), bin_fmax=f_max,
    )


def _binned_edges(pack, F):
    """[F, maxcnt] padded per-feature threshold sets for bin_features
    (pad = +inf: no threshold sorts above it, so every row stays sorted
    and lower_bound is unaffected — x = +inf gets the rank of a +inf
    threshold if the feature has one, else the count, and NaN still gets
    maxcnt); cached per F."""
    cached = pack.get("bedges")
    if cached is not None and cached.shape[0] == F:
        return cached
    dev = pack["dev"]
    mc = pack["bin_maxcnt"]
    edges = torch.full((F, mc), float("inf"), dtype=torch.float32, device=dev)
    fu, tu, offs = pack["bin_fu"], pack["bin_tu"], pack["bin_offs"]
    col = torch.arange(fu.numel(), device=dev) - offs[fu]
    edges[fu, col] = tu
    pack["bedges"] = edges
    return edges


def _run_fp2(m, x_in, pack, mode):
    """mode: 'raw' (f32 rows), 'binned' (u8 rank rows), 'binned_t'
    (transposed u8 — wave-coalesced top-level gathers)."""
    out = torch.zeros(x_in.shape[0], pack["D"], dtype=torch.float32,
                      device=x_in.device)
    if mode == "raw":
        m.forest_predict2(out, x_in, pack["node64"], pack["leaves"],
                          pack["offsets32"], pack["w"], pack["groups_t"],
                          pack["D"], pack["max_nodes"], 0)
        return out
    edges = _binned_edges(pack, x_in.shape[1])
    xb = torch.empty(x_in.shape, dtype=torch.uint8, device=x_in.device)
    m.bin_features(xb, x_in, edges)
    if mode == "binned_t":
        xbt = torch.empty(xb.shape[1], xb.shape[0], dtype=torch.uint8,
                          device=xb.device)
        m.transpose_u8(xbt, xb)
        xb = xbt
        m.forest_predict2(out, xb, pack["node64b"], pack["leaves"],
                          pack["offsets32"], pack["w"], pack["groups_t"],
                          pack["D"], pack["max_nodes"], 1)
    else:
        m.forest_predict2(out, xb, pack["node64b"], pack["leaves"],
                          pack["offsets32"], pack["w"], pack["groups_t"],
                          pack["D"], pack["max_nodes"], 0)
    return out


_SERVE_MODES = ("binned_t", "binned", "raw")


def _forest_predict_packed(m, x, pack):
    D = pack["D"]
    if x.shape[0] == 0:  # no launch: every kernel here sizes its grid by N
        return torch.zeros(0, D, dtype=torch.float32, device=x.device)
    if pack["v2"] and x.shape[1] < 32768 and hasattr(m, "forest_predict2"):
        xc = x.contiguous()
        env_mode = os.environ.get("SEA_SERVE_MODE")
        if os.environ.get("SEA_SERVE_RAW") == "1":
            env_mode = "raw"
        binned_avail = (
            pack.get("binned_ok") and pack["bin_fmax"] <= x.shape[1]
        )
        if not binned_avail:
            return _run_fp2(m, xc, pack, "raw")
        if env_mode in _SERVE_MODES:
            return _run_fp2(m, xc, pack, env_mode)
        # which walk mode wins depends on the forest's x-access pattern
        # (measured r02: binned 1.8x faster for a 100-tree GBM, raw 1.7x
        # faster for 50 subspace-bagged trees) — all modes are EXACT, so
        # on the first large batch time each once and remember the winner
        mode = pack.get("mode")
        if mode is None:
            if x.shape[0] < (1 << 20):
                return _run_fp2(m, xc, pack, "binned")  # small: either way
            import time

            probe = xc[: 1 << 19]
            times = {}
            for cand in _SERVE_MODES:
                _run_fp2(m, probe, pack, cand)  # warm
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _run_fp2(m, probe, pack, cand)
                torch.cuda.synchronize()
                times[cand] = time.perf_counter() - t0
            mode = min(times, key=times.get)
            pack["mode"] = mode
        return _run_fp2(m, xc, pack, mode)
    out = torch.zeros(x.shape[0], D, dtype=torch.float32, device=x.device)
    m.forest_predict(out, x.contiguous(), pack["feats"], pack["thrs"],
                     pack["lefts"], pack["leaves"], pack["offsets32"],
                     pack["w"], D)
    return out


# ---- per-row feature contributions (csrc/tree_contrib.hip) ---------------

CONTRIB_MAX_PATH = 32       # unique features on one path (lane group <= 32)
CONTRIB_LDS_BYTES = 163840  # the tile's i64 accumulators + f32 x rows
CONTRIB_MAX_ROWS = 64       # rows per tile once F is small enough
CONTRIB_MIN_ROWS = 4        # below this a path load is amortised too little
_CONTRIB_GROUPS = (8, 16, 32)

# what the last forest_contrib call did: {"path": "native" | "reference",
# "rows_per_tile": R} (tests assert the route without guessing the policy)
last_forest_contrib_info: dict = {}


def contrib_rows_per_tile(num_features: int) -> int:
    """Rows R of one LDS tile for F features: [R][F] i64 fixed-point
    accumulators plus [R][F] f32 of x within 160 KiB, capped at
    CONTRIB_MAX_ROWS.  The native kernel serves F while R >=
    CONTRIB_MIN_ROWS."""
    return min(CONTRIB_MAX_ROWS, CONTRIB_LDS_BYTES // (12 * int(num_features)))


def _pack_contrib(trees, weights, planes, num_planes, dev):
    """Path tables of the contribution kernel, built once per (model,
    device).  Paths are sorted by plane, then lane-group width, then m;
    ``ranges[p]`` holds plane p's bucket boundaries (8 | 16 | 32 | end)."""
    tb = reference.contrib_paths(trees, weights, planes, num_planes)
    pack = {"T": len(trees), "dev": dev, "num_planes": num_planes,
            "tables": tb, "bias": tb["bias"]}
    m = tb["m"]
    m_max = int(m.max()) if m.numel() else 0
    pack["m_max"] = m_max
    pack["f_max"] = int(tb["feat"].max()) if tb["feat"].numel() else -1
    # z <= 0 only comes from a node of zero cover and non-additive covers
    # only from hand-made dicts; no grower emits either.  The kernel's
    # factors assume z > 0, its fixed-point range additive covers.
    pack["native_ok"] = (
        m_max <= CONTRIB_MAX_PATH and tb["covers_additive"]
        and (tb["z"].numel() == 0 or bool((tb["z"] > 0).all()))
        and math.isfinite(tb["bound"]))
    if not pack["native_ok"]:
        return pack
    # power-of-two fixed-point scale: every partial sum of a cell stays
    # under 2 * bound, which the scale maps to 2^50 (the kernel's integer
    # conversion holds up to 2^51)
    pack["scale"] = 1.0
    if tb["bound"] > 0:
        pack["scale"] = 2.0 ** max(
            -1000, min(1000, 49 - math.frexp(tb["bound"])[1]))
    bucket = torch.bucketize(m, torch.tensor(_CONTRIB_GROUPS), right=False)
    key = (tb["plane"] * 4 + bucket) * (CONTRIB_MAX_PATH + 1) + m
    order = torch.argsort(key, stable=True)
    pb = (tb["plane"] * 4 + bucket)[order]
    # boundaries: first path of (plane p, bucket >= b) for b = 0..3
    ranges = torch.searchsorted(
        pb, torch.arange(num_planes * 4, dtype=torch.int64)
    ).reshape(num_planes, 4).clone()
    ends = torch.searchsorted(
        pb, (torch.arange(num_planes, dtype=torch.int64) + 1) * 4)
    ranges[:, 3] = ends
    feat_bits = (
        tb["feat"]
        | ((tb["flags"] & reference.CONTRIB_HAS_LO) != 0).long() << 29
        | ((tb["flags"] & reference.CONTRIB_HAS_HI) != 0).long() << 30
    )

    def up(t, dtype):
        return t.to(dtype).contiguous().to(dev)

    pack.update(
        ranges=up(ranges, torch.int32),
        path_off=up(tb["off"][order], torch.int32),
        path_m=up(m[order], torch.int32),
        path_plane=up(tb["plane"][order], torch.int32),
        path_v=up(tb["v"][order], torch.float32),
        e_feat=up(feat_bits, torch.int32),
        e_lo=up(tb["lo"], torch.float32),
        e_hi=up(tb["hi"], torch.float32),
        e_z=up(tb["z"], torch.float32),
        bias_dev=up(tb["bias"], torch.float32),
    )
    return pack


def forest_contrib(x, trees, weights=None, planes=None, num_planes=1,
                   cache=None):
    """Per-row additive feature contributions (path-dependent TreeSHAP) of
    a weighted forest: ``[N, num_planes, F + 1]`` f32, column F the bias;
    tree t adds its output d into plane ``planes[t] + d``.  Semantics:
    docs/contributions.md and ``reference.forest_contrib``.

    ``cache``: caller-owned dict; the path tables are built once per
    (model, device) and kept under "contrib_pack".  On the GPU the gfx950
    kernel computes the feature columns and the bias column (row-
    independent, summed in float64 on the host) is filled in here.  Forests
    with a path of more than CONTRIB_MAX_PATH unique features, and feature
    counts whose row tile falls under CONTRIB_MIN_ROWS, run the torch
    reference op on the same device.
    """
    if x.is_cuda and trees and x.dtype == torch.float32:
        m = _require_hip("forest_contrib")
        if m is not None:
            pack = cache.get("contrib_pack") if cache is not None else None
            if (pack is None or pack["T"] != len(trees)
                    or pack["dev"] != x.device
                    or pack["num_planes"] != num_planes):
                pack = _pack_contrib(trees, weights, planes, num_planes,
                                     x.device)
                if cache is not None:
                    cache["contrib_pack"] = pack
            N, F = x.shape
            if pack["f_max"] >= F:
                raise ValueError(
                    f"forest splits on feature {pack['f_max']} but x has "
                    f"{F} columns"
                )
            R = contrib_rows_per_tile(F)
            if pack["native_ok"] and R >= CONTRIB_MIN_ROWS:
                out = torch.empty(N, num_planes, F + 1, dtype=torch.float32,
                                  device=x.device)
                m.forest_contrib(
                    out, x.contiguous(), pack["ranges"], pack["path_off"],
                    pack["path_m"], pack["path_v"], pack["e_feat"],
                    pack["e_lo"], pack["e_hi"], pack["e_z"], int(R),
                    pack["scale"],
                )
                out[:, :, F] = pack["bias_dev"]
                last_forest_contrib_info.update(path="native",
                                                rows_per_tile=R)
                return out
            last_forest_contrib_info.update(path="reference",
                                            rows_per_tile=R)
            return reference.forest_contrib(
                x, trees, weights, planes, num_planes, tables=pack["tables"])
    last_forest_contrib_info.update(path="reference", rows_per_tile=0)
    return reference.forest_contrib(x, trees, weights, planes, num_planes)


# ---- per-stage loss curves (csrc/forest_staged.hip) -----------------------

STAGED_MAX_DIM = 8

# what the last forest_staged_loss call did: {"path": "native" |
# "reference", "mode": "binned" | "raw" | None, "rows_per_lane": R,
# "groups": G} (tests assert the route without guessing the policy)
last_forest_staged_info: dict = {}


def _staged_native_loss(loss, dim):
    """(loss id, param) when the kernel has ``loss``'s device form, else
    None: the nine built-in classes, dim > 1 only for logloss."""
    from ..boosting import losses as _losses

    builtin = {
        "squared": _losses.SquaredLoss, "absolute": _losses.AbsoluteLoss,
        "logcosh": _losses.LogCoshLoss,
        "scaledlogcosh": _losses.ScaledLogCoshLoss,
        "huber": _losses.HuberLoss, "quantile": _losses.QuantileLoss,
        "logloss": _losses.LogLoss, "exponential": _losses.ExponentialLoss,
        "bernoulli": _losses.BernoulliLoss,
    }
    if type(loss) is not builtin.get(getattr(loss, "name", None)):
        return None
    if loss.dim != dim or (dim > 1 and loss.name != "logloss"):
        return None
    return loss.loss_id, float(loss.param)


def forest_staged_loss(x, trees, weights, dim, init, label, row_weight, loss,
                       cache=None):
    """Per-stage weighted loss sums ``[S + 1]`` float64 of a boosted forest
    of ``S * dim`` scalar-leaf trees in stage-major order; semantics in
    ``reference.forest_staged_loss``.  The result is on the device of x.

    On the GPU one fused pass (csrc/forest_staged.hip) serves ``dim <=
    STAGED_MAX_DIM`` when the forest packs as v2 (every tree within
    ``_FP2_GROUP_NODES``) and the loss is one of the built-in nine;
    anything else runs the torch reference op on the same device.  Rows
    are read as u8 ranks (``bin_features`` against the pack's threshold
    sets, as ``forest_predict2``) whenever the pack has them, else as f32;
    ``SEA_STAGED_MODE=raw|binned`` overrides.  Both are exact.

    ``cache``: caller-owned dict; the pack is built once per (forest,
    device) and kept under "pack", as ``forest_predict`` keeps its own.
    """
    dim = int(dim)
    if len(trees) % dim:
        raise ValueError(
            f"{len(trees)} trees are not whole stages of {dim} trees")
    native = x.is_cuda and x.dtype == torch.float32 and dim <= STAGED_MAX_DIM
    lp = _staged_native_loss(loss, dim) if native else None
    m = _require_hip("forest_staged_loss") if lp is not None else None
    if m is not None and any(t["leaf_value"].shape[1] != 1 for t in trees):
        m = None
    if m is not None:
        N, F = x.shape
        pack = None
        if trees:
            pack = cache.get("pack") if cache is not None else None
            if (pack is None or pack["T"] != len(trees)
                    or pack["dev"] != x.device):
                w = torch.as_tensor(
                    [float(v) for v in weights], dtype=torch.float32)
                pack = _pack_forest(trees, w, x.device)
                if cache is not None:
                    cache["pack"] = pack
            if "f_max" not in pack:
                pack["f_max"] = int(pack["feats"].max())
            if pack["f_max"] >= F:
                raise ValueError(
                    f"forest splits on feature {pack['f_max']} but x has "
                    f"{F} columns")
        if (pack is None or pack["v2"]) and 1 <= F < 32768 and N >= 1:
            threads, rpl, _ = m.forest_staged_geometry()
            S1 = len(trees) // dim + 1
            n_slots = -(-N // (threads * rpl)) * (threads // 64)
            out = torch.empty(S1, dtype=torch.float64, device=x.device)
            partials = torch.empty(n_slots, S1, dtype=torch.float64,
                                   device=x.device)
            xc = x.contiguous()
            mode = "raw"
            if pack is None:
                nodes = torch.empty(0, dtype=torch.int64, device=x.device)
                tree_off = torch.empty(0, dtype=torch.int32, device=x.device)
                groups = torch.empty(0, 4, dtype=torch.int32, device=x.device)
                max_nodes = 0
            else:
                binned_avail = bool(
                    pack.get("binned_ok") and pack["bin_fmax"] <= F)
                env_mode = os.environ.get("SEA_STAGED_MODE")
                if binned_avail and env_mode != "raw":
                    mode = "binned"
                elif env_mode == "binned":
                    raise ValueError(
                        "SEA_STAGED_MODE=binned: this forest has no u8 rank "
                        "form (a feature with more than 255 thresholds, or "
                        "no split at all)")
                tree_off, groups = pack["offsets32"], pack["groups_t"]
                max_nodes = pack["max_nodes"]
                if mode == "binned":
                    nodes = pack["node64b"]
                    xb = torch.empty(xc.shape, dtype=torch.uint8,
                                     device=x.device)
                    m.bin_features(xb, xc, _binned_edges(pack, F))
                    xc = xb
                else:
                    nodes = pack["node64"]

            def f32(t, shape):
                return t.to(x.device, torch.float32).reshape(shape).contiguous()

            m.forest_staged_loss(
                out, partials, xc, nodes, tree_off, groups,
                f32(init, (N, dim)), f32(label, (N, dim)),
                f32(row_weight, (N,)), dim, int(max_nodes), int(lp[0]),
                float(lp[1]),
            )
            last_forest_staged_info.update(
                path="native", mode=mode, rows_per_lane=int(rpl),
                groups=int(groups.shape[0]))
            return out
    last_forest_staged_info.update(path="reference", mode=None,
                                   rows_per_lane=0, groups=0)
    return reference.forest_staged_loss(
        x, trees, weights, dim, init, label, row_weight, loss)


# ---- out-of-bag sums and counts (csrc/forest_oob.hip) ---------------------

OOB_MAX_DIM = 8
_OOB_PACK_ROWS = 1 << 20  # rows per step of the mask packing (256 MiB of i64)

# what the last forest_oob call did: {"path": "native" | "reference",
# "mode": "binned" | "raw" | None, "rows_per_lane": R, "groups": G}
last_forest_oob_info: dict = {}


def _pack_inbag(inbag):
    """``[N, T]`` bool -> ``[ceil(T / 32), N]`` int32: word ``t >> 5``, bit
    ``t & 31`` set where row i is in tree t's bag.  Word-major, so
    consecutive lanes of the kernel read consecutive words.  Built in int64
    and wrapped to int32 (bit 31 is the sign bit)."""
    N, T = inbag.shape
    W = -(-T // 32)
    out = torch.empty(W, N, dtype=torch.int32, device=inbag.device)
    shifts = torch.arange(32, dtype=torch.int64, device=inbag.device)
    for wd in range(W):
        cols = inbag[:, wd * 32:(wd + 1) * 32]
        for r0 in range(0, N, _OOB_PACK_ROWS):
            c = cols[r0:r0 + _OOB_PACK_ROWS].to(torch.int64)
            v = (c << shifts[:c.shape[1]]).sum(dim=1)
            v = torch.where(v >= 2 ** 31, v - 2 ** 32, v)
            out[wd, r0:r0 + _OOB_PACK_ROWS] = v.to(torch.int32)
    return out


def forest_oob(x, trees, inbag, cache=None):
    """Out-of-bag leaf sums ``[N, D]`` f32 and counts ``[N]`` int32 of a
    bagged forest under the ``[N, T]`` bool mask ``inbag`` (True: row i was
    in tree t's bag); semantics in ``reference.forest_oob``.  No tree
    weights.  Both results are on the device of x.

    On the GPU one pass (csrc/forest_oob.hip) computes both; a lane skips
    the walk of a tree whose bag held its row.  It serves f32 rows, ``D <= OOB_MAX_DIM`` and forests
    that pack as v2 (every tree within ``_FP2_GROUP_NODES``); anything else
    runs the torch reference op on the same device.  Rows are read as u8
    ranks (``bin_features`` against the pack's threshold sets, as
    ``forest_predict2``) whenever the pack has them, else as f32;
    ``SEA_OOB_MODE=raw|binned`` overrides.  Both are exact.

    ``cache``: caller-owned dict; the pack (tree weights all 1.0) is built
    once per (forest, device) and kept under "pack".  Keep a dict of its
    own for this op: the other forest ops reuse whatever pack they find
    under that key by tree count and device alone, and theirs carry tree
    weights.  A weighted pack found here is not used (and not replaced),
    so sharing costs a pack per call here and wrong weights there.
    """
    if not trees:
        raise ValueError("forest_oob needs at least one tree")
    N, F = x.shape
    inbag = torch.as_tensor(inbag)
    if inbag.dim() != 2 or tuple(inbag.shape) != (N, len(trees)):
        raise ValueError(
            f"inbag is {tuple(inbag.shape)}, expected ({N}, {len(trees)})")
    D = trees[0]["leaf_value"].shape[1]
    # N == 0 launches nothing and packs nothing: the reference route below
    # returns the empty tensors
    native = (x.is_cuda and x.dtype == torch.float32 and D <= OOB_MAX_DIM
              and N >= 1)
    m = _require_hip("forest_oob") if native else None
    if m is not None:
        pack = cache.get("pack") if cache is not None else None
        fits = (pack is not None and pack["T"] == len(trees)
                and pack["dev"] == x.device)
        if not (fits and pack.get("unit_weights")):
            pack = _pack_forest(trees, None, x.device)
            pack["unit_weights"] = True
            # a weighted pack of the same forest belongs to another op
            # (forest_predict folds tree weights into the D == 1 payload):
            # it is neither used here nor replaced
            if cache is not None and not fits:
                cache["pack"] = pack
        if "f_max" not in pack:
            pack["f_max"] = int(pack["feats"].max())
        if pack["f_max"] >= F:
            raise ValueError(
                f"forest splits on feature {pack['f_max']} but x has "
                f"{F} columns")
        if pack["v2"] and 1 <= F < 32768:
            _, rpl, _ = m.forest_oob_geometry()
            binned_avail = bool(
                pack.get("binned_ok") and pack["bin_fmax"] <= F)
            env_mode = os.environ.get("SEA_OOB_MODE")
            mode = "raw"
            if binned_avail and env_mode != "raw":
                mode = "binned"
            elif env_mode == "binned":
                raise ValueError(
                    "SEA_OOB_MODE=binned: this forest has no u8 rank form "
                    "(a feature with more than 255 thresholds, or no split "
                    "at all)")
            xc = x.contiguous()
            if mode == "binned":
                nodes = pack["node64b"]
                xb = torch.empty(xc.shape, dtype=torch.uint8, device=x.device)
                m.bin_features(xb, xc, _binned_edges(pack, F))
                xc = xb
            else:
                nodes = pack["node64"]
            mask = _pack_inbag(inbag.to(x.device, torch.bool))
            sums = torch.empty(N, D, dtype=torch.float32, device=x.device)
            counts = torch.empty(N, dtype=torch.int32, device=x.device)
            groups = pack["groups_t"]
            m.forest_oob(sums, counts, xc, nodes, pack["leaves"],
                         pack["offsets32"], groups, mask, D,
                         int(pack["max_nodes"]))
            last_forest_oob_info.update(
                path="native", mode=mode, rows_per_lane=int(rpl),
                groups=int(groups.shape[0]))
            return sums, counts
    last_forest_oob_info.update(path="reference", mode=None,
                                rows_per_lane=0, groups=0)
    f_max = max(int(t["feature"].max()) for t in trees)
    if f_max >= F:
        raise ValueError(
            f"forest splits on feature {f_max} but x has {F} columns")
    if x.shape[0] == 0:
        return (torch.empty(0, D, dtype=x.dtype, device=x.device),
                torch.empty(0, dtype=torch.int32, device=x.device))
    return reference.forest_oob(x, trees, inbag)


# ---- permutation loss sums (csrc/forest_permute.hip) ----------------------

# what the last forest_permute_loss call did: {"path": "native" |
# "reference", "mode": "binned" | "raw" | None, "feature_chunk": FC,
# "groups": G}
last_forest_permute_info: dict = {}


def forest_permute_geometry():
    """(threads, rows per lane, row-tile grid cap, features per chunk, nodes
    per LDS group, depth cap or 0) of the native ``forest_permute_loss``."""
    return tuple(int(v) for v in
                 _require_hip("forest_permute_loss").forest_permute_geometry())


def _permute_groups(pack, budget):
    """The trees of a v2 ``pack`` cut into contiguous groups of at most
    ``budget`` nodes: ``(groups [G, 4] int32, max_nodes)`` in the layout of
    ``pack["groups_t"]``, over the same node arena, or None when one tree
    alone is over the budget.  ``forest_permute_loss`` shares the LDS
    between its accumulators and the nodes, so its groups are smaller than
    ``_FP2_GROUP_NODES``; the pack's own groups stay as the other ops read
    them.  Cached on the pack per budget."""
    key = ("permute_groups", int(budget))
    if key not in pack:
        offs = pack["offsets32"].cpu().tolist() + [int(pack["feats"].numel())]
        sizes = [offs[t + 1] - offs[t] for t in range(pack["T"])]
        if max(sizes) > budget:
            pack[key] = None
        else:
            groups, first, acc = [], 0, 0
            for t, s in enumerate(sizes):
                if acc + s > budget and acc > 0:
                    groups.append([first, t - first, offs[first], acc])
                    first, acc = t, 0
                acc += s
            groups.append([first, pack["T"] - first, offs[first], acc])
            pack[key] = (
                torch.tensor(groups, dtype=torch.int32, device=pack["dev"]),
                max(g[3] for g in groups))
    return pack[key]


def forest_permute_loss(x, trees, weights, init, label, row_weight, loss,
                        donor, cache=None):
    """``(base, perm)``: the weighted loss sum of a forest of scalar-leaf
    trees on ``x`` (float64 scalar) and the same sum with column f replaced
    by ``x[donor[r], f]`` for every repeat r and feature f (float64
    ``[R, F]``); semantics in ``reference.forest_permute_loss``.  Both
    results are on the device of x.

    On the GPU one launch (csrc/forest_permute.hip) serves f32 rows, the
    built-in nine losses at ``dim == 1``, forests that pack as v2 with every
    tree within the op's own LDS group budget (``forest_permute_geometry``)
    and ``donor`` of at most 65535 repeats; anything else runs the torch
    reference op on the same device.  Rows are read as u8 ranks
    (``bin_features`` against the pack's threshold sets, as
    ``forest_predict2``) whenever the pack has them, else as f32;
    ``SEA_PERMUTE_MODE=raw|binned`` overrides.  Both are exact.

    ``cache``: caller-owned dict; the weighted pack is built once per
    (forest, device) and kept under "pack", as ``forest_staged_loss`` keeps
    its own.
    """
    N, F = x.shape
    donor = torch.as_tensor(donor)
    if donor.dim() != 2 or donor.shape[1] != N:
        raise ValueError(
            f"donor is {tuple(donor.shape)}, expected (R, {N})")
    R = donor.shape[0]
    if N and R and (int(donor.min()) < 0 or int(donor.max()) >= N):
        raise ValueError(f"donor holds an index outside [0, {N})")
    if N == 0:  # no launch, no pack
        last_forest_permute_info.update(
            path="reference", mode=None, feature_chunk=0, groups=0)
        return (torch.zeros((), dtype=torch.float64, device=x.device),
                torch.zeros(R, F, dtype=torch.float64, device=x.device))

    native = (x.is_cuda and x.dtype == torch.float32 and bool(trees)
              and 1 <= F < 32768 and N < 2 ** 31 and 1 <= R <= 65535
              and all(t["leaf_value"].shape[1] == 1 for t in trees))
    lp = _staged_native_loss(loss, 1) if native else None
    m = _require_hip("forest_permute_loss") if lp is not None else None
    if m is not None:
        pack = cache.get("pack") if cache is not None else None
        if (pack is None or pack["T"] != len(trees)
                or pack["dev"] != x.device):
            w = torch.as_tensor(
                [float(v) for v in weights], dtype=torch.float32)
            pack = _pack_forest(trees, w, x.device)
            if cache is not None:
                cache["pack"] = pack
        threads, _, max_blocks, fc, budget, _ = (
            int(v) for v in m.forest_permute_geometry())
        if "f_max" not in pack:
            pack["f_max"] = int(pack["feats"].max())
        if pack["f_max"] >= F:
            raise ValueError(
                f"forest splits on feature {pack['f_max']} but x has "
                f"{F} columns")
        # the kernel has no depth cap (geometry's last entry is 0)
        grp = _permute_groups(pack, budget) if pack["v2"] else None
        if grp is not None:
            groups, max_nodes = grp
            binned_avail = bool(
                pack.get("binned_ok") and pack["bin_fmax"] <= F)
            env_mode = os.environ.get("SEA_PERMUTE_MODE")
            mode = "raw"
            if binned_avail and env_mode != "raw":
                mode = "binned"
            elif env_mode == "binned":
                raise ValueError(
                    "SEA_PERMUTE_MODE=binned: this forest has no u8 rank "
                    "form (a feature with more than 255 thresholds, or no "
                    "split at all)")
            xc = x.contiguous()
            if mode == "binned":
                nodes = pack["node64b"]
                xb = torch.empty(xc.shape, dtype=torch.uint8, device=x.device)
                m.bin_features(xb, xc, _binned_edges(pack, F))
                xc = xb
            else:
                nodes = pack["node64"]
            C = R * F + 1
            n_slots = min(-(-N // threads), max_blocks) * (threads // 64)
            out = torch.empty(C, dtype=torch.float64, device=x.device)
            partials = torch.empty(n_slots, C, dtype=torch.float64,
                                   device=x.device)

            def f32(t):
                return t.to(x.device, torch.float32).reshape(N).contiguous()

            m.forest_permute_loss(
                out, partials, xc, nodes, pack["offsets32"], groups,
                f32(init), f32(label), f32(row_weight),
                donor.to(x.device, torch.int32).contiguous(),
                int(max_nodes), int(lp[0]), float(lp[1]))
            last_forest_permute_info.update(
                path="native", mode=mode, feature_chunk=fc,
                groups=int(groups.shape[0]))
            return out[C - 1], out[:C - 1].view(R, F)
    last_forest_permute_info.update(
        path="reference", mode=None, feature_chunk=0, groups=0)
    f_max = max([int(t["feature"].max()) for t in trees], default=-1)
    if f_max >= F:
        raise ValueError(
            f"forest splits on feature {f_max} but x has {F} columns")
    return reference.forest_permute_loss(
        x, trees, weights, init, label, row_weight, loss, donor)


def logreg_loss_grad(x, y_int, w, wmat, has_bias):
    """Single-pass fused logistic loss+gradient.

    Returns payload [1 + (F+1)*K]: [loss_sum, grad(F,K) flat, grad_bias(K)]
    (unnormalized sums; caller all-reduces and divides by total weight).
    On GPU uses the hand-written gfx950 kernel (csrc/linear.hip) when the
    (F, K) shape fits the register budget, else the torch fallback.
    """
    f = x.shape[1]
    k = wmat.shape[1]
    if x.is_cuda:
        m = _require_hip("logreg_loss_grad")
        if m is not None and m.logreg_fused_supported(f, k):
            payload = torch.zeros(
                1 + (f + 1) * k, dtype=torch.float32, device=x.device
            )
            m.logreg_loss_grad(
                payload, x.contiguous(), y_int.contiguous(),
                w.contiguous(), wmat.contiguous(), bool(has_bias),
            )
            return payload
    return reference.logreg_loss_grad(x, y_int, w, wmat, has_bias)
