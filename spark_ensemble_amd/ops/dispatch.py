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


def goss_geometry(n):
    """How the native goss_weights cuts ``n`` rows: ``tile_rows`` consecutive
    rows per tile, ``tiles``, ``blocks`` (block b takes tiles b, b + blocks,
    ..., so one grid round covers ``blocks * tile_rows`` rows), the
    ``digit_bits`` of the three radix passes, the ``slot_bytes`` of the
    per-block histogram slots and ``max_blocks``, the grid cap."""
    m = _require_hip("goss_geometry")
    if m is None:
        raise RuntimeError("goss_geometry needs the HIP extension")
    tile, tiles, blocks, b0, b1, b2, slot_bytes, cap = m.goss_geometry(int(n))
    return {"tile_rows": int(tile), "tiles": int(tiles),
            "blocks": int(blocks), "digit_bits": (int(b0), int(b1), int(b2)),
            "slot_bytes": int(slot_bytes), "max_blocks": int(cap)}


def goss_weights(g, w, top_rate, other_rate, seed, rank=0):
    """GOSS row multiplicities ``[N]`` f32 from the gradient matrix ``g``
    [N, D] and the row weights ``w`` [N]; semantics in
    ``reference.goss_weights`` and docs/gbm.md.  On the GPU the selection is
    the radix select of csrc/goss.hip: no sort, no host sync."""
    if g.is_cuda:
        m = _require_hip("goss_weights")
        if m is not None:
            n = g.shape[0]
            g2 = g.to(torch.float32).reshape(n, -1).contiguous()
            k, p_other, amp = reference.goss_params(top_rate, other_rate, n)
            out = torch.empty(n, dtype=torch.float32, device=g.device)
            if n == 0:  # a 0-block grid is not a valid launch
                return out
            m.goss_weights(out, g2, w.to(torch.float32).contiguous(), k,
                           p_other, amp, int(seed), int(rank))
            return out
    return reference.goss_weights(g, w, top_rate, other_rate, seed, rank)


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


def round_fused_enabled() -> bool:
    """``SEA_ROUND_FUSED=0`` keeps the dim-1 GBM round on its composed
    prologue (sample_weights, grad_hess, neg, mul, the base learner's fit
    statistics and the grower's cat); read at every call."""
    return os.environ.get("SEA_ROUND_FUSED", "1") != "0"


def gbm_round_prologue_geometry(n):
    """(threads per block, blocks) of the native gbm_round_prologue at ``n``
    rows; one trip of its grid-stride loop covers threads * blocks rows."""
    m = _require_hip("gbm_round_prologue_geometry")
    if m is None:
        raise RuntimeError("gbm_round_prologue_geometry needs the HIP "
                           "extension")
    threads, blocks = m.gbm_round_prologue_geometry(int(n))
    return int(threads), int(blocks)


def gbm_round_prologue(label, pred, weight, loss, unit_weight):
    """What a dim-1 gradient-boosting round needs from its rows before the
    tree grows, in one pass: ``(gh, grad, gmax)`` with ``grad = weight *
    (-g)`` [N] for the gradient ``g`` of the scalar ``loss`` at (``label``,
    ``pred``) [N, 1], ``gh`` the grower's [N, C] matrix (``(grad, weight)``
    when ``unit_weight``, a fact about ``weight`` the caller vouches for,
    else ``(grad, weight, 1)``) and ``gmax`` the one-element ``max |grad|``,
    NaN when a gradient is NaN.  The gradient sum is left to the caller
    (``grad.sum``): its order is part of the fitted model."""
    if pred.is_cuda:
        m = _require_hip("gbm_round_prologue")
        if m is not None:
            n = pred.shape[0]
            c = 2 if unit_weight else 3
            gh = torch.empty(n, c, dtype=torch.float32, device=pred.device)
            grad = torch.empty(n, dtype=torch.float32, device=pred.device)
            if n == 0:  # a 0-block grid is not a valid launch
                return gh, grad, grad.new_zeros(1)
            gmax = torch.empty(1, dtype=torch.float32, device=pred.device)
            m.gbm_round_prologue(
                gh, grad, gmax, label.contiguous(), pred.contiguous(),
                weight.contiguous(), loss.loss_id, float(loss.param),
                bool(unit_weight),
            )
            return gh, grad, gmax
    return reference.gbm_round_prologue(label, pred, weight, loss, unit_weight)


def level_fused_enabled() -> bool:
    """``SEA_LEVEL_FUSED=0`` keeps the tree level loop on the composed ops
    (assemble + split_search + pack, device-side left counts); read at every
    call."""
    return os.environ.get("SEA_LEVEL_FUSED", "1") != "0"


def level_chain_enabled() -> bool:
    """``SEA_LEVEL_CHAIN=0`` keeps every tree level planned on the host, after
    the partition's row counts have arrived; read at every call."""
    return os.environ.get("SEA_LEVEL_CHAIN", "1") != "0"


def level_plan(cursors, child, max_abs, rows_bound, src_rows, gh_cols,
               num_features, num_bins, d_dims, c_per_node):
    """Plan the next level's histogram build on the device.

    ``cursors`` is the partition's device cursor table [n_pairs, 2] (it may
    still be being written), ``child`` a host int32 [n, 5] table of (pair,
    1 if right child, gh col0, parent start, parent end) per built child,
    ``rows_bound`` at least the rows of those parents.  Returns the device
    tables (table, seg): ``table`` is what ``hist_build_planned`` launches
    from -- C scales, the record and slot counts, padding to 2 C words, the
    chunk records, the slot records -- and ``seg`` the int64 [3 n + 1]
    compact offsets, source starts and col0 of the ranges to gather."""
    m = _require_hip("level_plan")
    return m.level_plan(
        cursors, child.to(torch.int32).cpu().contiguous(),
        max_abs.to(torch.float32).cpu(), int(rows_bound), int(src_rows),
        int(gh_cols), int(num_features), int(num_bins), int(d_dims),
        int(c_per_node),
    )


def hist_build_planned(bins, gh, row_idx, table, n_nodes, num_bins, d_dims):
    """``hist_build_forest(..., gh_by_position=True)`` from a ``level_plan``
    table: gh [R, C] and row_idx [R] are filled up to the planned total, the
    grid is sized by the planner's bound."""
    m = _require_hip("hist_build_planned")
    out = torch.empty(n_nodes, bins.shape[1], num_bins, gh.shape[1],
                      dtype=torch.float32, device=bins.device)
    m.hist_build_planned(out, bins, gh, row_idx, table, int(num_bins),
                         int(d_dims))
    return out


def level_chain_hist(bins, gh, new_rows, cursors, child, max_abs, rows_bound,
                     num_bins, d_dims, c_per_node):
    """The built children's histograms [n, F, B, C] of the next level, queued
    behind the partition that fills ``new_rows`` and ``cursors`` without
    waiting for it: ``level_plan``, the gather of their rows and gradients,
    ``hist_build_planned``.  ``child`` as in :func:`level_plan`."""
    m = _require_hip("level_chain_hist")
    out = torch.empty(child.shape[0], bins.shape[1], num_bins, c_per_node,
                      dtype=torch.float32, device=bins.device)
    m.level_chain_hist(out, bins, gh, new_rows, cursors, child, max_abs,
                       int(rows_bound), int(num_bins), int(d_dims))
    return out


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
        # the device table rides along for level_chain_hist
        return new_rows, (cur_h, ev, cursors), offs_cpu
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
        lc_h, ev = left_counts[:2]
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


# ---- vote sums of 9-32 class forests (csrc/forest_vote.hip) ---------------

VOTE_MIN_CLASSES = 9    # below: forest_predict2 / forest_oob serve the forest
VOTE_MAX_CLASSES = 32   # a row's counters are 32 16-bit register fields
VOTE_MAX_MEMBERS = 65535  # what one 16-bit counter field holds

# what the last forest_vote call did: {"path": "native" | "reference",
# "mode": "binned" | "raw" | None, "vote": "hard" | "soft", "kp": KP (the
# soft table width; 32 for hard votes), "rows_per_lane": R, "groups": G}
last_forest_vote_info: dict = {}


def forest_vote_geometry():
    """``{"threads", "rows_per_lane": {"hard", 12, 16, 24, 32}, "grid_cap"}``
    of the native ``forest_vote``: a block's row tile is ``threads *
    rows_per_lane[...]``, keyed by "hard" or by the soft table width KP."""
    m = _require_hip("forest_vote_geometry")
    if m is None:
        raise RuntimeError("forest_vote_geometry needs the HIP extension")
    th, hard, s12, s16, s24, s32, cap = m.forest_vote_geometry()
    return {"threads": int(th), "grid_cap": int(cap),
            "rows_per_lane": {"hard": int(hard), 12: int(s12), 16: int(s16),
                              24: int(s24), 32: int(s32)}}


def _vote_kp(K):
    """Soft leaf-table width of a K-class forest: the kernel's compile-time
    widths are 12, 16, 24 and 32."""
    return 12 if K <= 12 else 16 if K <= 16 else 24 if K <= 24 else 32


def _pack_forest_vote(trees, soft, dev):
    """Pack voting trees (``leaf_value`` ALREADY transformed per node, as
    ``ensemble.utils._vote_leaves`` does) for ``forest_vote``: the node
    words and groups of ``_pack_forest``, with other payloads.

    Hard: a leaf's payload is its class id, the argmax of its one-hot row,
    and there is no leaf tensor.  Soft: a leaf's payload is its row in
    ``table`` ``[n_leaves, KP]`` f32, the leaf rows in node order zero-padded
    to KP columns; inner nodes have no row.  Both carry ``node64`` (f32
    thresholds) and, through ``_pack_forest_binned``, ``node64b`` and the
    rank structures.  ``fits`` is False, and nothing else is packed, when a
    tree exceeds the LDS group budget."""
    sizes = [t["feature"].numel() for t in trees]
    T = len(trees)
    K = trees[0]["leaf_value"].shape[1]
    pack = {"T": T, "K": K, "dev": dev, "soft": bool(soft),
            "kp": _vote_kp(K) if soft else 32,
            "fits": max(sizes) <= _FP2_GROUP_NODES}
    if not pack["fits"]:
        return pack
    feats = torch.cat([t["feature"].to(dev, torch.int32) for t in trees])
    thrs = torch.cat([t["threshold"].to(dev, torch.float32) for t in trees])
    lefts = torch.cat([t["left_child"].to(dev, torch.int32) for t in trees])
    leaves = torch.cat([t["leaf_value"].to(dev, torch.float32) for t in trees])
    is_leaf = feats < 0
    if soft:
        ids = (is_leaf.to(torch.int32).cumsum(0) - 1).to(torch.int32)
        table = torch.zeros(int(is_leaf.sum()), pack["kp"],
                            dtype=torch.float32, device=dev)
        table[:, :K] = leaves[is_leaf]
        pack["table"] = table.contiguous()
    else:
        ids = leaves.argmax(dim=1).to(torch.int32)
        pack["table"] = torch.empty(0, dtype=torch.float32, device=dev)
    # integer select: the payload bits of a leaf are an index, not a float
    payload = torch.where(is_leaf, ids, thrs.view(torch.int32)).view(
        torch.float32)
    offsets = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0)
    pack.update(
        feats=feats, lefts=lefts, f_max=int(feats.max()),
        offsets32=offsets.to(torch.int32).to(dev),
        node64=(
            (feats.to(torch.int64) & 0xFFFF)
            | ((lefts.to(torch.int64) & 0xFFFF) << 16)
            | ((payload.view(torch.int32).to(torch.int64) & 0xFFFFFFFF) << 32)
        ).contiguous())

    # greedy contiguous tree groups under the LDS node budget
    groups, off_list = [], offsets.tolist()
    first = acc = 0
    for t in range(T):
        if acc + sizes[t] > _FP2_GROUP_NODES and acc > 0:
            groups.append([first, t - first, off_list[first], acc])
            first, acc = t, 0
        acc += sizes[t]
    groups.append([first, T - first, off_list[first], acc])
    pack.update(
        groups_t=torch.tensor(groups, dtype=torch.int32, device=dev),
        max_nodes=max(g[3] for g in groups))
    _pack_forest_binned(pack, feats, thrs, payload)
    return pack


def forest_vote(x, trees, soft, inbag=None, cache=None, native_only=False):
    """Vote sums ``[N, K]`` f32 of a K-class voting forest: member t adds
    its leaf's row to the row's sums, members in order.  With ``inbag``
    (``[N, T]`` bool, True: row i was in tree t's bag) only the members
    that left the row out are summed and the result is ``(sums, counts
    [N] int32)``, the semantics of ``reference.forest_oob``.

    ``trees`` carry leaves ALREADY transformed per node, as
    ``ensemble.utils._vote_leaves`` makes and caches them: one-hot argmax
    rows for hard votes (``soft=False``), normalised probability rows for
    soft ones.  The packer reads class ids (hard) or the compact leaf table
    (soft) from them, and the declined route uses them as they are.

    The native pass (csrc/forest_vote.hip) serves CUDA f32 rows,
    ``9 <= K <= 32``, every tree within ``_FP2_GROUP_NODES``,
    ``1 <= F < 32768``, ``T <= 65535`` and ``N >= 1``.  Anything else
    returns what ``forest_predict`` / ``forest_oob`` return (or None under
    ``native_only``); ``SEA_VOTE_WIDE=0`` forces that route.  Hard sums
    are exact integers; soft sums are f32 adds in member order, bitwise
    those of the declined route.  Rows are read as u8 ranks whenever the
    pack has them, else as f32 (``forest_oob``'s rule);
    ``SEA_VOTE_MODE=raw|binned`` overrides.  Both are exact.

    ``cache``: caller-owned dict; the pack is kept under "vote_pack", a
    key no other forest op reads.  Keep one dict per voting strategy."""
    if not trees:
        raise ValueError("forest_vote needs at least one tree")
    N, F = x.shape
    T = len(trees)
    K = trees[0]["leaf_value"].shape[1]
    vote = "soft" if soft else "hard"
    if inbag is not None:
        inbag = torch.as_tensor(inbag)
        if inbag.dim() != 2 or tuple(inbag.shape) != (N, T):
            raise ValueError(
                f"inbag is {tuple(inbag.shape)}, expected ({N}, {T})")
    native = (x.is_cuda and x.dtype == torch.float32 and N >= 1
              and VOTE_MIN_CLASSES <= K <= VOTE_MAX_CLASSES
              and 1 <= F < 32768 and T <= VOTE_MAX_MEMBERS
              and os.environ.get("SEA_VOTE_WIDE") != "0")
    m = _require_hip("forest_vote") if native else None
    if m is not None:
        pack = cache.get("vote_pack") if cache is not None else None
        if (pack is None or pack["T"] != T or pack["dev"] != x.device
                or pack["soft"] != bool(soft) or pack["K"] != K):
            pack = _pack_forest_vote(trees, soft, x.device)
            if cache is not None:
                cache["vote_pack"] = pack
        if pack["fits"]:
            if pack["f_max"] >= F:
                raise ValueError(
                    f"forest splits on feature {pack['f_max']} but x has "
                    f"{F} columns")
            binned_avail = bool(
                pack.get("binned_ok") and pack["bin_fmax"] <= F)
            env_mode = os.environ.get("SEA_VOTE_MODE")
            mode = "raw"
            if binned_avail and env_mode != "raw":
                mode = "binned"
            elif env_mode == "binned":
                raise ValueError(
                    "SEA_VOTE_MODE=binned: this forest has no u8 rank form "
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
            sums = torch.empty(N, K, dtype=torch.float32, device=x.device)
            if inbag is not None:
                mask = _pack_inbag(inbag.to(x.device, torch.bool))
                counts = torch.empty(N, dtype=torch.int32, device=x.device)
            else:
                mask = counts = torch.empty(0, dtype=torch.int32,
                                            device=x.device)
            groups = pack["groups_t"]
            m.forest_vote(sums, counts, xc, nodes, pack["table"],
                          pack["offsets32"], groups, mask, K, bool(soft),
                          inbag is not None, int(pack["max_nodes"]))
            rpl = forest_vote_geometry()["rows_per_lane"]
            last_forest_vote_info.update(
                path="native", mode=mode, vote=vote, kp=pack["kp"],
                rows_per_lane=rpl[pack["kp"] if soft else "hard"],
                groups=int(groups.shape[0]))
            return sums if inbag is None else (sums, counts)
    last_forest_vote_info.update(path="reference", mode=None, vote=vote,
                                 kp=0, rows_per_lane=0, groups=0)
    if native_only:
        return None
    if inbag is None:
        return forest_predict(x, trees, None, cache=cache)
    return forest_oob(x, trees, inbag, cache=cache)


# ---- margins of a multi-plane boosted forest (csrc/forest_margin.hip) -----

# what the last forest_margin call did: {"path": "native" | "reference",
# "mode": "binned" | "raw" | None, "rows_per_lane": R, "groups": G,
# "planes": P}
last_forest_margin_info: dict = {}


def forest_margin_geometry():
    """``{"threads", "rows_per_lane", "grid_cap"}`` of the native
    ``forest_margin``: a block's row tile is ``threads * rows_per_lane``."""
    m = _require_hip("forest_margin_geometry")
    if m is None:
        raise RuntimeError("forest_margin_geometry needs the HIP extension")
    th, rows, cap = m.forest_margin_geometry()
    return {"threads": int(th), "rows_per_lane": int(rows),
            "grid_cap": int(cap)}


def _pack_forest_margin(trees, weights, planes, dev):
    """Pack scalar-leaf trees PLANE-MAJOR for ``forest_margin``: ``order`` is
    the stable sort of the tree indices by plane (stage order survives inside
    a plane) and every tensor below is in that order.  The node words and
    groups are those of ``_pack_forest`` at ``D == 1`` (a leaf's payload is
    the f32 bits of ``weight * leaf``); ``planes_t`` is the per-tree int32
    plane table beside ``offsets32``.  ``fits`` is False, and nothing else is
    packed, when a tree exceeds the LDS group budget."""
    T = len(trees)
    order = sorted(range(T), key=planes.__getitem__)  # stable
    trees = [trees[i] for i in order]
    sizes = [t["feature"].numel() for t in trees]
    pack = {"T": T, "dev": dev, "order": order,
            "fits": max(sizes) <= _FP2_GROUP_NODES}
    if not pack["fits"]:
        return pack
    feats = torch.cat([t["feature"].to(dev, torch.int32) for t in trees])
    thrs = torch.cat([t["threshold"].to(dev, torch.float32) for t in trees])
    lefts = torch.cat([t["left_child"].to(dev, torch.int32) for t in trees])
    leaves = torch.cat([t["leaf_value"].to(dev, torch.float32) for t in trees])
    w = torch.as_tensor(weights, dtype=torch.float32)[order].to(dev)
    tree_id = torch.repeat_interleave(
        torch.arange(T, device=dev), torch.tensor(sizes, device=dev))
    payload = torch.where(feats < 0, w[tree_id] * leaves[:, 0], thrs)
    offsets = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0)
    pack.update(
        feats=feats, lefts=lefts, f_max=int(feats.max()),
        offsets32=offsets.to(torch.int32).to(dev),
        planes_t=torch.tensor([planes[i] for i in order], dtype=torch.int32,
                              device=dev),
        node64=(
            (feats.to(torch.int64) & 0xFFFF)
            | ((lefts.to(torch.int64) & 0xFFFF) << 16)
            | ((payload.view(torch.int32).to(torch.int64) & 0xFFFFFFFF) << 32)
        ).contiguous())

    # greedy contiguous tree groups under the LDS node budget
    groups, off_list = [], offsets.tolist()
    first = acc = 0
    for t in range(T):
        if acc + sizes[t] > _FP2_GROUP_NODES and acc > 0:
            groups.append([first, t - first, off_list[first], acc])
            first, acc = t, 0
        acc += sizes[t]
    groups.append([first, T - first, off_list[first], acc])
    pack.update(
        groups_t=torch.tensor(groups, dtype=torch.int32, device=dev),
        max_nodes=max(g[3] for g in groups))
    _pack_forest_binned(pack, feats, thrs, payload)
    return pack


def forest_margin(x, trees, weights, planes, num_planes, cache=None,
                  native_only=False):
    """Margins ``[N, num_planes]`` f32 of a forest of scalar-leaf trees: tree
    t adds ``weights[t] * leaf`` to column ``planes[t]``, the trees of a
    plane in the order given.  A K-class GBM is ``stages * K`` such trees
    with ``planes[t] = t % K``.  A plane without trees is legal and stays 0.

    The native pass (csrc/forest_margin.hip) walks all planes in ONE launch
    over ONE plane-major pack: CUDA f32 rows, ``N >= 1``, ``num_planes >= 2``,
    every tree within ``_FP2_GROUP_NODES`` and ``1 <= F < 32768``.  Anything
    else returns the per-plane composition of ``forest_predict`` (or None
    under ``native_only``); ``SEA_MARGIN_FUSED=0`` forces that route.  Every
    element is an f32 sum in the given order: reproducible bit for bit.  Rows
    are read as u8 ranks whenever the pack has them, else as f32
    (``forest_vote``'s rule); ``SEA_MARGIN_MODE=raw|binned`` overrides.  Both
    are exact.

    ``cache``: caller-owned dict; the pack is kept under "margin_pack", a
    key no other forest op reads (the declined route keeps its per-plane
    packs under "plane_caches")."""
    if not trees:
        raise ValueError("forest_margin needs at least one tree")
    N, F = x.shape
    T = len(trees)
    P = int(num_planes)
    planes = [int(p) for p in planes]
    if len(planes) != T or len(weights) != T:
        raise ValueError(
            f"{T} trees need {T} weights and planes, got {len(weights)} "
            f"and {len(planes)}")
    if min(planes) < 0 or max(planes) >= P:
        raise ValueError(f"planes must lie in [0, {P})")
    if any(t["leaf_value"].shape[1] != 1 for t in trees):
        raise ValueError("forest_margin needs scalar-leaf trees")
    native = (x.is_cuda and x.dtype == torch.float32 and N >= 1 and P >= 2
              and 1 <= F < 32768
              and os.environ.get("SEA_MARGIN_FUSED") != "0")
    m = _require_hip("forest_margin") if native else None
    if m is not None:
        pack = cache.get("margin_pack") if cache is not None else None
        if pack is None or pack["T"] != T or pack["dev"] != x.device:
            pack = _pack_forest_margin(trees, weights, planes, x.device)
            if cache is not None:
                cache["margin_pack"] = pack
        if pack["fits"]:
            if pack["f_max"] >= F:
                raise ValueError(
                    f"forest splits on feature {pack['f_max']} but x has "
                    f"{F} columns")
            binned_avail = bool(
                pack.get("binned_ok") and pack["bin_fmax"] <= F)
            env_mode = os.environ.get("SEA_MARGIN_MODE")
            mode = "raw"
            if binned_avail and env_mode != "raw":
                mode = "binned"
            elif env_mode == "binned":
                raise ValueError(
                    "SEA_MARGIN_MODE=binned: this forest has no u8 rank form "
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
            # the kernel stores a plane when it leaves it: one that no tree
            # names is never stored
            alloc = torch.empty if len(set(planes)) == P else torch.zeros
            out = alloc(N, P, dtype=torch.float32, device=x.device)
            groups = pack["groups_t"]
            m.forest_margin(out, xc, nodes, pack["offsets32"],
                            pack["planes_t"], groups, P,
                            int(pack["max_nodes"]))
            last_forest_margin_info.update(
                path="native", mode=mode,
                rows_per_lane=forest_margin_geometry()["rows_per_lane"],
                groups=int(groups.shape[0]), planes=P)
            return out
    last_forest_margin_info.update(path="reference", mode=None,
                                   rows_per_lane=0, groups=0, planes=P)
    if native_only:
        return None
    if not x.is_cuda:
        return reference.forest_margin(x, trees, weights, planes, P)
    w = torch.as_tensor(weights, dtype=torch.float32)
    caches = cache.setdefault("plane_caches", {}) if cache is not None else {}
    out = torch.zeros(N, P, dtype=torch.float32, device=x.device)
    for j in range(P):
        idx = [t for t in range(T) if planes[t] == j]
        if idx:
            out[:, j] = forest_predict(
                x, [trees[t] for t in idx], w[idx],
                cache=caches.setdefault(j, {}))[:, 0]
    return out


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


# ---- weighted quantiles of member values (csrc/forest_wquantile.hip) -------

WQUANTILE_MAX_MEMBERS = 256   # the member index is the low byte of a key
WQUANTILE_MAX_PROBS = 16
WQUANTILE_MAX_LEAF_VALUES = 1 << 24  # the value rank is the other 24 bits

# what the last forest_wquantile call did: {"path": "native" | "reference",
# "mode": "binned" | "raw" | None, "rows_per_block": R, "groups": G}
last_forest_wquantile_info: dict = {}


def forest_wquantile_geometry():
    """Launch shape of the native ``forest_wquantile``: ``rows`` is
    ``((member limit, rows per block), ...)`` in ascending member limit (the
    padded member count picks the first limit it fits), ``max_blocks`` the
    row-tile grid cap, ``slab_bytes`` the LDS share of the keys and
    ``group_nodes`` the node budget of one LDS group."""
    g = [int(v) for v in
         _require_hip("forest_wquantile").forest_wquantile_geometry()]
    return {"rows": ((g[1], g[0]), (g[3], g[2]), (g[5], g[4])),
            "max_blocks": g[6], "slab_bytes": g[7], "group_nodes": g[8]}


def _wquantile_ranks(pack):
    """Leaf-rank arenas of a unit-weight D == 1 v2 ``pack``, cached on it:
    ``leaf_table`` [U] f32, the sorted distinct leaf values of the whole
    forest (-0.0 and +0.0 are one value), and ``node64r`` / ``node64rb``,
    copies of ``node64`` / ``node64b`` whose LEAF payload is the rank of
    the leaf's value in that table (inner nodes unchanged), as
    ``_pack_forest_binned`` puts threshold ranks into inner payloads.  None
    when a leaf is NaN (a NaN has no rank) or U exceeds 24 bits."""
    if "wq_ranks" not in pack:
        leaf = pack["feats"] < 0
        vals = pack["leaves"][leaf, 0] + 0.0  # -0.0 + 0.0 = +0.0
        ranks = None
        if not bool(torch.isnan(vals).any()):
            table, inv = torch.unique(vals, return_inverse=True)
            if table.numel() <= WQUANTILE_MAX_LEAF_VALUES:
                rank_full = torch.zeros_like(pack["node64"])
                rank_full[leaf] = inv

                def with_ranks(arena):
                    return torch.where(
                        leaf, (arena & 0xFFFFFFFF) | (rank_full << 32),
                        arena).contiguous()

                ranks = {"leaf_table": table.contiguous(),
                         "node64r": with_ranks(pack["node64"])}
                if pack.get("binned_ok"):
                    ranks["node64rb"] = with_ranks(pack["node64b"])
        pack["wq_ranks"] = ranks
    return pack["wq_ranks"]


def _wquantile_qtab(weights, probs):
    """Exact integer form of the rule ``cum >= p * total``: the f32 member
    weights scaled by one power of two into integers q_t, and per
    probability the threshold ``ceil(p * sum q_t)`` from exact rationals, so
    ``cum_q >= threshold`` decides what the real numbers decide.  Returns the
    ``M + Q`` integers, or None when a weight is not finite or the scaled
    sums could leave 62 bits."""
    from fractions import Fraction

    w32 = torch.as_tensor(weights, dtype=torch.float32).reshape(-1)
    if not bool(torch.isfinite(w32).all()):
        return None
    fr = [Fraction(v) for v in w32.tolist()]
    den = max(f.denominator for f in fr)  # denominators are powers of two
    q = [int(f * den) for f in fr]
    if len(q) * max(abs(v) for v in q) >= 1 << 62:
        return None
    total = sum(q)
    # ceil(a / b) == -((-a) // b) for b > 0
    thr = []
    for p in probs:
        t = Fraction(p) * total
        thr.append(-((-t.numerator) // t.denominator))
    return q + thr


def forest_wquantile(x, trees, weights, probs, cache=None,
                     native_only=False):
    """Per-row weighted quantiles over the member values of a forest of
    scalar-leaf trees: ``[N, Q]`` f32 on the device of x, ``out[i, q]`` the
    first of the M values ``leaf_t(x_i)``, in ascending order, whose
    cumulative member weight reaches ``probs[q]`` times the total weight
    (the smallest value when none does); semantics in
    ``reference.forest_wquantile``.  ``weights`` are read as f32.

    On the GPU one launch (csrc/forest_wquantile.hip) walks the forest,
    orders each row's member values on chip and selects in exact integer
    arithmetic.  It serves f32 rows, ``1 <= M <= 256`` trees with ``D == 1``
    that pack as v2 with every tree within the op's LDS group budget
    (``forest_wquantile_geometry``), no NaN leaf, at most 2^24 distinct leaf
    values, ``1 <= Q <= 16`` and weights that scale to integers within 62
    bits; anything else runs the torch reference op on the same device.
    Rows are read as u8 ranks (``bin_features`` against the pack's threshold
    sets, as ``forest_predict2``) whenever the pack has them, else as f32;
    ``SEA_WQUANTILE_MODE=raw|binned`` overrides.  Both are exact.
    ``native_only``: return None where the reference op would run, for a
    caller that has a route of its own for those cases.

    The kernel decides ``cum >= p * total`` in exact arithmetic, the
    reference op in float64 with ``p * total`` rounded.  They agree whenever
    the float64 sums and that product are exact (weights and p with few
    significant bits, as in every test); otherwise they can differ on a row
    whose cumulative weight lies within a float64 rounding of the
    threshold.

    ``cache``: caller-owned dict; the pack (tree weights all 1.0) is built
    once per (forest, device) and kept under "pack".  Keep a dict of its own
    for this op, for the reason ``forest_oob`` gives.
    """
    if not trees:
        raise ValueError("forest_wquantile needs at least one tree")
    probs = [float(p) for p in probs]
    if not all(0.0 <= p <= 1.0 for p in probs):
        raise ValueError(f"probabilities must lie in [0, 1], got {probs}")
    N, F = x.shape
    M, Q = len(trees), len(probs)
    w32 = torch.as_tensor(weights, dtype=torch.float32).reshape(-1)
    if w32.numel() != M:
        raise ValueError(f"{w32.numel()} weights for {M} trees")

    def check_features(f_max):
        if f_max >= F:
            raise ValueError(
                f"forest splits on feature {f_max} but x has {F} columns")

    # N == 0 launches nothing and packs nothing
    native = (x.is_cuda and x.dtype == torch.float32 and 1 <= F < 32768
              and N >= 1
              and 1 <= M <= WQUANTILE_MAX_MEMBERS
              and 1 <= Q <= WQUANTILE_MAX_PROBS
              and all(t["leaf_value"].shape[1] == 1 for t in trees))
    qtab = _wquantile_qtab(w32, probs) if native else None
    m = _require_hip("forest_wquantile") if qtab is not None else None
    if m is not None:
        pack = cache.get("pack") if cache is not None else None
        fits = (pack is not None and pack["T"] == M
                and pack["dev"] == x.device)
        if not (fits and pack.get("unit_weights")):
            pack = _pack_forest(trees, None, x.device)
            pack["unit_weights"] = True
            if cache is not None and not fits:
                cache["pack"] = pack
        if "f_max" not in pack:
            pack["f_max"] = int(pack["feats"].max())
        check_features(pack["f_max"])
        geo = forest_wquantile_geometry()
        grp = _permute_groups(pack, geo["group_nodes"]) if pack["v2"] else None
        ranks = _wquantile_ranks(pack) if grp is not None else None
        if ranks is not None:
            groups, max_nodes = grp
            binned_avail = bool("node64rb" in ranks and pack["bin_fmax"] <= F)
            env_mode = os.environ.get("SEA_WQUANTILE_MODE")
            mode = "raw"
            if binned_avail and env_mode != "raw":
                mode = "binned"
            elif env_mode == "binned":
                raise ValueError(
                    "SEA_WQUANTILE_MODE=binned: this forest has no u8 rank "
                    "form (a feature with more than 255 thresholds, or no "
                    "split at all)")
            xc = x.contiguous()
            if mode == "binned":
                nodes = ranks["node64rb"]
                xb = torch.empty(xc.shape, dtype=torch.uint8, device=x.device)
                m.bin_features(xb, xc, _binned_edges(pack, F))
                xc = xb
            else:
                nodes = ranks["node64r"]
            m_pad = 1 << (M - 1).bit_length()
            rows = next(r for lim, r in geo["rows"] if m_pad <= lim)
            out = torch.empty(N, Q, dtype=torch.float32, device=x.device)
            m.forest_wquantile(
                out, xc, nodes, pack["offsets32"], groups,
                torch.tensor(qtab, dtype=torch.int64).to(x.device),
                ranks["leaf_table"], int(max_nodes))
            last_forest_wquantile_info.update(
                path="native", mode=mode, rows_per_block=rows,
                groups=int(groups.shape[0]))
            return out
    last_forest_wquantile_info.update(
        path="reference", mode=None, rows_per_block=0, groups=0)
    if native_only:
        return None
    check_features(max(int(t["feature"].max()) for t in trees))
    if N == 0:
        return torch.empty(0, Q, dtype=torch.float32, device=x.device)
    return reference.forest_wquantile(x, trees, w32, probs)


last_logreg_info: dict = {}


def logreg_loss_grad(x, y_int, w, wmat, has_bias, native_only=False):
    """Single-pass fused logistic loss+gradient.

    Returns payload [1 + (F+1)*K]: [loss_sum, grad(F,K) flat, grad_bias(K)]
    (unnormalized sums; caller all-reduces and divides by total weight).
    On GPU uses the hand-written gfx950 kernels: the narrow vector kernel
    (csrc/linear.hip) where the (F, K) shape fits its register budget, else
    the MFMA kernel (csrc/linear_wide.hip) for K <= 32 and F <= 1024, else
    the torch fallback.  Where both kernels take the shape and F > 512 the
    MFMA kernel runs: at 768 and 1024 features it measured 1.6x to 3.1x
    faster than the narrow one for K = 2..5 (profiles/logreg_wide.md) and it
    is bitwise reproducible, which the narrow kernel's f32 atomics are not.

    Every call records what ran in ``last_logreg_info``: ``path`` is
    "narrow", "wide" or "reference", and the six values of
    ``logreg_wide_geometry`` follow (all 0 unless the path is "wide").

    ``native_only``: return None where the torch fallback would run.
    """
    f = x.shape[1]
    k = wmat.shape[1]
    geometry = (0, 0, 0, 0, 0, 0)
    if x.is_cuda:
        m = _require_hip("logreg_loss_grad")
        if m is not None:
            wide = x.shape[0] > 0 and m.logreg_wide_supported(f, k)
            if m.logreg_fused_supported(f, k) and not (wide and f > 512):
                payload = torch.zeros(
                    1 + (f + 1) * k, dtype=torch.float32, device=x.device
                )
                kernel, path = m.logreg_loss_grad, "narrow"
            elif wide:
                # every entry is written by the slot reduction
                payload = torch.empty(
                    1 + (f + 1) * k, dtype=torch.float32, device=x.device
                )
                kernel, path = m.logreg_loss_grad_wide, "wide"
                geometry = m.logreg_wide_geometry(f, k)
            else:
                kernel = None
            if kernel is not None:
                kernel(
                    payload, x.contiguous(), y_int.contiguous(),
                    w.contiguous(), wmat.contiguous(), bool(has_bias),
                )
                _set_logreg_info(path, geometry)
                return payload
    _set_logreg_info("reference", geometry)
    if native_only:
        return None
    return reference.logreg_loss_grad(x, y_int, w, wmat, has_bias)


def _set_logreg_info(path, geometry):
    kp, s, rows, lds, nt, db = geometry
    last_logreg_info.update(
        path=path, kp=kp, slices=s, rows_per_tile=rows, lds_bytes=lds,
        nt=nt, db=db)


last_weighted_gram_info: dict = {}


def weighted_gram(x, y, w, native_only=False):
    """Augmented weighted Gram matrix ``G = sum_i w_i z_i z_i^T``,
    ``z_i = [x_i, 1, y_i]``, ``[F+2, F+2]``: ``G[:F+1, :F+1]`` is
    ``X_a^T W X_a`` and ``G[:F+1, F+1]`` is ``X_a^T W y``.

    On GPU, for f32 inputs with ``F + 2 <= 1024`` and at least one row, the
    MFMA kernel (csrc/linear_gram.hip) runs: one pass over x, f64 result,
    exactly symmetric and bitwise reproducible.  Every supported shape takes
    it; the measured times against the two-GEMM path it replaces are in
    profiles/linear_gram.md.  Otherwise reference.weighted_gram runs in the
    dtype of the inputs.

    ``native_only``: return None where the reference would run.
    """
    f = x.shape[1]
    if x.is_cuda and x.dtype == torch.float32:
        m = _require_hip("weighted_gram")
        if m is not None and x.shape[0] > 0 and m.linear_gram_supported(f):
            g = torch.empty(f + 2, f + 2, dtype=torch.float64, device=x.device)
            m.linear_gram(g, x.contiguous(), y.float().contiguous(),
                          w.float().contiguous())
            tiles, panels, rows, lds, flush, _ = m.linear_gram_geometry(f)
            last_weighted_gram_info.update(
                path="native", tiles=tiles, panels=panels, rows_per_tile=rows,
                lds_bytes=lds, flush_rows=flush)
            return g
    last_weighted_gram_info.update(
        path="reference", tiles=0, panels=0, rows_per_tile=0, lds_bytes=0,
        flush_rows=0)
    if native_only:
        return None
    return reference.weighted_gram(x, y, w)
