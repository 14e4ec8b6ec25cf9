"""Pure-torch reference implementations of every compute op.

These define the semantics that the hand-written CDNA4 HIP kernels
(csrc/*.hip) must reproduce; GPU numerics tests compare kernel output
against these at fp32.  On CPU (no GPU available) they ARE the execution
path, which keeps the whole framework runnable for the non-gpu test suite.

Each op cites the reference behavior it implements (SURVEY.md section 2.7
maps ops -> reference call sites).
"""

from __future__ import annotations

from typing import List, Optional, Tuple

import torch


# ---------------------------------------------------------------------------
# Sampling (reference RDD.sample sites: BaggingRegressor.scala:149-150,
# GBMRegressor.scala:357-359, GBMClassifier.scala:329-331)
# ---------------------------------------------------------------------------


def _gen_for(device, seed: int):
    dev = torch.device(device) if device is not None else torch.device("cpu")
    g = torch.Generator(device=dev)
    g.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
    return g, dev


def sample_weights(
    replacement: bool,
    ratio: float,
    n: int,
    seed: int,
    device=None,
    base_weight: Optional[torch.Tensor] = None,
    rank: int = 0,
) -> torch.Tensor:
    """Poisson(ratio) multiplicities (with replacement) or Bernoulli(ratio)
    0/1 mask (without), as an instance-weight vector."""
    g, dev = _gen_for(device, seed * 1_000_003 + rank)
    if ratio >= 1.0 and not replacement:
        w = torch.ones(n, dtype=torch.float32, device=dev)
    elif replacement:
        rate = torch.full((n,), float(ratio), device=dev)
        w = torch.poisson(rate, generator=g)
    else:
        w = (torch.rand(n, generator=g, device=dev) < ratio).float()
    if base_weight is not None:
        w = w * base_weight
    return w


# ---------------------------------------------------------------------------
# Quantile binning (the columnar-frame equivalent of MLlib's tree binning;
# also backs approxQuantile uses: DummyRegressor.scala:120-124,
# GBMRegressor.scala:306,347-351)
# ---------------------------------------------------------------------------


def quantile_bins(
    x: torch.Tensor, max_bins: int = 256, sample_rows: int = 262_144, seed: int = 17
) -> torch.Tensor:
    """Per-feature quantile cut points.

    x: [N, F] f32 -> edges [F, max_bins-1] f32; bin b covers
    (edges[b-1], edges[b]].  Built from a row sample (cap ``sample_rows``)
    like MLlib's ``findSplits``; duplicated cut points simply leave empty
    bins.
    """
    n, f = x.shape
    if n > sample_rows:
        g, _ = _gen_for(x.device, seed)
        idx = torch.randint(0, n, (sample_rows,), generator=g, device=x.device)
        xs = x.index_select(0, idx)
    else:
        xs = x
    s = xs.shape[0]
    xs_sorted, _ = xs.sort(dim=0)
    # cut at interior quantile positions
    q = torch.arange(1, max_bins, device=x.device, dtype=torch.float32) / max_bins
    pos = (q * (s - 1)).long().clamp_(0, s - 1)
    edges = xs_sorted.index_select(0, pos).T.contiguous()  # [F, B-1]
    # NaNs sort last, so a column with many of them would end its cut
    # points in NaN: the bin search would treat those as below every x
    # (merging real values with the NaN bin) and a split there would get a
    # NaN threshold, which sends every row right when serving.  +inf keeps
    # the row sorted and  bin <= t  <=>  x <= edges[t]  for every x; a NaN
    # x still lands in the last bin.
    return edges.masked_fill_(edges.isnan(), float("inf"))


def bin_features(x: torch.Tensor, edges: torch.Tensor) -> torch.Tensor:
    """Map raw features to bin indices: [N, F] f32 -> [N, F] uint8.

    bin = number of edges strictly below-or-equal x (searchsorted right on
    edges gives index of first edge > x ... we use left: x <= edge -> bin of
    that edge).  Convention: row goes LEFT iff bin <= split_bin.
    """
    # searchsorted wants [F, N]
    xt = x.T.contiguous()
    b = torch.searchsorted(edges.contiguous(), xt, right=False)
    return b.T.contiguous().to(torch.uint8)


# ---------------------------------------------------------------------------
# Histogram build (replaces MLlib DecisionTree's treeAggregate histogram
# rounds invoked via fitBaseLearner, reference ensembleParams.scala:64-81)
# ---------------------------------------------------------------------------


def hist_build(
    bins: torch.Tensor,  # [N, F] uint8
    gh: torch.Tensor,  # [N, C] f32  (C = D grad dims + hess + count-weight)
    row_idx: torch.Tensor,  # [M] int32/int64 rows grouped by node
    node_offsets: torch.Tensor,  # [n_nodes+1] int64 segment bounds in row_idx
    num_bins: int,
) -> torch.Tensor:
    """Per-(node, feature, bin) sums of gh channels.

    Returns [n_nodes, F, num_bins, C] f32.  The HIP kernel stages per-
    feature-group histograms in LDS with atomic adds; this reference uses
    index_add_ per node.
    """
    n_nodes = node_offsets.numel() - 1
    N, F = bins.shape
    C = gh.shape[1]
    out = torch.zeros(n_nodes, F, num_bins, C, dtype=torch.float32, device=bins.device)
    offs = node_offsets.tolist()
    fb = torch.arange(F, device=bins.device, dtype=torch.long) * num_bins
    for nd in range(n_nodes):
        s, e = offs[nd], offs[nd + 1]
        if e <= s:
            continue
        rows = row_idx[s:e].long()
        b = bins.index_select(0, rows).long()  # [m, F]
        flat = (b + fb.unsqueeze(0)).reshape(-1)  # [m*F]
        vals = (
            gh.index_select(0, rows)
            .unsqueeze(1)
            .expand(-1, F, -1)
            .reshape(-1, C)
        )
        out[nd].reshape(F * num_bins, C).index_add_(0, flat, vals)
    return out


def hist_build_forest(bins, gh, row_idx, node_offsets, node_col0, num_bins,
                      c_per_node):
    """Forest-build reference: gh [N, T*C] interleaves per-tree channel
    groups; node nd accumulates columns [col0, col0+C) only."""
    n_nodes = node_offsets.numel() - 1
    N, F = bins.shape
    C = int(c_per_node)
    out = torch.zeros(n_nodes, F, num_bins, C, dtype=torch.float32,
                      device=bins.device)
    offs = node_offsets.tolist()
    col0s = node_col0.tolist()
    fb = torch.arange(F, device=bins.device, dtype=torch.long) * num_bins
    for nd in range(n_nodes):
        s, e = offs[nd], offs[nd + 1]
        if e <= s:
            continue
        c0 = int(col0s[nd])
        rows = row_idx[s:e].long()
        b = bins.index_select(0, rows).long()
        flat = (b + fb.unsqueeze(0)).reshape(-1)
        vals = (
            gh[:, c0:c0 + C].index_select(0, rows)
            .unsqueeze(1)
            .expand(-1, F, -1)
            .reshape(-1, C)
        )
        out[nd].reshape(F * num_bins, C).index_add_(0, flat, vals)
    return out


def hist_build_class(bins, label, weight, row_idx, node_offsets, node_col0,
                     num_bins, num_classes, nn, w_max=None):
    """Label-indexed histograms for K-class gini trees.

    ``label`` [N] u8 in [0, K), ``weight`` [N, T] f32 >= 0; node nd sums
    weight column ``node_col0[nd]`` (its owning tree).  Returns
    [n_nodes, F, num_bins, K + nn] f32 in the grower's layout: channels
    [0, K) per-class weight sums, channel K the hessian (weight sum over all
    classes), channel K + 1 (nn == 2) the row count — what ``hist_build``
    gives for the one-hot x weight gradient matrix, without building it.
    ``w_max`` only sizes the GPU kernel's quantisation; unused here.
    """
    n_nodes = node_offsets.numel() - 1
    N, F = bins.shape
    K = int(num_classes)
    C = K + int(nn)
    dev = bins.device
    out = torch.zeros(n_nodes, F, num_bins, C, dtype=torch.float32, device=dev)
    offs = node_offsets.tolist()
    col0s = node_col0.tolist()
    fb = torch.arange(F, device=dev, dtype=torch.long) * num_bins
    for nd in range(n_nodes):
        s, e = offs[nd], offs[nd + 1]
        if e <= s:
            continue
        rows = row_idx[s:e].long()
        cell = bins.index_select(0, rows).long() + fb.unsqueeze(0)  # [m, F]
        lab = label.index_select(0, rows).long().unsqueeze(1)  # [m, 1]
        w = weight[:, int(col0s[nd])].index_select(0, rows)
        flat = out[nd].reshape(F * num_bins * C)  # view: rows of C channels
        wf = w.unsqueeze(1).expand(-1, F).reshape(-1)
        base = (cell * C).reshape(-1)
        flat.index_add_(0, (cell * C + lab).reshape(-1), wf)
        flat.index_add_(0, base + K, wf)
        if nn == 2:
            flat.index_add_(0, base + K + 1, torch.ones_like(wf))
    return out


# ---------------------------------------------------------------------------
# Split search (vectorized over nodes x features x bins; works on both
# devices as plain tensor algebra — small relative to hist_build)
# ---------------------------------------------------------------------------


def split_search(
    hist: torch.Tensor,  # [n_nodes, F, B, C]
    lam: float = 1e-6,
    min_child_weight: float = 0.0,
    min_instances: float = 1.0,
    min_info_gain: float = 0.0,
    d_dims: int = -1,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Best variance-reduction / newton-gain split per node.

    Gain for child stats (G vec, H): score = |G|^2 / (H + lam); split gain =
    scoreL + scoreR - scoreParent.  With G = sum of one-hot labels and
    H = count this is exactly weighted gini gain x const; with
    G = residual sums, H = hessian sums it is the XGBoost-style newton gain.

    Returns (gain [n], feature [n], bin [n], left_stats [n, C]).
    gain = -inf where no valid split exists.
    """
    n, F, B, C = hist.shape
    D = d_dims if d_dims > 0 else C - 2
    idx_c = C - 1  # count channel; == hess channel when C == D + 1
    total = hist.sum(dim=2)  # [n, F, B, C] -> [n, F, C]
    parent = total[:, 0, :]  # same for every feature: [n, C]
    cum = hist.cumsum(dim=2)  # left stats if split at bin b (x <= edge_b)
    left = cum[:, :, : B - 1, :]  # last bin can't split
    right = total.unsqueeze(2) - left

    def score(stats):
        g = stats[..., :D]
        h = stats[..., D]
        return (g * g).sum(dim=-1) / (h + lam)

    gain = score(left) + score(right) - score(parent)[:, None, None]
    hl = left[..., D]
    hr = right[..., D]
    cl = left[..., idx_c]
    cr = right[..., idx_c]
    valid = (
        (hl >= min_child_weight)
        & (hr >= min_child_weight)
        & (cl >= min_instances)
        & (cr >= min_instances)
    )
    gain = torch.where(valid, gain, torch.full_like(gain, float("-inf")))
    flat = gain.reshape(n, F * (B - 1))
    best = flat.argmax(dim=1)
    best_gain = flat.gather(1, best.unsqueeze(1)).squeeze(1)
    feat = best // (B - 1)
    b = best % (B - 1)
    left_stats = left[torch.arange(n, device=hist.device), feat, b]  # [n, C]
    # apply min_info_gain
    best_gain = torch.where(
        best_gain >= min_info_gain, best_gain, torch.full_like(best_gain, float("-inf"))
    )
    return best_gain, feat, b, left_stats


# ---------------------------------------------------------------------------
# Row partition (tree growth bookkeeping; MLlib keeps a nodeIdCache — we
# keep explicit per-node row-index segments)
# ---------------------------------------------------------------------------


def partition_rows(
    bins: torch.Tensor,  # [N, F] uint8
    row_idx: torch.Tensor,  # [M]
    node_offsets: torch.Tensor,  # [n+1]
    feat: torch.Tensor,  # [n] best feature per node (-1 = leaf, don't split)
    thr: torch.Tensor,  # [n] split bin per node
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Partition each node's rows into (left, right) by bin <= thr.

    Returns (new_row_idx, new_node_offsets [2n+1], left_counts [n]).
    Nodes with feat < 0 keep all rows on the left side (callers drop them
    from the active set before the next level).
    """
    offs = node_offsets.tolist()
    n = len(offs) - 1
    pieces: List[torch.Tensor] = []
    sizes: List[int] = []
    left_counts = []
    for nd in range(n):
        s, e = offs[nd], offs[nd + 1]
        rows = row_idx[s:e]
        f = int(feat[nd])
        if f < 0:
            pieces.append(rows)
            pieces.append(rows[:0])
            left_counts.append(rows.numel())
            sizes.extend([rows.numel(), 0])
            continue
        go_left = bins[rows.long(), f] <= thr[nd]
        l = rows[go_left]
        r = rows[~go_left]
        pieces.extend([l, r])
        left_counts.append(l.numel())
        sizes.extend([l.numel(), r.numel()])
    new_rows = torch.cat(pieces) if pieces else row_idx[:0]
    new_offs = torch.tensor(
        [0] + list(torch.tensor(sizes).cumsum(0).tolist()), dtype=torch.int64
    )
    return new_rows, new_offs, torch.tensor(left_counts, dtype=torch.int64)


# ---------------------------------------------------------------------------
# Tree inference (reference per-row model.predict loops, e.g.
# BaggingRegressor.scala:221-228, GBMClassifier.scala:567-589)
# ---------------------------------------------------------------------------


def tree_predict(
    x: torch.Tensor,  # [N, F] f32 raw features
    feature: torch.Tensor,  # [n_nodes] int32 (-1 leaf)
    threshold: torch.Tensor,  # [n_nodes] f32 (go left iff x <= thr)
    left_child: torch.Tensor,  # [n_nodes] int32 (right = left+1)
    leaf_value: torch.Tensor,  # [n_nodes, D] f32
    max_depth: int,
) -> torch.Tensor:
    """Vectorized level-synchronous walk; returns [N, D]."""
    N = x.shape[0]
    node = torch.zeros(N, dtype=torch.long, device=x.device)
    featl = feature.long()
    leftl = left_child.long()
    for _ in range(max_depth + 1):
        f = featl[node]
        is_leaf = f < 0
        if bool(is_leaf.all()):
            break
        fx = x.gather(1, f.clamp(min=0).unsqueeze(1)).squeeze(1)
        go_left = fx <= threshold[node]
        nxt = leftl[node] + (~go_left).long()
        node = torch.where(is_leaf, node, nxt)
    return leaf_value[node]


def forest_predict(
    x: torch.Tensor,
    trees: List[dict],
    weights: Optional[torch.Tensor] = None,
    max_depth: int = 64,
) -> torch.Tensor:
    """Sum (optionally weighted) of per-tree predictions: [N, D]."""
    out = None
    for i, t in enumerate(trees):
        p = tree_predict(
            x, t["feature"], t["threshold"], t["left_child"], t["leaf_value"], max_depth
        )
        if weights is not None:
            p = p * weights[i]
        out = p if out is None else out + p
    return out


def forest_staged_loss(x, trees, weights, dim, init, label, row_weight, loss):
    """Per-stage loss sums of a boosted forest: ``[S + 1]`` float64.

    ``trees`` holds ``S * dim`` scalar-leaf trees in stage-major order: tree
    t belongs to stage ``t // dim`` and adds ``weights[t] * leaf`` to margin
    column ``t % dim``.  Entry 0 is ``sum_i w_i * loss(label_i, init_i)``
    with ``init`` the ``[N, dim]`` start margins, entry s the same sum after
    the first s stages (sums, not means).  ``label`` is the encoded label
    ``[N, dim]``, ``loss`` a ``GBMLoss``.

    Runs in the dtype of ``x``: margins and the per-row weighted loss are
    in that dtype, the sum over rows is always float64.  ``x.double()``
    gives the float64 oracle, ``x.float()`` the f32 reference.  The result
    is on the device of ``x``."""
    dt = x.dtype
    dim = int(dim)
    if len(trees) % dim:
        raise ValueError(
            f"{len(trees)} trees are not whole stages of {dim} trees")
    margin = init.to(dt).reshape(x.shape[0], dim).clone()
    lab = label.to(dt).reshape(x.shape[0], dim)
    w = row_weight.to(dt)
    out = [(loss.loss(lab, margin) * w).double().sum()]
    for t, tree in enumerate(trees):
        leaf = tree_predict(
            x, *(tree[k].to(x.device) for k in
                 ("feature", "threshold", "left_child", "leaf_value")), 64,
        )[:, 0].to(dt)
        margin[:, t % dim] += leaf * float(weights[t])
        if t % dim == dim - 1:
            out.append((loss.loss(lab, margin) * w).double().sum())
    return torch.stack(out)


def forest_oob(x, trees, inbag):
    """Out-of-bag leaf sums and counts of a bagged forest.

    ``x`` is ``[N, F]``, ``trees`` T tree dicts with D-wide leaves, ``inbag``
    ``[N, T]`` bool, True where row i was in tree t's bag::

        sums[i, :] = sum over t with not inbag[i, t], t = 0 .. T-1 in order,
                     of leaf_t(x_i)                              [N, D]
        counts[i]  = number of t with not inbag[i, t]            int32 [N]

    There are no tree weights.  Routing is serving's (``x <= thr`` goes
    left, a NaN goes right).  A row that is in every bag gets ``sums = 0,
    counts = 0``.

    Runs in the dtype of ``x``: ``x.double()`` gives the float64 oracle,
    ``x.float()`` the f32 reference.  Both results are on the device of
    ``x``."""
    if not trees:
        raise ValueError("forest_oob needs at least one tree")
    dt = x.dtype
    N = x.shape[0]
    inbag = torch.as_tensor(inbag).to(x.device, torch.bool)
    if inbag.dim() != 2 or tuple(inbag.shape) != (N, len(trees)):
        raise ValueError(
            f"inbag is {tuple(inbag.shape)}, expected ({N}, {len(trees)})")
    D = trees[0]["leaf_value"].shape[1]
    sums = torch.zeros(N, D, dtype=dt, device=x.device)
    zero = torch.zeros((), dtype=dt, device=x.device)
    for t, tree in enumerate(trees):
        leaf = tree_predict(
            x, *(tree[k].to(x.device) for k in
                 ("feature", "threshold", "left_child", "leaf_value")), 64,
        ).to(dt)
        oob = ~inbag[:, t]
        sums = sums + torch.where(oob[:, None], leaf, zero)
    counts = (~inbag).sum(dim=1).to(torch.int32)
    return sums, counts


def forest_permute_loss(x, trees, weights, init, label, row_weight, loss,
                        donor):
    """Loss sums of a forest with one feature column shuffled at a time:
    ``(base, perm)``, a float64 scalar and a float64 ``[R, F]``.

    ``trees`` are T scalar-leaf trees with tree weights ``weights``,
    ``init`` / ``label`` / ``row_weight`` are ``[N]``, ``loss`` a ``GBMLoss``
    of ``dim == 1`` and ``donor`` ``[R, N]`` row indices, each row a
    permutation of ``0 .. N-1``::

        base       = sum_i w_i * loss(label_i, init_i + sum_t w_t leaf_t(x_i))
        perm[r, f] = the same sum over x with column f replaced by
                     x[donor[r], f]; every other column untouched

    One permutation per repeat is shared by all features.  Routing is
    serving's (``x <= thr`` goes left, a NaN goes right), for a donor's
    value as for the row's own.

    Runs in the dtype of ``x`` (margins and per-row weighted loss), the sum
    over rows is always float64: ``x.double()`` gives the float64 oracle.
    Both results are on the device of ``x``.  Naive on purpose: R * F
    column swaps and full forest walks."""
    dt, dev = x.dtype, x.device
    N, F = x.shape
    donor = torch.as_tensor(donor).to(dev, torch.long)
    if donor.dim() != 2 or donor.shape[1] != N:
        raise ValueError(
            f"donor is {tuple(donor.shape)}, expected (R, {N})")
    R = donor.shape[0]
    if N == 0:
        return (torch.zeros((), dtype=torch.float64, device=dev),
                torch.zeros(R, F, dtype=torch.float64, device=dev))
    if int(donor.min()) < 0 or int(donor.max()) >= N:
        raise ValueError(f"donor holds an index outside [0, {N})")
    tr = [{"feature": t["feature"].to(dev),
           "threshold": t["threshold"].to(dev),
           "left_child": t["left_child"].to(dev),
           "leaf_value": t["leaf_value"].to(dev, dt)} for t in trees]
    tw = torch.as_tensor([float(v) for v in weights], dtype=dt, device=dev)
    ini = init.to(dev, dt).reshape(N)
    lab = label.to(dev, dt).reshape(N, 1)
    w = row_weight.to(dev, dt).reshape(N)

    def loss_sum(xx):
        margin = ini.clone()
        if tr:
            margin = margin + forest_predict(xx, tr, tw)[:, 0].to(dt)
        return (loss.loss(lab, margin.unsqueeze(1)) * w).double().sum()

    base = loss_sum(x)
    perm = torch.empty(R, F, dtype=torch.float64, device=dev)
    for r in range(R):
        for f in range(F):
            xp = x.clone()
            xp[:, f] = x[donor[r], f]
            perm[r, f] = loss_sum(xp)
    return base, perm


def logreg_loss_grad(x, y_int, w, wmat, has_bias):
    """Torch reference for the fused logistic loss+grad payload
    (dispatch.logreg_loss_grad contract)."""
    f = x.shape[1]
    k = wmat.shape[1]
    wm = wmat[:f]
    raw = x @ wm
    if has_bias:
        raw = raw + wmat[f]
    logp = torch.log_softmax(raw, dim=1)
    yl = y_int.long()
    nll = -(logp.gather(1, yl.unsqueeze(1)).squeeze(1) * w).sum()
    p = logp.exp()
    onehot = torch.zeros_like(p)
    onehot.scatter_(1, yl.unsqueeze(1), 1.0)
    gmat = (p - onehot) * w.unsqueeze(1)
    gw = x.T @ gmat
    gb = gmat.sum(dim=0) if has_bias else torch.zeros(k, device=x.device)
    return torch.cat([nll.reshape(1), gw.reshape(-1), gb.reshape(-1)])


# ---------------------------------------------------------------------------
# Per-row feature contributions (path-dependent TreeSHAP; semantics in
# docs/contributions.md)
# ---------------------------------------------------------------------------

CONTRIB_HAS_LO = 1  # element flag bits
CONTRIB_HAS_HI = 2


def _tree_paths(tree: dict):
    """Root-to-leaf paths of one tree with repeated features merged.

    Returns ``[(leaf_id, [(feature, lo, has_lo, hi, has_hi, z), ...]), ...]``
    in left-to-right leaf order: a row satisfies element e iff
    ``lo < x[feature] <= hi`` (each bound only when its flag is set), and z
    is the product of child/parent covers over the merged nodes, in float64.
    """
    if "node_weight" not in tree:
        raise ValueError(
            "tree has no node_weight (per-node covers): it was fitted or "
            "saved before covers were recorded; refit the model to compute "
            "contributions"
        )
    feat = tree["feature"].cpu().tolist()
    thr = tree["threshold"].cpu().double().tolist()
    left = tree["left_child"].cpu().tolist()
    cov = tree["node_weight"].cpu().double().tolist()
    paths = []
    stack = [(0, {})]
    while stack:
        nid, el = stack.pop()
        f = feat[nid]
        if f < 0:
            paths.append((nid, [(k,) + v for k, v in el.items()]))
            continue
        t, c, l = thr[nid], cov[nid], left[nid]
        for child, go_left in ((l + 1, False), (l, True)):  # left pops first
            z = cov[child] / c if c > 0 else 0.0
            lo, has_lo, hi, has_hi, zz = el.get(f, (0.0, False, 0.0, False, 1.0))
            if go_left:
                hi, has_hi = (min(hi, t) if has_hi else t), True
            else:
                lo, has_lo = (max(lo, t) if has_lo else t), True
            e = dict(el)
            e[f] = (lo, has_lo, hi, has_hi, zz * z)
            stack.append((child, e))
    return paths


def contrib_paths(trees: List[dict], weights=None, planes=None,
                  num_planes: int = 1) -> dict:
    """Flat host tables of every path of a weighted forest (float64 values),
    shared by :func:`forest_contrib` and the GPU packer.

    Per path: ``off`` (first element), ``m`` (unique elements), ``plane``,
    ``v`` (leaf value x tree weight).  Per element: ``feat``, ``lo``, ``hi``,
    ``flags`` (CONTRIB_HAS_LO | CONTRIB_HAS_HI), ``z``.  ``bias`` [num_planes]
    is ``sum_leaves v * c_leaf / c_root``; ``bound`` is
    ``sum_t |w_t| max|leaf_t|`` (no cell of the result, and no partial sum of
    its path terms, exceeds twice that when ``covers_additive``: every
    parent's cover equals the sum of its children's to 1e-3 relative, as the
    growers' do).  A tree with D leaf outputs adds
    output d into plane ``planes[t] + d``; its paths are listed once per
    output with a nonzero leaf value and share their elements.  Trees of
    weight 0 and paths of value 0 are left out (they add exactly nothing).
    """
    T = len(trees)
    w_l = [1.0] * T if weights is None else [float(v) for v in weights]
    p_l = [0] * T if planes is None else [int(v) for v in planes]
    assert len(w_l) == T and len(p_l) == T
    p_off, p_m, p_plane, p_v = [], [], [], []
    e_feat, e_lo, e_hi, e_flags, e_z = [], [], [], [], []
    bias = [0.0] * num_planes
    bound, additive = 0.0, True
    for tree, w, pl in zip(trees, w_l, p_l):
        leaf = tree["leaf_value"].cpu().double()
        D = leaf.shape[1]
        if pl < 0 or pl + D > num_planes:
            raise ValueError(
                f"tree with {D} outputs at plane {pl} exceeds num_planes="
                f"{num_planes}"
            )
        paths = _tree_paths(tree)  # validates node_weight even at weight 0
        if w == 0.0:
            continue
        bound += abs(w) * float(leaf.abs().max())
        cov_t = tree["node_weight"].cpu().double()
        split = (tree["feature"].cpu() >= 0).nonzero(as_tuple=True)[0]
        kids = tree["left_child"].cpu().long()[split]
        additive = additive and bool(
            ((cov_t[kids] + cov_t[kids + 1] - cov_t[split]).abs()
             <= 1e-3 * cov_t[split]).all())
        leaf = leaf.tolist()
        cov = cov_t.tolist()
        for leaf_id, elems in paths:
            off = len(e_feat)
            listed = False
            for d in range(D):
                v = leaf[leaf_id][d] * w
                if v == 0.0:
                    continue
                if cov[0] > 0:
                    bias[pl + d] += v * cov[leaf_id] / cov[0]
                if not elems:
                    continue
                if not listed:
                    for f, lo, has_lo, hi, has_hi, z in elems:
                        e_feat.append(f)
                        e_lo.append(lo)
                        e_hi.append(hi)
                        e_flags.append((CONTRIB_HAS_LO if has_lo else 0)
                                       | (CONTRIB_HAS_HI if has_hi else 0))
                        e_z.append(z)
                    listed = True
                p_off.append(off)
                p_m.append(len(elems))
                p_plane.append(pl + d)
                p_v.append(v)
    i64, f64 = torch.int64, torch.float64
    return {
        "off": torch.tensor(p_off, dtype=i64),
        "m": torch.tensor(p_m, dtype=i64),
        "plane": torch.tensor(p_plane, dtype=i64),
        "v": torch.tensor(p_v, dtype=f64),
        "feat": torch.tensor(e_feat, dtype=i64),
        "lo": torch.tensor(e_lo, dtype=f64),
        "hi": torch.tensor(e_hi, dtype=f64),
        "flags": torch.tensor(e_flags, dtype=i64),
        "z": torch.tensor(e_z, dtype=f64),
        "bias": torch.tensor(bias, dtype=f64),
        "bound": bound,
        "covers_additive": additive,
    }


def gauss_legendre_01(n: int):
    """Nodes and weights (float64 tensors) of the n-point Gauss-Legendre
    rule on [0, 1]; exact for polynomials of degree <= 2n - 1."""
    import numpy as np

    xs, ws = np.polynomial.legendre.leggauss(n)
    return torch.from_numpy((xs + 1.0) / 2.0), torch.from_numpy(ws / 2.0)


def forest_contrib(
    x: torch.Tensor,  # [N, F] f32 or f64
    trees: List[dict],
    weights=None,
    planes=None,
    num_planes: int = 1,
    tables: Optional[dict] = None,
) -> torch.Tensor:
    """Per-row additive feature contributions: ``[N, num_planes, F + 1]`` in
    the dtype of ``x`` (float64 in, float64 throughout); column F is the
    bias.  Rows sum to the weighted forest prediction of the plane.

    Evaluates the path form: for a path with m unique elements the
    coefficient sum ``sum_k k!(m-1-k)!/m! [t^k] prod_{j != e}(z_j + o_j t)``
    equals ``integral_0^1 prod_{j != e}(z_j (1 - s) + o_j s) ds``, and the
    integrand has degree m - 1, so Gauss-Legendre with ceil(m / 2) nodes is
    exact.  The product over the other elements is prefix x suffix: nothing
    is divided out and every term is non-negative.  Vectorised over rows and
    over all paths of equal m.  ``tables`` takes a precomputed
    :func:`contrib_paths` result.
    """
    assert x.dim() == 2
    dt = x.dtype if x.dtype == torch.float64 else torch.float32
    x = x.to(dt)
    N, F = x.shape
    dev = x.device
    tb = tables if tables is not None else contrib_paths(
        trees, weights, planes, num_planes)
    out = torch.zeros(N, num_planes, F + 1, dtype=dt, device=dev)
    out[:, :, F] = tb["bias"].to(device=dev, dtype=dt)
    if tb["feat"].numel() and int(tb["feat"].max()) >= F:
        raise ValueError(
            f"forest splits on feature {int(tb['feat'].max())} but x has "
            f"{F} columns"
        )
    flat = out.view(N, num_planes * (F + 1))
    for m in sorted(set(tb["m"].tolist())):
        sel = (tb["m"] == m).nonzero(as_tuple=True)[0]
        q = (m + 1) // 2
        s64, w64 = gauss_legendre_01(q)
        s = s64.to(device=dev, dtype=dt)
        a = (1.0 - s64).to(device=dev, dtype=dt)
        wq = w64.to(device=dev, dtype=dt)
        # chunk so the [N, P, m, q] factor tensor stays modest
        step = max(1, (1 << 22) // max(N * m * q, 1))
        for c0 in range(0, sel.numel(), step):
            ps = sel[c0:c0 + step]
            eidx = tb["off"][ps].unsqueeze(1) + torch.arange(m)  # [P, m]
            feat = tb["feat"][eidx].to(dev)
            flags = tb["flags"][eidx].to(dev)
            lo = tb["lo"][eidx].to(device=dev, dtype=dt)
            hi = tb["hi"][eidx].to(device=dev, dtype=dt)
            z = tb["z"][eidx].to(device=dev, dtype=dt)
            v = tb["v"][ps].to(device=dev, dtype=dt)
            xv = x[:, feat.reshape(-1)].reshape(N, -1, m)
            o = (((flags & CONTRIB_HAS_LO) == 0) | (xv > lo)) & (
                ((flags & CONTRIB_HAS_HI) == 0) | (xv <= hi))
            o = o.to(dt)  # [N, P, m]
            f = (z.unsqueeze(-1) * a).unsqueeze(0) + o.unsqueeze(-1) * s
            one = torch.ones_like(f[:, :, :1])
            pre = torch.cat([one, f[:, :, :-1].cumprod(dim=2)], dim=2)
            suf = torch.cat(
                [f[:, :, 1:].flip(2).cumprod(dim=2).flip(2), one], dim=2)
            S = ((pre * suf) * wq).sum(dim=-1)  # [N, P, m]
            contrib = v.view(1, -1, 1) * (o - z) * S
            col = tb["plane"][ps].to(dev).unsqueeze(1) * (F + 1) + feat
            flat.index_add_(1, col.reshape(-1), contrib.reshape(N, -1))
    return out
