"""Helpers shared by tests/test_serving_pack.py and test_serving_gpu.py:
random unbalanced forests with integer leaves, rows that sit on (and right
next to) every threshold, a float64 oracle walk, and a pure-torch CPU
emulation of the packed LDS walk (``forest_predict2_kernel``) that reads
the host-side pack exactly the way the kernel does.

Exactness: leaves are integers in [-64, 64], tree weights come from
{0.5, 1, 2} and T <= 64, so every partial sum is an exact f32 whatever
the accumulation order, and for D == 1 the packed payload ``w * leaf`` is
exact too.  Every comparison built on these helpers is ``torch.equal``.
"""

import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.frame import TensorFrame
from spark_ensemble_amd.ops import dispatch, reference

INT_POOL = torch.arange(-4, 5, dtype=torch.float32)
SPECIALS_POOL = torch.tensor(
    [float("-inf"), -3e38, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, 3.4e38,
     float("inf")], dtype=torch.float32)
WEIGHT_SET = torch.tensor([0.5, 1.0, 2.0])

_SPECIAL_X = (0.0, -0.0, 1e-45, -1e-45, 3.3e38, -3.3e38, float("inf"),
              float("-inf"), float("nan"))


def _int_leaves(n, D, gen):
    return torch.randint(-64, 65, (n, D), generator=gen).float()


def rand_tree(depth, F, D, gen, thr_pool, p_stop=0.0):
    """Random tree in the project's node layout, grown level by level:
    a node at level < ``depth`` (the root always, when depth > 0) splits
    unless a ``p_stop`` draw stops it; children are allocated in pairs,
    right = left + 1.  Thresholds are drawn from ``thr_pool``, leaves are
    integers in [-64, 64].  ``p_stop = 0`` gives a complete tree."""
    pool = torch.as_tensor(thr_pool, dtype=torch.float32)
    feat, thr, left = [-1], [0.0], [-1]
    frontier = [0]
    for d in range(depth):
        if not frontier:
            break
        k = len(frontier)
        stop = torch.rand(k, generator=gen) < p_stop
        if d == 0:
            stop[:] = False
        fs = torch.randint(0, F, (k,), generator=gen).tolist()
        ts = pool[torch.randint(0, pool.numel(), (k,), generator=gen)].tolist()
        nxt = []
        for j, nid in enumerate(frontier):
            if bool(stop[j]):
                continue
            l = len(feat)
            feat.extend([-1, -1]); thr.extend([0.0, 0.0]); left.extend([-1, -1])
            feat[nid], thr[nid], left[nid] = fs[j], ts[j], l
            nxt.extend([l, l + 1])
        frontier = nxt
    n = len(feat)
    feature = torch.tensor(feat, dtype=torch.int32)
    leaf = _int_leaves(n, D, gen)
    leaf[feature >= 0] = 0.0
    return {"feature": feature,
            "threshold": torch.tensor(thr, dtype=torch.float32),
            "left_child": torch.tensor(left, dtype=torch.int32),
            "leaf_value": leaf}


def sized_tree(n_nodes, F, D, gen, thr_pool):
    """Heap-shaped tree with EXACTLY ``n_nodes`` (odd) nodes: nodes
    0 .. (n-1)/2 - 1 split, left = 2i + 1."""
    assert n_nodes % 2 == 1
    pool = torch.as_tensor(thr_pool, dtype=torch.float32)
    k = (n_nodes - 1) // 2
    feature = torch.full((n_nodes,), -1, dtype=torch.int32)
    feature[:k] = torch.randint(0, F, (k,), generator=gen).int()
    thr = torch.zeros(n_nodes)
    thr[:k] = pool[torch.randint(0, pool.numel(), (k,), generator=gen)]
    left = torch.full((n_nodes,), -1, dtype=torch.int32)
    left[:k] = 2 * torch.arange(k, dtype=torch.int32) + 1
    leaf = _int_leaves(n_nodes, D, gen)
    leaf[:k] = 0.0
    return {"feature": feature, "threshold": thr, "left_child": left,
            "leaf_value": leaf}


def complete_tree(depth, F, D, gen, thr_pool):
    return sized_tree(2 ** (depth + 1) - 1, F, D, gen, thr_pool)


def leaf_tree(D=1, value=7.0):
    """A root-only tree."""
    return {"feature": torch.tensor([-1], dtype=torch.int32),
            "threshold": torch.zeros(1),
            "left_child": torch.tensor([-1], dtype=torch.int32),
            "leaf_value": torch.full((1, D), float(value))}


def rand_weights(T, gen):
    return WEIGHT_SET[torch.randint(0, 3, (T,), generator=gen)]


def special_candidates(F, pool):
    """[F, C] candidate cell values per feature; ``pool`` is [k] (shared)
    or [F, k] (per feature): every pool value (a tie with a threshold),
    the two floats adjacent to it, a value between each two neighbouring
    pool entries, values below the min and above the max, and +-0.0,
    +-1e-45, +-3.3e38, +-inf, NaN."""
    pool = torch.as_tensor(pool, dtype=torch.float32)
    if pool.dim() == 1:
        pool = pool.unsqueeze(0).expand(F, -1)
    assert pool.shape[0] == F
    big = torch.tensor(float("inf"))
    srt = pool.sort(dim=1).values
    mids = srt[:, :-1] / 2 + srt[:, 1:] / 2
    finite = torch.where(torch.isfinite(pool), pool, torch.zeros(()))
    lo = finite.min(dim=1, keepdim=True).values
    hi = finite.max(dim=1, keepdim=True).values
    return torch.cat(
        [pool, torch.nextafter(pool, big), torch.nextafter(pool, -big), mids,
         lo - 1.0, lo * 2 - 1.0, hi + 1.0, hi * 2 + 1.0,
         torch.tensor(_SPECIAL_X).expand(F, -1)], dim=1).contiguous()


def special_x(n, F, pool, gen):
    """[n, F] f32 rows for exact routing tests, each cell drawn from
    ``special_candidates``.  The first rows cycle through all candidates
    so each one occurs when n allows it."""
    cand = special_candidates(F, pool)
    C = cand.shape[1]
    idx = torch.randint(0, C, (n, F), generator=gen)
    m = min(n, C)
    idx[:m] = (torch.arange(m)[:, None] + torch.arange(F)[None, :]) % C
    return cand.gather(1, idx.T.contiguous()).T.contiguous()


def to_dev(trees, dev):
    return [{k: v.to(dev) for k, v in t.items()} for t in trees]


def oracle(x, trees, weights=None):
    """float64 level-synchronous walk on the CPU: [N, D] float64."""
    t64 = [{"feature": t["feature"].cpu(),
            "threshold": t["threshold"].cpu().double(),
            "left_child": t["left_child"].cpu(),
            "leaf_value": t["leaf_value"].cpu().double()} for t in trees]
    w64 = None if weights is None else weights.cpu().double()
    return reference.forest_predict(x.cpu().double(), t64, w64)


def id_tree(tree):
    """Copy of ``tree`` whose leaf value is the node's own index."""
    n = tree["feature"].numel()
    out = dict(tree)
    out["leaf_value"] = torch.arange(
        n, dtype=torch.float32, device=tree["feature"].device)[:, None]
    return out


def _s16(v):
    return ((v & 0xFFFF) ^ 0x8000) - 0x8000


def lower_bound_bins(x, edges):
    """bin_features_kernel's search, lane by lane: first index with
    ``e[idx] >= v`` by bisection over [0, nedges).  Written out as the
    explicit loop (not a library searchsorted) so an unsorted edge row
    misbehaves here exactly as it does in the kernel."""
    n, F = x.shape
    nedges = edges.shape[1]
    fcol = torch.arange(F)[None, :].expand(n, F)
    lo = torch.zeros(n, F, dtype=torch.long)
    hi = torch.full((n, F), nedges, dtype=torch.long)
    while True:
        active = lo < hi
        if not bool(active.any()):
            break
        mid = (lo + hi) >> 1
        e = edges[fcol, mid.clamp(max=nedges - 1)]
        ge = e >= x
        hi = torch.where(active & ge, mid, hi)
        lo = torch.where(active & ~ge, mid + 1, lo)
    assert int(lo.max()) <= 255
    return lo.to(torch.uint8)


def emulate_packed_walk(x, pack, binned):
    """CPU emulation of ``forest_predict2_kernel`` over a CPU pack from
    ``dispatch._pack_forest``: decodes node64 / node64b (s16 feature, s16
    left, high-32 payload), stages one group at a time the way a block
    fills LDS, and walks each tree with indices RELATIVE to the group.
    ``binned`` rows are first rank-transformed against ``_binned_edges``
    with the kernel's own lower-bound loop.  Returns [N, D] float64."""
    assert pack["v2"]
    x = x.float()
    N, F = x.shape
    D = pack["D"]
    nodes = pack["node64b"] if binned else pack["node64"]
    if binned:
        assert pack.get("binned_ok") and pack["bin_fmax"] <= F
        xb = lower_bound_bins(x, dispatch._binned_edges(pack, F)).long()
    out = torch.zeros(N, D, dtype=torch.float64)
    offsets = pack["offsets32"].long()
    rows = torch.arange(N)
    for first_tree, n_trees, node_base, n_nodes in pack["groups_t"].tolist():
        tlds = nodes[node_base:node_base + n_nodes]
        assert tlds.numel() == n_nodes
        for t in range(first_tree, first_tree + n_trees):
            toff = int(offsets[t]) - node_base
            node = torch.full((N,), toff, dtype=torch.long)
            while True:
                assert int(node.min()) >= 0 and int(node.max()) < n_nodes
                nd = tlds[node]
                f = _s16(nd)
                inner = f >= 0
                if not bool(inner.any()):
                    break
                left = _s16(nd >> 16)
                hi32 = (nd >> 32) & 0xFFFFFFFF
                fc = f.clamp(min=0)
                if binned:
                    go_left = xb[rows, fc] <= hi32
                else:
                    go_left = x[rows, fc] <= _bits_to_f32(hi32)
                node = torch.where(inner, toff + left + (~go_left).long(), node)
            if D == 1:
                out[:, 0] += _bits_to_f32((nd >> 32) & 0xFFFFFFFF).double()
            else:
                lv = pack["leaves"][node_base + node].double()
                out += float(pack["w"][t]) * lv
    return out


def _bits_to_f32(u32_as_i64):
    """Low 32 bits of an int64 tensor reinterpreted as f32."""
    v = u32_as_i64 & 0xFFFFFFFF
    v = torch.where(v >= 2 ** 31, v - 2 ** 32, v)
    return v.to(torch.int32).view(torch.float32)


def check_groups(pack, trees):
    """Group-plan invariants the kernel relies on; returns the group rows
    ``[first_tree, n_trees, node_base, n_nodes]``."""
    sizes = [t["feature"].numel() for t in trees]
    groups = pack["groups_t"].tolist()
    offs = pack["offsets32"].tolist()
    nxt = 0
    for first, cnt, base, n_nodes in groups:
        assert first == nxt and cnt >= 1
        assert base == offs[first]
        assert n_nodes == sum(sizes[first:first + cnt])
        assert n_nodes <= dispatch._FP2_GROUP_NODES
        nxt = first + cnt
    assert nxt == len(trees)
    assert pack["max_nodes"] == max(g[3] for g in groups)
    return groups


def exact_fill_forest(F, D, g, pool, tail):
    """19 complete depth-9 trees (19437 nodes) + one 915-node tree fill
    the LDS group budget exactly; ``tail`` further depth-4 trees."""
    trees = [complete_tree(9, F, D, g, pool) for _ in range(19)]
    trees.append(sized_tree(dispatch._FP2_GROUP_NODES - 19 * 1023, F, D, g, pool))
    trees += [rand_tree(4, F, D, g, pool, p_stop=0.2) for _ in range(tail)]
    return trees


# ---- a row goes the same way in training (bin <= t) and in serving --------

ROUTING_DATASETS = ("ties", "nan", "inf", "nan_inf", "nan_heavy")


def routing_dataset(kind, dev="cpu"):
    """N = 4000, F = 6 integer features in 0..9, y from two of them.
    Column 0 carries 20 % NaN and / or 20 % +inf; in ``nan_inf`` the
    labels of the NaN rows are shifted so that the "is not NaN" split
    (threshold +inf) is worth taking.  ``nan_heavy`` has 40 % NaN in
    column 0, enough for the sorted column's NaNs to reach the cut points
    the bin search probes first, and labels that lean on that column."""
    g = torch.Generator().manual_seed(31)
    n, F = 4000, 6
    x = torch.randint(0, 10, (n, F), generator=g).float()
    y = 3.0 * x[:, 1] - 2.0 * x[:, 2] + (x[:, 0] > 4).float()
    u = torch.rand(n, generator=g)
    if kind in ("nan", "nan_inf"):
        x[u < 0.2, 0] = float("nan")
    if kind in ("inf", "nan_inf"):
        x[(u >= 0.2) & (u < 0.4), 0] = float("inf")
    if kind == "nan_inf":
        y = y + 100.0 * (u < 0.2).float()
    if kind == "nan_heavy":
        y = y + 5.0 * x[:, 0]
        x[u < 0.4, 0] = float("nan")
    return TensorFrame(features=x.to(dev), label=y.to(dev))


def fit_routing_tree(kind, dev="cpu"):
    df = routing_dataset(kind, dev)
    m = sea.DecisionTreeRegressor().setMaxDepth(5).setMaxBins(16).fit(df)
    tree = {k: v.cpu() for k, v in m._tree.items()}
    return df["features"], tree


def check_routing(ids, x, tree, label):
    """``ids`` [N] are the served leaf ids of the TRAINING rows: per-leaf
    row counts must equal the cover the grower recorded, and every id
    must equal the float64 oracle walk."""
    idt = id_tree(tree)
    ids = ids.cpu().double()
    n_nodes = tree["feature"].numel()
    leaves = tree["feature"] < 0
    assert bool((ids == ids.round()).all())
    counts = torch.bincount(ids.long(), minlength=n_nodes)
    assert bool((counts[~leaves] == 0).all()), label
    want = tree["node_weight"].double()
    assert torch.equal(counts[leaves].double(), want[leaves]), \
        (label, counts[leaves], want[leaves])
    assert torch.equal(ids, oracle(x, [idt])[:, 0]), label


def check_bin_split_invariant(x, edges, bins):
    """The train / serve contract at the level of one split: for every
    feature f, cut t and row,  bins[:, f] <= t  <=>  x[:, f] <= edges[f, t]
    (a NaN x is on the right of every cut)."""
    x, edges, bins = x.cpu(), edges.cpu(), bins.cpu().long()
    assert not bool(edges.isnan().any())
    assert bool((edges[:, 1:] >= edges[:, :-1]).all())
    t = torch.arange(edges.shape[1])
    train = bins[:, :, None] <= t[None, None, :]
    serve = x[:, :, None] <= edges[None, :, :]
    assert torch.equal(train, serve)


def nan_columns(gen, n=3000):
    """[n, 4] integer columns 0..9 with 0 % / 20 % / 40 % / 70 % NaN and,
    in the last two, 10 % +inf."""
    x = torch.randint(0, 10, (n, 4), generator=gen).float()
    u = torch.rand(n, 4, generator=gen)
    x[u < torch.tensor([0.0, 0.2, 0.4, 0.7])] = float("nan")
    x[u > torch.tensor([2.0, 2.0, 0.9, 0.9])] = float("inf")
    return x
