"""The gfx950 forest_contrib kernel against the float64 reference op.

Tolerance, per case:  err <= 4 * e_ref32 + 2^-23 * S  with e_ref32 the max
abs error of the float32 reference op against its float64 run on the same
inputs (both on the CPU) and S = sum_t |w_t| * max|leaf_t| (4x covers the
reordered summation, the floor is one f32 ulp of the output scale).
Measured figures per shape are in profiles/tree_contrib.md."""

import pytest
import torch

from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.ops import reference

pytestmark = pytest.mark.gpu

GRID = (-1.0, -0.5, 0.0, 0.5, 1.0)  # thresholds; x lands on them often


def random_tree(g, nf, depth, leaf_dim=1, p_leaf=0.15):
    """Random tree (children adjacent, integer covers); thresholds on GRID."""
    feat, thr, left, leaf, cov = [], [], [], [], []

    def alloc():
        feat.append(-1); thr.append(0.0); left.append(-1)
        leaf.append([0.0] * leaf_dim); cov.append(0.0)
        return len(feat) - 1

    def fill(nid, d):
        stop = d == depth or (d > 0 and float(torch.rand((), generator=g)) < p_leaf)
        if stop:
            leaf[nid] = torch.randn(leaf_dim, generator=g).tolist()
            cov[nid] = float(torch.randint(1, 10, (), generator=g))
            return cov[nid]
        l = alloc()
        alloc()
        feat[nid] = int(torch.randint(0, nf, (), generator=g))
        thr[nid] = GRID[int(torch.randint(0, len(GRID), (), generator=g))]
        left[nid] = l
        cov[nid] = fill(l, d + 1) + fill(l + 1, d + 1)
        return cov[nid]

    fill(alloc(), 0)
    return _tree(feat, thr, left, leaf, cov)


def chain_tree(g, feats):
    """One split per entry of ``feats``, each on the right child of the one
    before: the deepest path tests every entry."""
    n = len(feats)
    feat, thr, left = [-1] * (2 * n + 1), [0.0] * (2 * n + 1), [-1] * (2 * n + 1)
    leaf = torch.randn(2 * n + 1, 1, generator=g).tolist()
    cov = [float(v) for v in torch.randint(1, 10, (2 * n + 1,), generator=g)]
    for i, f in enumerate(feats):
        feat[2 * i], left[2 * i] = f, 2 * i + 1
        # non-decreasing thresholds keep every repeated feature's merged
        # interval non-empty
        thr[2 * i] = GRID[min(len(GRID) - 1, (i * len(GRID)) // n)]
    for i in reversed(range(n)):
        cov[2 * i] = cov[2 * i + 1] + cov[2 * i + 2]
    return _tree(feat, thr, left, leaf, cov)


def _tree(feat, thr, left, leaf, cov):
    return {
        "feature": torch.tensor(feat, dtype=torch.int32),
        "threshold": torch.tensor(thr, dtype=torch.float32),
        "left_child": torch.tensor(left, dtype=torch.int32),
        "leaf_value": torch.tensor(leaf, dtype=torch.float32),
        "node_weight": torch.tensor(cov, dtype=torch.float32),
    }


def rows(g, n, nf):
    """Half the cells sit exactly on a threshold value."""
    x = torch.randn(n, nf, generator=g)
    on = torch.tensor(GRID)[torch.randint(0, len(GRID), (n, nf), generator=g)]
    return torch.where(torch.rand(n, nf, generator=g) < 0.5, on, x)


def check(x, trees, weights=None, planes=None, num_planes=1,
          expect="native", label=""):
    w_l = [1.0] * len(trees) if weights is None else list(weights)
    r64 = reference.forest_contrib(x.double(), trees, weights, planes, num_planes)
    r32 = reference.forest_contrib(x, trees, weights, planes, num_planes)
    e_ref32 = float((r32.double() - r64).abs().max())
    scale = sum(abs(w) * float(t["leaf_value"].abs().max())
                for w, t in zip(w_l, trees))
    got = ops.forest_contrib(x.cuda(), trees, weights, planes, num_planes,
                             cache={})
    torch.cuda.synchronize()
    info = dict(ops.last_forest_contrib_info)
    assert info["path"] == expect, info
    assert got.dtype == torch.float32 and got.shape == r64.shape
    err = float((got.cpu().double() - r64).abs().max())
    tol = 4.0 * e_ref32 + 2.0 ** -23 * scale
    print(f"[contrib] {label} N={x.shape[0]} F={x.shape[1]} "
          f"R={info['rows_per_tile']} err={err:.3e} e_ref32={e_ref32:.3e} "
          f"S={scale:.3e} tol={tol:.3e}")
    assert err <= tol
    nf = x.shape[1]
    used = set()
    for t, w in zip(trees, w_l):
        if w != 0:
            used |= {f for f in t["feature"].tolist() if f >= 0}
    unused = [f for f in range(nf) if f not in used]
    if unused:  # features no (weighted) tree splits on: exactly 0.0
        assert bool((got[:, :, unused] == 0).all())
    assert bool((got[:, :, nf] == got[:1, :, nf]).all())  # constant bias
    return got, info


def test_rows_per_tile_policy():
    assert ops.contrib_rows_per_tile(1) == 64
    assert ops.contrib_rows_per_tile(213) == 64
    assert ops.contrib_rows_per_tile(214) == 63  # first F at which R changes
    assert ops.contrib_rows_per_tile(256) == 53
    for f in (1, 37, 213, 214, 256, 3413):
        r = ops.contrib_rows_per_tile(f)
        # [R][F] i64 accumulators + [R][F] f32 rows within the 160 KiB LDS
        assert r >= ops.CONTRIB_MIN_ROWS and 12 * r * f <= 163840
    assert ops.contrib_rows_per_tile(3414) < ops.CONTRIB_MIN_ROWS


@pytest.mark.parametrize("n,nf", [
    (1, 37), (63, 37), (64, 37), (65, 37), (100, 37),  # tile edges at R = 64
    (65, 1), (110, 256),  # R = 53 at F = 256: 2 tiles + 4 rows
    (130, 213), (130, 214),  # R = 64 -> 63: 130 rows are 2 tiles + 2 / + 4
])
def test_kernel_shapes(n, nf):
    g = torch.Generator().manual_seed(1000 * nf + n)
    trees = [random_tree(g, nf, 6) for _ in range(6)]
    weights = [1.0, -0.7, 0.3, 2.0, -1.5, 0.5]
    _, info = check(rows(g, n, nf), trees, weights, label="shapes")
    assert info["rows_per_tile"] == {214: 63, 256: 53}.get(nf, 64)


@pytest.mark.parametrize("m", [1, 7, 8, 9, 15, 16, 17, 31, 32])
def test_kernel_chain_lengths(m):
    """Unique path lengths around every lane-group width (8 / 16 / 32) and
    at the supported maximum."""
    assert ops.CONTRIB_MAX_PATH == 32
    g = torch.Generator().manual_seed(m)
    nf = 37
    perm = torch.randperm(nf, generator=g).tolist()
    trees = [chain_tree(g, perm[:m]), chain_tree(g, perm[nf - m:])]
    assert max(len(e) for _, e in reference._tree_paths(trees[0])) == m
    check(rows(g, 65, nf), trees, [1.0, -0.5], label=f"chain m={m}")


def test_kernel_chain_repeated_features():
    """40 splits over 31 features: merged elements, m = 31."""
    g = torch.Generator().manual_seed(40)
    feats = list(range(31)) + list(range(9))
    tree = chain_tree(g, feats)
    assert max(len(e) for _, e in reference._tree_paths(tree)) == 31
    check(rows(g, 65, 37), [tree], label="chain repeated")


def test_path_over_maximum_routes_to_reference():
    g = torch.Generator().manual_seed(33)
    nf = 37
    trees = [chain_tree(g, torch.randperm(nf, generator=g).tolist()[:33]),
             random_tree(g, nf, 4)]
    check(rows(g, 65, nf), trees, [1.0, 0.5], expect="reference",
          label="chain m=33")


def test_feature_count_over_maximum_routes_to_reference():
    g = torch.Generator().manual_seed(3414)
    nf = 3414
    trees = [random_tree(g, nf, 3)]
    check(rows(g, 3, nf), trees, expect="reference", label="wide F")


def test_kernel_large_forest_many_chunks():
    """64 full depth-6 trees: 4096 paths, so every wave of a block loops
    over many path chunks."""
    g = torch.Generator().manual_seed(64)
    trees = [random_tree(g, 37, 6, p_leaf=0.0) for _ in range(64)]
    assert sum(int((t["feature"] < 0).sum()) for t in trees) == 64 * 64
    weights = [(-1.0) ** i * (0.5 + 0.01 * i) for i in range(64)]
    check(rows(g, 130, 37), trees, weights, label="64 trees")


def test_kernel_is_bitwise_reproducible():
    """The accumulators are integers, so the order in which lane groups
    reach a cell cannot change the bits."""
    g = torch.Generator().manual_seed(77)
    trees = [random_tree(g, 37, 6, p_leaf=0.0) for _ in range(16)]
    x = rows(g, 200, 37).cuda()
    cache = {}
    first = ops.forest_contrib(x, trees, cache=cache)
    for _ in range(3):
        assert torch.equal(ops.forest_contrib(x, trees, cache=cache), first)


def test_kernel_planes_and_weights():
    """3 interleaved planes; negative and zero tree weights."""
    g = torch.Generator().manual_seed(3)
    nf = 37
    trees = [random_tree(g, nf, 5) for _ in range(9)]
    planes = [0, 2, 1, 0, 2, 1, 1, 0, 2]
    weights = [1.0, -2.0, 0.0, 0.5, 0.0, -0.25, 3.0, -1.0, 0.75]
    x = rows(g, 65, nf)
    got, _ = check(x, trees, weights, planes, 3, label="planes")
    # the zero-weight trees are left out of the pack altogether
    pack = ops._pack_contrib(trees, weights, planes, 3, torch.device("cpu"))
    keep = [i for i, w in enumerate(weights) if w != 0]
    kept = ops._pack_contrib(
        [trees[i] for i in keep], [weights[i] for i in keep],
        [planes[i] for i in keep], 3, torch.device("cpu"))
    for k in ("ranges", "path_m", "path_v", "e_feat", "e_z"):
        assert torch.equal(pack[k], kept[k])


def test_kernel_empty_plane_is_zero():
    g = torch.Generator().manual_seed(8)
    trees = [random_tree(g, 5, 3)]
    got, _ = check(rows(g, 10, 5), trees, [1.0], [2], 3, label="empty planes")
    assert bool((got[:, :2, :] == 0).all())


def test_kernel_vector_leaf_tree():
    g = torch.Generator().manual_seed(13)
    tree = random_tree(g, 37, 5, leaf_dim=3)
    # hard-vote style leaves: exact zeros in some outputs
    tree["leaf_value"][::2, 1] = 0.0
    check(rows(g, 65, 37), [tree], None, None, 3, label="K=3 leaves")


def test_kernel_rows_on_thresholds_go_left():
    """x == thr takes the left branch, as the predictors do."""
    tree = _tree([0, -1, -1], [0.5, 0.0, 0.0], [1, -1, -1],
                 [[0.0], [1.0], [3.0]], [10.0, 4.0, 6.0])
    x = torch.tensor([[0.5], [0.5000001], [0.4999999]])
    got, _ = check(x, [tree], label="stump")
    pred = ops.tree_predict(x.cuda(), tree["feature"], tree["threshold"],
                            tree["left_child"], tree["leaf_value"], 64)
    assert pred[:, 0].tolist() == [1.0, 3.0, 1.0]
    assert torch.allclose(got.sum(-1)[:, 0], pred[:, 0], rtol=0, atol=1e-6)


def test_kernel_cache_and_fitted_model():
    """predictContrib of a GBM fitted on the GPU runs the kernel, from the
    pack cached on the model."""
    from spark_ensemble_amd import GBMRegressor
    from spark_ensemble_amd.utils.io import synthetic_regression

    frame = synthetic_regression(2000, 20, seed=17, device="cuda")
    m = GBMRegressor().setNumBaseLearners(4).fit(frame)
    x = frame["features"][:300]
    c1 = m.predictContrib(x)
    assert ops.last_forest_contrib_info["path"] == "native"
    assert c1.shape == (300, 21) and c1.is_cuda
    pack = m._contrib_cache["contrib_pack"]
    m.predictContrib(x)
    assert m._contrib_cache["contrib_pack"] is pack
    trees = [{k: v.cpu() for k, v in t._tree.items()} for t in m._models]
    r64 = reference.forest_contrib(x.cpu().double(), trees, m._weights)
    r32 = reference.forest_contrib(x.cpu(), trees, m._weights)
    tol = 4.0 * float((r32.double() - r64).abs().max()) + 2.0 ** -23 * sum(
        abs(w) * float(t["leaf_value"].abs().max())
        for w, t in zip(m._weights, trees))
    r64[:, 0, -1] += float(m._init._constant)
    assert float((c1.cpu().double() - r64[:, 0]).abs().max()) <= tol
