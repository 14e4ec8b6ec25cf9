"""Host side of forest_margin: the torch reference op against the float64
oracle, and what ``_pack_forest_margin`` hands the kernel."""

import pytest
import torch

from spark_ensemble_amd.ops import dispatch as ops, reference

import serving_util as S

CPU = torch.device("cpu")
PLANES = [2, 9, 26, 33]


def forest(P, g, pool=S.INT_POOL, F=6):
    """Two stages of shuffled planes (stage-major, so the stable sort has
    work to do): two small random trees per plane, plane 1 a single
    root-only tree, and plane 4 of ``P == 9`` empty."""
    trees, planes = [], []
    for stage in range(2):
        for j in torch.randperm(P, generator=g).tolist():
            if (j == 1 and stage == 1) or (P == 9 and j == 4):
                continue
            trees.append(S.leaf_tree(1, 5.0) if j == 1 else
                         S.rand_tree(3, F, 1, g, pool, p_stop=0.3))
            planes.append(j)
    return trees, S.rand_weights(len(trees), g), planes


def expected(x, trees, weights, planes, P):
    """[N, P] float64: the oracle walk over each plane's trees."""
    out = torch.zeros(x.shape[0], P, dtype=torch.float64)
    for j in range(P):
        idx = [t for t, p in enumerate(planes) if p == j]
        if idx:
            out[:, j] = S.oracle(x, [trees[t] for t in idx], weights[idx])[:, 0]
    return out


@pytest.mark.parametrize("P", PLANES)
def test_reference_equals_oracle(P):
    g = torch.Generator().manual_seed(P)
    trees, w, planes = forest(P, g)
    x = S.special_x(200, 6, S.INT_POOL, g)
    want = expected(x, trees, w, planes, P)
    got = reference.forest_margin(x, trees, w, planes, P)
    assert got.dtype == torch.float32 and torch.equal(got.double(), want)
    # CPU tensors take the declined route of the dispatcher
    assert torch.equal(ops.forest_margin(x, trees, w, planes, P), got)
    assert ops.last_forest_margin_info["path"] == "reference"
    assert ops.forest_margin(x, trees, w, planes, P, native_only=True) is None


def test_pack_is_plane_major():
    g = torch.Generator().manual_seed(3)
    # 42 x 1023 nodes, given stage-major: groups cut at trees 19 and 38 of
    # the PACK order, planes at 14 and 28
    trees = [S.complete_tree(9, 5, 1, g, S.INT_POOL) for _ in range(42)]
    planes = [t % 3 for t in range(42)]
    w = S.rand_weights(42, g)
    pack = ops._pack_forest_margin(trees, w, planes, CPU)
    order = pack["order"]
    assert order == [3 * s + j for j in range(3) for s in range(14)]
    assert pack["planes_t"].tolist() == [0] * 14 + [1] * 14 + [2] * 14
    packed = [trees[i] for i in order]
    groups = S.check_groups(pack, packed)
    assert [grp[0] for grp in groups] == [0, 19, 38]
    # a leaf carries weight * leaf, an inner node its threshold (or its rank)
    is_leaf = torch.cat([t["feature"] for t in packed]) < 0
    wl = torch.cat([w[i] * trees[i]["leaf_value"][:, 0] for i in order])
    thr = torch.cat([t["threshold"] for t in packed])
    for key in ("node64", "node64b"):
        assert torch.equal(S._bits_to_f32(pack[key] >> 32)[is_leaf],
                           wl[is_leaf])
    assert torch.equal(S._bits_to_f32(pack["node64"] >> 32)[~is_leaf],
                       thr[~is_leaf])
    over = trees + [S.sized_tree(ops._FP2_GROUP_NODES + 1, 5, 1, g, S.INT_POOL)]
    assert ops._pack_forest_margin(over, [1.0] * 43, planes + [0], CPU)[
        "fits"] is False
