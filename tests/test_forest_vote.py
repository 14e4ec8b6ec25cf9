"""Host side of forest_vote: what ``_pack_forest_vote`` puts into the node
payloads and the leaf table, and the route of CPU tensors."""

import types

import pytest
import torch

from spark_ensemble_amd.ensemble.utils import _vote_leaves
from spark_ensemble_amd.ops import dispatch as ops

import serving_util as S

CPU = torch.device("cpu")


def voting(trees, soft):
    """The trees with class-count leaves (|integer leaf|) transformed per
    node by ``_vote_leaves``, as ``packed_forest_vote`` hands them on."""
    out = []
    for t in trees:
        m = types.SimpleNamespace(_tree=dict(t, leaf_value=t["leaf_value"].abs()))
        out.append(dict(t, leaf_value=_vote_leaves(m, soft)))
    return out


def forest(K, soft, g):
    trees = [S.rand_tree(5, 7, K, g, S.INT_POOL, p_stop=0.2) for _ in range(6)]
    trees.insert(3, S.leaf_tree(K, 3.0))
    return voting(trees, soft)


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("K,kp", [(9, 12), (12, 12), (13, 16), (17, 24),
                                  (25, 32), (32, 32)])
def test_payloads_and_table(K, kp, soft):
    vt = forest(K, soft, torch.Generator().manual_seed(K))
    pack = ops._pack_forest_vote(vt, soft, CPU)
    leaves = torch.cat([t["leaf_value"] for t in vt])
    is_leaf = torch.cat([t["feature"] for t in vt]) < 0
    n_leaves = int(is_leaf.sum())
    if soft:  # row indices enumerate the leaves in node order
        want = torch.arange(n_leaves)
        assert pack["kp"] == kp and pack["table"].shape == (n_leaves, kp)
        assert torch.equal(pack["table"][:, :K], leaves[is_leaf])
        assert bool((pack["table"][:, K:] == 0).all())
    else:     # the class id is the argmax of the one-hot row
        want = leaves.argmax(dim=1)[is_leaf]
        assert pack["kp"] == 32 and pack["table"].numel() == 0
    for key in ("node64", "node64b"):
        assert torch.equal(((pack[key] >> 32) & 0xFFFFFFFF)[is_leaf], want)
    # an inner node keeps its threshold bits
    thr = torch.cat([t["threshold"] for t in vt])
    assert torch.equal(S._bits_to_f32(pack["node64"] >> 32)[~is_leaf],
                       thr[~is_leaf])


@pytest.mark.parametrize("soft", [False, True])
def test_groups_are_those_of_pack_forest(soft):
    g = torch.Generator().manual_seed(4)
    budget = ops._FP2_GROUP_NODES
    sizes = [budget - 1, 1, budget - 3, 3, 1, 5]  # two full groups and a tail
    trees = voting([S.sized_tree(n, 5, 9, g, S.INT_POOL) for n in sizes], soft)
    pack = ops._pack_forest_vote(trees, soft, CPU)
    S.check_groups(pack, trees)
    # _pack_forest cuts groups only for D <= 8: same sizes, scalar leaves
    narrow = [dict(t, leaf_value=t["leaf_value"][:, :1]) for t in trees]
    want = ops._pack_forest(narrow, None, CPU)
    assert torch.equal(pack["groups_t"], want["groups_t"])
    assert torch.equal(pack["offsets32"], want["offsets32"])
    over = trees + voting([S.sized_tree(budget + 1, 5, 9, g, S.INT_POOL)], soft)
    assert ops._pack_forest_vote(over, soft, CPU)["fits"] is False


@pytest.mark.parametrize("soft", [False, True])
def test_cpu_tensors_take_the_old_route(soft):
    g = torch.Generator().manual_seed(21)
    vt = forest(12, soft, g)
    x = S.special_x(200, 7, S.INT_POOL, g)
    inbag = torch.rand(200, len(vt), generator=g) < 0.63
    got = ops.forest_vote(x, vt, soft)
    assert ops.last_forest_vote_info["path"] == "reference"
    assert torch.equal(got, ops.forest_predict(x, vt))
    sums, counts = ops.forest_vote(x, vt, soft, inbag=inbag)
    want = ops.forest_oob(x, vt, inbag)
    assert torch.equal(sums, want[0]) and torch.equal(counts, want[1])
    assert ops.forest_vote(x, vt, soft, native_only=True) is None
