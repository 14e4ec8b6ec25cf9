"""The gfx950 forest_vote kernel against the float64 reference ops on the CPU.

Hard votes and counts are exact (``torch.equal``).  Soft votes are T f32 adds
of non-negative terms in member order, so they lie within ``(T - 1) * 2**-24
* row_sum`` of the float64 sums, and they equal the ``SEA_VOTE_WIDE=0`` route
(the v1 kernel, or the reference op under a mask) bit for bit."""

import math

import pytest
import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.ensemble.utils import _vote_leaves, orig_space_features
from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.utils.io import synthetic_classification

import oob_util as U
import serving_util as S
from test_forest_vote import voting

pytestmark = pytest.mark.gpu

BUDGET = ops._FP2_GROUP_NODES
KP = {9: 12, 12: 12, 13: 16, 16: 16, 17: 24, 24: 24, 25: 32, 32: 32}
VOTES, MODES = [False, True], ["raw", "binned"]


def check(mp, x, trees, soft, mode=None, inbag=None, expect="native"):
    """``trees`` are already transformed (``voting``).  Runs forest_vote on
    the GPU, with and without ``inbag``, against the float64 ops."""
    if mode is not None:
        mp.setenv("SEA_VOTE_MODE", mode)
    dev, T = S.to_dev(trees, "cuda"), len(trees)
    K = trees[0]["leaf_value"].shape[1]
    for bag in ([None] if inbag is None else [None, inbag]):
        got = ops.forest_vote(x.cuda(), dev, soft, inbag=bag)
        info = dict(ops.last_forest_vote_info)
        assert info["path"] == expect, info
        if expect == "native":
            assert info["vote"] == ("soft" if soft else "hard")
            assert info["kp"] == (KP[K] if soft else 32), info
            assert mode is None or info["mode"] == mode, info
        if bag is None:
            want = S.oracle(x, trees)
        else:
            want, counts = U.oracle(x, trees, bag)
            assert torch.equal(got[1].cpu(), counts)
            got = got[0]
            assert bool((got.cpu()[bag.all(dim=1)] == 0).all())
        assert got.dtype == torch.float32 and got.shape == want.shape
        if not soft:
            assert torch.equal(got.cpu().double(), want)
            continue
        err = (got.cpu().double() - want).abs()
        bound = (T - 1) * 2.0 ** -24 * want.sum(dim=1, keepdim=True)
        print("soft max err", float(err.max()), "bound", float(bound.max()))
        assert bool((err <= bound).all())
        mp.setenv("SEA_VOTE_WIDE", "0")
        old = ops.forest_vote(x.cuda(), dev, soft, inbag=bag)
        assert ops.last_forest_vote_info["path"] == "reference"
        mp.delenv("SEA_VOTE_WIDE")
        assert torch.equal(got, old if bag is None else old[0])
    return info


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("soft", VOTES)
@pytest.mark.parametrize("K", sorted(KP))
def test_class_counts(monkeypatch, K, soft, mode):
    g = torch.Generator().manual_seed(K)
    trees = [S.rand_tree(6, 20, K, g, S.SPECIALS_POOL, p_stop=0.2)
             for _ in range(12)]
    trees.insert(6, S.leaf_tree(K, 2.0))
    x = S.special_x(600, 20, S.SPECIALS_POOL, g)
    check(monkeypatch, x, voting(trees, soft), soft, mode,
          inbag=U.mask_patterns(600, 13, g))


@pytest.mark.parametrize("soft", VOTES)
@pytest.mark.parametrize("n", [1, 63, "tile", "tile+1", "wrap"])
def test_row_counts(monkeypatch, n, soft):
    geo = ops.forest_vote_geometry()
    tile = geo["threads"] * geo["rows_per_lane"][12 if soft else "hard"]
    if isinstance(n, str):
        n = {"tile": tile, "tile+1": tile + 1,
             "wrap": geo["grid_cap"] * tile + 1}[n]
    g = torch.Generator().manual_seed(5)
    trees = [S.rand_tree(3, 5, 9, g, S.INT_POOL) for _ in range(3)]
    info = check(monkeypatch, S.special_x(n, 5, S.INT_POOL, g),
                 voting(trees, soft), soft)
    assert info["rows_per_lane"] * geo["threads"] == tile


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("soft", VOTES)
@pytest.mark.parametrize("sizes,groups", [
    ([BUDGET - 1, 1], 1),       # one group, filled exactly
    ([BUDGET - 1, 3], 2),       # one node too many
    ([BUDGET - 1, 1, 1, BUDGET - 3, 1, 1, 7, 1], 3),  # root-only at the edges
])
def test_groups(monkeypatch, sizes, groups, soft, mode):
    g = torch.Generator().manual_seed(len(sizes))
    trees = [S.sized_tree(n, 5, 9, g, S.INT_POOL) for n in sizes]
    x = S.special_x(300, 5, S.INT_POOL, g)
    info = check(monkeypatch, x, voting(trees, soft), soft, mode,
                 inbag=U.mask_patterns(300, len(sizes), g))
    assert info["groups"] == groups


@pytest.mark.parametrize("soft", VOTES)
@pytest.mark.parametrize("T", [31, 32, 33, 70])
def test_mask_words(monkeypatch, T, soft):
    g = torch.Generator().manual_seed(T)
    # a tree that fills a group alone: group boundaries inside a mask word
    trees = [S.rand_tree(4, 6, 12, g, S.INT_POOL, p_stop=0.2) for _ in range(T)]
    trees[T // 2] = S.sized_tree(BUDGET - 1, 6, 12, g, S.INT_POOL)
    x = S.special_x(300, 6, S.INT_POOL, g)
    vt = voting(trees, soft)
    info = check(monkeypatch, x, vt, soft, inbag=U.mask_patterns(300, T, g))
    assert info["groups"] >= 2
    bootstrap = torch.rand(300, T, generator=g) < 1.0 - math.exp(-1.0)
    check(monkeypatch, x, vt, soft, inbag=bootstrap)


def test_hard_counter_fields(monkeypatch):
    # 300 votes on one class (past 8 bits), and the field / word edges of K = 32
    votes = [31] * 300 + [0] * 2 + [3] * 3 + [4] * 5
    trees = []
    for c in votes:
        t = S.leaf_tree(32, 0.0)
        t["leaf_value"][0, c] = 1.0
        trees.append(t)
    check(monkeypatch, torch.zeros(70, 3), trees, False,
          inbag=torch.rand(70, len(votes)) < 0.5)


@pytest.mark.parametrize("soft", VOTES)
@pytest.mark.parametrize("why", ["K8", "K33", "oversize", "env", "thresholds"])
def test_declines(monkeypatch, why, soft):
    g = torch.Generator().manual_seed(9)
    K = {"K8": 8, "K33": 33}.get(why, 12)
    trees = [S.rand_tree(4, 4, K, g, S.INT_POOL, p_stop=0.2) for _ in range(5)]
    expect = "reference"
    if why == "oversize":
        trees.append(S.sized_tree(BUDGET + 1, 4, K, g, S.INT_POOL))
    elif why == "env":
        monkeypatch.setenv("SEA_VOTE_WIDE", "0")
    elif why == "thresholds":  # no u8 rank form: the raw walk is still native
        trees.append(S.sized_tree(2047, 1, K, g, torch.arange(4000.0) / 8))
        expect = "native"
    x = S.special_x(400, 4, S.INT_POOL, g)
    inbag = U.mask_patterns(400, len(trees), g)
    if expect == "native":
        info = check(monkeypatch, x, voting(trees, soft), soft, inbag=inbag)
        assert info["mode"] == "raw"
        return
    dev = S.to_dev(voting(trees, soft), "cuda")
    got = ops.forest_vote(x.cuda(), dev, soft)
    assert ops.last_forest_vote_info["path"] == "reference"
    assert torch.equal(got, ops.forest_predict(x.cuda(), dev))
    sums, counts = ops.forest_vote(x.cuda(), dev, soft, inbag=inbag)
    want = ops.forest_oob(x.cuda(), dev, inbag)
    assert torch.equal(sums, want[0]) and torch.equal(counts, want[1])
    assert ops.forest_vote(x.cuda(), dev, soft, native_only=True) is None


@pytest.mark.parametrize("vote", ["hard", "soft"])
def test_bagging_classifier_end_to_end(vote):
    soft = vote == "soft"
    frame = synthetic_classification(3000, 10, k=12, seed=3, device="cuda")
    est = (sea.BaggingClassifier()
           .setBaseLearner(sea.DecisionTreeClassifier().setMaxDepth(5))
           .setNumBaseLearners(7).setSubspaceRatio(0.7).setSeed(2)
           .setVotingStrategy(vote).setComputeOob(True))
    ops.last_forest_vote_info.clear()
    model = est.fit(frame)
    assert ops.last_forest_vote_info["path"] == "native"
    x = frame["features"].float()
    n, T = x.shape[0], model.numModels
    trees = [{**{k: v.cpu() for k, v in m._tree.items()},
              "feature": orig_space_features(m, sub, x.shape[1]).cpu(),
              "leaf_value": _vote_leaves(m, soft).cpu()}
             for m, sub in zip(model.models, model.subspaces)]
    ops.last_forest_vote_info.clear()
    raw = model.predictRaw(x).cpu().double()
    assert ops.last_forest_vote_info["path"] == "native"
    want = S.oracle(x, trees)  # the per-member loop over _vote_leaves
    tol = (T - 1) * 2.0 ** -24 * want.sum(dim=1, keepdim=True) if soft else 0
    assert bool(((raw - want).abs() <= tol).all())
    inbag = torch.stack(
        [est.sample_weights(est.getReplacement(), est.getSubsampleRatio(), n,
                            est.getOrDefault("seed") + i, x.device,
                            torch.ones(n, device=x.device), 0) > 0
         for i in range(T)], dim=1).cpu()
    sums, counts = U.oracle(x, trees, inbag)
    assert torch.equal(model.oobCounts.cpu(), counts)
    has = counts > 0
    hit = (sums.argmax(dim=1) == frame["label"].cpu().long()) & has
    assert abs(model.oobScore - float(hit.sum()) / float(has.sum())) <= 1e-12
