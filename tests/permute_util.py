"""Helpers shared by tests/test_permute.py and test_permute_gpu.py.

Op-level forests come from tests/serving_util.py: integer leaves in
[-64, 64], tree weights from {0.5, 1, 2}, thresholds and rows from
``INT_POOL`` / ``SPECIALS_POOL``.  With at most ``MAX_EXACT_TREES`` trees,
integer labels and inits in [-4, 4] and unit row weights every margin is a
multiple of 0.5 below 2048 in magnitude, so ``m0 + (v' - v0)`` equals the
direct sum bitwise, ``0.5 d^2`` is an exact f32 (a multiple of 1/8 below
2^21) and every f64 sum over the rows is exact in any order: the exact cases
compare with ``torch.equal``.

The toleranced cases use the rule the project applies to per-row loss sums
over this pack (tests/staged_eval_util.py ``check_op``), per (r, f) entry:

    |got - r64| <= 4 * |r32 - r64| + 2^-23 * sum_i w_i max(|loss_i|, 1)

with r64 / r32 the reference op run on ``x.double()`` / ``x.float()``.
"""

import functools

import torch

import serving_util as su
import staged_eval_util as seu
from spark_ensemble_amd.boosting.losses import SquaredLoss
from spark_ensemble_amd.inspection import draw_donors
from spark_ensemble_amd.ops import dispatch, reference

MAX_EXACT_TREES = 12
# the other eight built-in losses; logloss at dim 1 is the degenerate
# one-class cross-entropy (identically zero), which the op still serves
OTHER_LOSSES = tuple(n for n in seu.ALL_LOSSES if n != "squared")


def exact_args(trees, weights, x, R, seed=0, donor=None):
    """Squared loss, integer labels and inits, unit row weights."""
    assert len(trees) <= MAX_EXACT_TREES
    g = torch.Generator().manual_seed(1000 + seed)
    N = x.shape[0]
    init = torch.randint(-4, 5, (N,), generator=g).float()
    label = torch.randint(-4, 5, (N,), generator=g).float()
    w = torch.ones(N)
    if donor is None:
        donor = draw_donors(N, R, seed)
    return x, trees, weights, init, label, w, SquaredLoss(), donor


def forest_case(seed, N, F, T, depth=4, R=1, pool=su.INT_POOL, p_stop=0.2,
                used=None):
    """Random exact case; ``used`` restricts the split features to a list
    of columns (the rows still have F columns)."""
    g = torch.Generator().manual_seed(seed)
    nf = F if used is None else len(used)
    trees = [su.rand_tree(depth, nf, 1, g, pool, p_stop) for _ in range(T)]
    if used is not None:
        remap = torch.tensor(list(used), dtype=torch.int32)
        for t in trees:
            f = t["feature"].long()
            t["feature"] = torch.where(
                f >= 0, remap[f.clamp_min(0)].long(), f).to(torch.int32)
    weights = su.rand_weights(T, g)
    x = su.special_x(N, F, pool, g)
    return exact_args(trees, weights, x, R, seed)


def toleranced_case(seed, N, F, T, name, depth=4, R=2):
    """The same integer-leaf forests under another loss, with real-valued
    labels, inits and row weights."""
    g = torch.Generator().manual_seed(seed)
    trees = [su.rand_tree(depth, F, 1, g, su.INT_POOL, 0.2) for _ in range(T)]
    # small leaves keep the exponential loss finite
    for t in trees:
        t["leaf_value"] = t["leaf_value"] / 64.0
    weights = su.rand_weights(T, g)
    x = su.special_x(N, F, su.INT_POOL, g)
    loss = seu.make_loss(name, 1)
    label = loss.encode_label(seu.raw_labels(g, N, name, 1))[:, 0]
    init = 0.5 * torch.randn(N, generator=g)
    w = 0.25 + torch.rand(N, generator=g)
    return x, trees, weights, init, label, w, loss, draw_donors(N, R, seed)


def oracle64(args, with_floor=False):
    """(base, perm) float64 from the definition, independent of the
    reference op: column swap, serving_util's float64 walk, ``loss.loss``.
    ``with_floor`` adds the 2^-23 * sum w max(|loss|, 1) term of every
    entry, as (base_floor, perm_floor)."""
    x, trees, weights, init, label, w, loss, donor = args
    xd = x.double().cpu()
    wt = torch.as_tensor([float(v) for v in weights], dtype=torch.float64)
    ini, lab, wr = (t.double().cpu() for t in (init, label, w))
    donor = donor.cpu().long()

    def one(xx):
        m = ini + su.oracle(xx, trees, wt)[:, 0]
        li = loss.loss(lab[:, None], m[:, None])
        return (li * wr).sum(), 2.0 ** -23 * (wr * li.abs().clamp_min(1.0)).sum()

    R, F = donor.shape[0], x.shape[1]
    base, base_floor = one(xd)
    perm = torch.empty(R, F, dtype=torch.float64)
    floor = torch.empty(R, F, dtype=torch.float64)
    for r in range(R):
        for f in range(F):
            xp = xd.clone()
            xp[:, f] = xd[donor[r], f]
            perm[r, f], floor[r, f] = one(xp)
    if with_floor:
        return base, perm, base_floor, floor
    return base, perm


def ref64(args):
    """The float64 reference op on the CPU."""
    x, trees, weights, init, label, w, loss, donor = args
    return reference.forest_permute_loss(
        x.double().cpu(), su.to_dev(trees, "cpu"), weights, init.cpu(),
        label.cpu(), w.cpu(), loss, donor.cpu())


def run_op(args, dev="cpu", cache=None):
    x, trees, weights, init, label, w, loss, donor = args
    base, perm = dispatch.forest_permute_loss(
        x.to(dev), su.to_dev(trees, dev), weights, init.to(dev),
        label.to(dev), w.to(dev), loss, donor, cache=cache)
    assert base.dtype == torch.float64 and perm.dtype == torch.float64
    assert base.shape == () and perm.shape == (donor.shape[0], x.shape[1])
    assert base.device.type == perm.device.type == torch.device(dev).type
    return base.cpu(), perm.cpu()


def check_exact(got, args, want=None):
    """``torch.equal`` against the float64 reference op."""
    base, perm = got
    rb, rp = ref64(args) if want is None else want
    assert torch.equal(base, rb), (base, rb)
    assert torch.equal(perm, rp), (perm - rp).abs().max()
    return rb, rp


def check_tol(got, args, label=""):
    """The project's rule per entry; prints the worst err / tol."""
    x, trees, weights, init, lab, w, loss, donor = args
    base, perm = got
    rb64, rp64 = ref64(args)
    rb32, rp32 = reference.forest_permute_loss(
        x.float().cpu(), su.to_dev(trees, "cpu"), weights, init.cpu(),
        lab.cpu(), w.cpu(), loss, donor.cpu())
    _, _, bfloor, pfloor = oracle64(args, with_floor=True)
    got_all = torch.cat([base.reshape(1), perm.reshape(-1)])
    r64 = torch.cat([rb64.reshape(1), rp64.reshape(-1)])
    r32 = torch.cat([rb32.reshape(1), rp32.reshape(-1)])
    floor = torch.cat([bfloor.reshape(1), pfloor.reshape(-1)])
    err = (got_all - r64).abs()
    tol = 4.0 * (r32 - r64).abs() + floor
    print(f"[permute] {label} N={x.shape[0]} F={x.shape[1]} T={len(trees)} "
          f"R={donor.shape[0]} {loss.name}: err={float(err.max()):.3e} "
          f"e_ref32={float((r32 - r64).abs().max()):.3e} "
          f"floor={float(floor.max()):.3e} "
          f"worst err/tol={float((err / tol).max()):.3f}")
    assert bool((err <= tol).all()), (err, tol)


# ---- hand-built trees -------------------------------------------------------

def tree_from_nodes(nodes):
    """``nodes``: list of (feature, threshold, left) for a split or a
    number for a leaf, in node order (right child = left + 1)."""
    feat, thr, left, leaf = [], [], [], []
    for nd in nodes:
        if isinstance(nd, tuple):
            feat.append(nd[0]); thr.append(float(nd[1])); left.append(nd[2])
            leaf.append([0.0])
        else:
            feat.append(-1); thr.append(0.0); left.append(-1)
            leaf.append([float(nd)])
    return {"feature": torch.tensor(feat, dtype=torch.int32),
            "threshold": torch.tensor(thr, dtype=torch.float32),
            "left_child": torch.tensor(left, dtype=torch.int32),
            "leaf_value": torch.tensor(leaf, dtype=torch.float32)}


def twice_tree():
    """Splits on feature 0 at depth 0 (x0 <= 0) and again at depth 2 on the
    left-left path (x0 <= -2), on feature 1 between them; the right subtree
    of the root splits on feature 0 once more (x0 <= 2), so a sub-walk that
    left at the root meets the swapped feature again.

        0: x0 <= 0 ? 1 : 2
        1: x1 <= 0 ? 3 : 4          2: x0 <= 2 ? 5 : 6
        3: x0 <= -2 ? 7 : 8         4: leaf 10
        5: leaf 20   6: leaf 30     7: leaf 40   8: leaf 50
    """
    return tree_from_nodes([
        (0, 0.0, 1), (1, 0.0, 3), (0, 2.0, 5), (0, -2.0, 7), 10.0,
        20.0, 30.0, 40.0, 50.0])


def chain_tree(depth, F):
    """A right-leaning chain of ``depth`` splits (2 * depth + 1 nodes):
    node 2k splits on feature k % F at 0, its left child is a leaf."""
    nodes = []
    for k in range(depth):
        nodes.append((k % F, 0.0, 2 * k + 1))
        nodes.append(float(k % 7 - 3))
    nodes.append(5.0)
    # node order: split k at index 2k, its left leaf at 2k + 1, and the
    # right child (the next split) must sit at 2k + 2 = left + 1
    return tree_from_nodes(nodes)


# ---- a CPU emulation of the kernel's (row, tree) algorithm -----------------

def emulate_kernel(x, pack, groups, donor_row, f0, fc, binned):
    """Per-row ``m0 [N]`` and ``acc [N, fc]`` the way forest_permute_kernel
    forms them for one (chunk, repeat): packed nodes staged group by group,
    indices relative to the group, base walk, divergence walk with the u64
    diverged mask, sub-walk under the donor's value.  Scalar Python: keep N
    and T small."""
    x = x.float()
    N, F = x.shape
    nodes = (pack["node64b"] if binned else pack["node64"]).tolist()
    if binned:
        rows = su.lower_bound_bins(x, dispatch._binned_edges(pack, F)).tolist()
    else:
        rows = x.tolist()
    offsets = pack["offsets32"].tolist()

    def dec(nd):
        f = su._s16(nd & 0xFFFF)
        left = su._s16((nd >> 16) & 0xFFFF)
        pay = (nd >> 32) & 0xFFFFFFFF
        if binned and f >= 0:
            return f, left, pay
        return f, left, float(su._bits_to_f32(torch.tensor(pay)))

    m0 = [0.0] * N
    acc = [[0.0] * fc for _ in range(N)]
    for first, cnt, base, n_nodes in groups.tolist():
        tlds = [dec(nd) for nd in nodes[base:base + n_nodes]]
        for t in range(first, first + cnt):
            toff = offsets[t] - base
            for i in range(N):
                own, don = rows[i], rows[int(donor_row[i])]
                f, left, pay = tlds[toff]
                while f >= 0:
                    f, left, pay = tlds[toff + left + (0 if own[f] <= pay else 1)]
                v0 = pay
                m0[i] += v0
                diverged = 0
                f, left, pay = tlds[toff]
                while f >= 0:
                    go_left = own[f] <= pay
                    j = f - f0
                    if 0 <= j < fc and not (diverged >> j) & 1:
                        d_left = don[f] <= pay
                        if d_left != go_left:
                            diverged |= 1 << j
                            f2, l2, p2 = tlds[toff + left + (0 if d_left else 1)]
                            while f2 >= 0:
                                v = don[f] if f2 == f else own[f2]
                                f2, l2, p2 = tlds[toff + l2 + (0 if v <= p2 else 1)]
                            acc[i][j] += p2 - v0
                    f, left, pay = tlds[toff + left + (0 if go_left else 1)]
    return torch.tensor(m0, dtype=torch.float64), \
        torch.tensor(acc, dtype=torch.float64).reshape(N, fc)


def permuted_margins64(x, trees, weights, donor_row):
    """[N, F] float64: column f is the forest sum on x with column f taken
    from the donors; and the unshuffled sum [N]."""
    xd = x.double()
    wt = torch.as_tensor([float(v) for v in weights], dtype=torch.float64)
    base = su.oracle(xd, trees, wt)[:, 0]
    cols = []
    for f in range(x.shape[1]):
        xp = xd.clone()
        xp[:, f] = xd[donor_row.long(), f]
        cols.append(su.oracle(xp, trees, wt)[:, 0])
    return base, torch.stack(cols, dim=1)


# ---- model level ------------------------------------------------------------

def margins64(model, x):
    """[N, dim] float64 margins of a GBM, bagging-regression or tree model
    on the CPU: every built-in tree walked in float64
    (staged_eval_util._predict64), other members by their own predict."""
    from spark_ensemble_amd.ensemble.utils import slice_features

    N = x.shape[0]
    if hasattr(model, "_init"):
        stages = seu.model_stages(model)
        m = seu.model_init_margins(model, x).double().cpu().clone()
    elif hasattr(model, "_subspaces"):
        k = len(model._models)
        stages = [([mm], [1.0 / k], sub)
                  for mm, sub in zip(model._models, model._subspaces)]
        m = torch.zeros(N, 1, dtype=torch.float64)
    else:
        stages = [([model], [1.0], None)]
        m = torch.zeros(N, 1, dtype=torch.float64)
    for models, wts, sub in stages:
        xs = x if sub is None else slice_features(x, sub)
        for j, mm in enumerate(models):
            m[:, j] += float(wts[j]) * seu._predict64(mm, xs)
    return m


def brute_force_model(model, frame, loss, margins, numRepeats, seed,
                      weight=None):
    """(r64_base, r64_imp, tol_base, tol_imp): the definition by column
    swaps with the same donors.  r64 takes float64 margins (``margins64``),
    loss and sums; r32 is the same loop over the model's own f32
    ``margins(x) -> [N, dim]`` with f32 losses.  Each loss sum has the
    rule's tolerance ``4 |r32 - r64| + 2^-23 sum w max(|loss|, 1)``; both
    are divided by the weight sum, and an importance entry, the difference
    of a shuffled sum and the base sum, may be off by both tolerances."""
    x = frame["features"].float()
    y = frame["label"].float()
    N, F = x.shape
    w = torch.ones(N, device=x.device) if weight is None else weight.float()
    lab = loss.encode_label(y)
    lab64, w64 = lab.double().cpu(), w.double().cpu()
    donors = draw_donors(N, numRepeats, seed).to(x.device)
    wsum = float(w64.sum())

    def one(xx):
        l64 = loss.loss(lab64, margins64(model, xx))
        s64 = float((l64 * w64).sum())
        m32 = margins(xx).float().reshape(N, -1)
        s32 = float((loss.loss(lab, m32) * w).double().sum())
        fl = 2.0 ** -23 * float((w64 * l64.abs().clamp_min(1.0)).sum())
        return s64, 4.0 * abs(s32 - s64) + fl

    b, tb = one(x)
    imp = torch.empty(numRepeats, F, dtype=torch.float64)
    tol = torch.empty(numRepeats, F, dtype=torch.float64)
    for r in range(numRepeats):
        for f in range(F):
            xp = x.clone()
            xp[:, f] = x[donors[r], f]
            s, t = one(xp)
            imp[r, f] = (s - b) / wsum
            tol[r, f] = (t + tb) / wsum
    return b / wsum, imp, tb / wsum, tol


def check_model(res, want, label=""):
    b, imp, tb, tol = want
    assert isinstance(res.baseline, float)
    assert res.importances.dtype == torch.float64
    assert res.importances.device.type == "cpu"
    assert res.importances.shape == imp.shape
    err = (res.importances - imp).abs()
    eb = abs(res.baseline - b)
    print(f"[permute-model] {label}: err={float(err.max()):.3e} "
          f"worst err/tol={float((err / tol).max()):.3f} "
          f"baseline err/tol={eb / tb:.3f}")
    assert eb <= tb, (eb, tb)
    assert bool((err <= tol).all()), (err, tol)


@functools.lru_cache(maxsize=None)
def sanity_frame():
    """y = 3 x0 + x1 + noise on 8 features, 2000 rows."""
    from spark_ensemble_amd.frame import TensorFrame

    g = torch.Generator().manual_seed(7)
    x = torch.randn(2000, 8, generator=g)
    y = 3.0 * x[:, 0] + x[:, 1] + 0.1 * torch.randn(2000, generator=g)
    return TensorFrame(features=x, label=y)
