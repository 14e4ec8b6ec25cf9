"""Helpers shared by tests/test_oob.py and tests/test_oob_gpu.py: in-bag mask
patterns that exercise the 32-bit word packing, the brute-force out-of-bag
loop over today's public API, and the label-noise leakage experiment.

Exactness: the forests come from tests/serving_util.py (integer leaves in
[-64, 64], T <= 65), so every partial sum is an exact f32 and the f32
reference op, its float64 run and the kernel agree bit for bit."""

import torch

import spark_ensemble_amd as sea
from spark_ensemble_amd.ensemble.utils import slice_features
from spark_ensemble_amd.frame import TensorFrame
from spark_ensemble_amd.ops import reference
from spark_ensemble_amd.utils.io import synthetic_classification


def mask_patterns(n, T, gen):
    """[n, T] bool in-bag mask, mixed per row: random p = 0.5 everywhere,
    then, at the first and at the last rows (as far as n allows): a row all
    True (in every bag), a row all False, a row with only bit 31 out of bag,
    a row with only bit 32 out of bag."""
    m = torch.rand(n, T, generator=gen) < 0.5
    pats = [torch.ones(T, dtype=torch.bool), torch.zeros(T, dtype=torch.bool)]
    for t in (31, 32):
        if T > t:
            p = torch.ones(T, dtype=torch.bool)
            p[t] = False
            pats.append(p)
    for j, p in enumerate(pats):
        if n - 1 - j >= 0:
            m[n - 1 - j] = p
    for j, p in enumerate(pats):  # the first rows win when n is small
        if j < n:
            m[j] = p
    return m


def oracle(x, trees, inbag):
    """(sums float64, counts) of the reference op on x.double(), CPU."""
    cpu = [{k: v.cpu() for k, v in t.items()} for t in trees]
    return reference.forest_oob(x.cpu().double(), cpu, inbag.cpu())


def check_exact(got, x, trees, inbag, label=""):
    """``got`` (sums, counts) equals the f32 reference op on the CPU, which
    in turn equals its own float64 run."""
    cpu = [{k: v.cpu() for k, v in t.items()} for t in trees]
    s32, c32 = reference.forest_oob(x.cpu().float(), cpu, inbag.cpu())
    s64, c64 = oracle(x, trees, inbag)
    assert s32.dtype == torch.float32 and c32.dtype == torch.int32
    assert torch.equal(s32.double(), s64), label
    assert torch.equal(c32, c64), label
    sums, counts = got
    assert sums.dtype == torch.float32 and counts.dtype == torch.int32
    assert sums.shape == s32.shape and counts.shape == c32.shape, label
    assert torch.equal(counts.cpu(), c32), label
    assert torch.equal(sums.cpu(), s32), label
    # a row in every bag gets sums = 0, counts = 0
    full = inbag.cpu().all(dim=1)
    assert bool((counts.cpu()[full] == 0).all()), label
    assert bool((sums.cpu()[full] == 0).all()), label


# ---- estimator level -------------------------------------------------------

def brute_force(est, model, frame, vote=None, weight=None):
    """(sums, counts) of the out-of-bag loop over the public API: bag i is
    regenerated with ``est.sample_weights`` at seed + i, member i predicts
    on its own feature slice, and the members are added in order.
    ``vote`` None: regression sums [N]; "soft" / "hard": vote sums [N, K]."""
    x = frame["features"].float()
    n = x.shape[0]
    w = weight if weight is not None else torch.ones(n, device=x.device)
    seed = est.getOrDefault("seed")
    sums, counts = None, torch.zeros(n, dtype=torch.int32, device=x.device)
    for i, (m, sub) in enumerate(zip(model.models, model.subspaces)):
        bw = est.sample_weights(est.getReplacement(), est.getSubsampleRatio(),
                                n, seed + i, x.device, w, 0)
        out = ~(bw > 0)
        xs = slice_features(x, sub)
        if vote is None:
            p = m.predict(xs).float()
        elif vote == "soft":
            p = m.predictProbability(xs).float()
        else:
            p = torch.zeros(n, model._num_classes, device=x.device)
            p.scatter_(1, m.predict(xs).long().unsqueeze(1), 1.0)
        mask = out if p.dim() == 1 else out[:, None]
        p = torch.where(mask, p, torch.zeros((), device=x.device))
        sums = p if sums is None else sums + p
        counts += out.to(torch.int32)
    return sums, counts


def check_regressor(est, frame, weight=None):
    model = est.setComputeOob(True).fit(frame)
    sums, counts = brute_force(est, model, frame, weight=weight)
    assert model.oobCounts.dtype == torch.int32
    assert torch.equal(model.oobCounts, counts)
    has = counts > 0
    assert bool(has.any())
    pred = model.oobPrediction
    assert pred.dtype == torch.float32 and pred.shape == sums.shape
    assert torch.equal(pred[has], (sums / counts)[has])
    assert bool(pred[~has].isnan().all())
    # weighted R^2 over the covered rows, float64
    y = frame["label"].double()
    w = (weight if weight is not None else torch.ones_like(pred)).double()
    wc = torch.where(has, w, torch.zeros_like(w))
    mean = float((wc * y).sum() / wc.sum())
    resid = torch.where(has, y - pred.double(), torch.zeros_like(y))
    r2 = 1.0 - float((wc * resid ** 2).sum()) / float((wc * (y - mean) ** 2).sum())
    assert abs(model.oobScore - r2) <= 1e-9 * max(1.0, abs(r2))
    assert abs(model.oobCoverage - float(wc.sum() / w.sum())) <= 1e-12
    return model


def check_classifier(est, frame, weight=None):
    vote = est.getVotingStrategy()
    model = est.setComputeOob(True).fit(frame)
    sums, counts = brute_force(est, model, frame, vote=vote, weight=weight)
    assert torch.equal(model.oobCounts, counts)
    raw = model.oobRawPrediction
    assert raw.dtype == torch.float32 and raw.shape == sums.shape
    assert torch.equal(raw, sums)
    has = counts > 0
    prob, pred = model.oobProbability, model.oobPrediction
    assert torch.equal(prob[has], (sums / counts[:, None])[has])
    assert bool(prob[~has].isnan().all())
    assert torch.equal(pred[has], sums.argmax(dim=1).float()[has])
    assert bool(pred[~has].isnan().all())
    y = frame["label"]
    w = (weight if weight is not None else torch.ones_like(pred)).double()
    wc = torch.where(has, w, torch.zeros_like(w))
    acc = float((wc * (pred == y).double()).sum() / wc.sum())
    assert abs(model.oobScore - acc) <= 1e-12
    assert abs(model.oobCoverage - float(wc.sum() / w.sum())) <= 1e-12
    return model


def leakage_experiment(device):
    """Labels independent of the features: (training accuracy, oobScore,
    oobCoverage) of 10 depth-12 hard-voting trees."""
    frame = synthetic_classification(4000, 20, k=2, seed=13, device=device)
    g = torch.Generator().manual_seed(0)
    y = torch.randint(0, 2, (4000,), generator=g).float().to(device)
    frame = TensorFrame(features=frame["features"], label=y)
    est = (sea.BaggingClassifier()
           .setBaseLearner(sea.DecisionTreeClassifier().setMaxDepth(12))
           .setNumBaseLearners(10).setVotingStrategy("hard")
           .setComputeOob(True))
    model = est.fit(frame)
    train = float((model.predict(frame["features"]) == y).float().mean())
    return train, model.oobScore, model.oobCoverage
