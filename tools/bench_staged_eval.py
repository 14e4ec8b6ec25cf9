"""evaluateEachIteration (one fused forest pass) against the per-stage loop
it replaces, on one GPU.

Two shapes: a --stages-bin stage depth-6 bernoulli model and a --stages-k3
stage logloss k=3 model, each fitted on --fit-rows rows and evaluated on
--rows x --features rows.  The loop is the one ``fit`` runs for its validation
rows, written with what a user has: per stage ``model.predict`` of the stage
model, add into the margins, ``loss.loss`` and a mean (one host sync per
stage).  Prints one JSON line per shape: median and min wall seconds of each
over --reps warm repeats (the two alternate inside one process, every repeat
ends in a device synchronise), the ratio, the op alone in each row mode, and
the rate at which the fused pass moves x.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed(fn):
    import torch

    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _loop(model, frame, loss, dim):
    """The per-stage curve by hand (what fit does for validation rows)."""
    import torch

    from spark_ensemble_amd.ensemble.utils import slice_features
    from spark_ensemble_amd.utils.stats import dist_mean

    x = frame["features"].float()
    label = loss.encode_label(frame["label"].float())
    init = model._init
    if dim == 1 and not hasattr(model, "_dim"):
        margins = init.predict(x).unsqueeze(1)
    else:
        margins = init.predictRaw(x)[:, :dim].contiguous()
    out = [dist_mean(loss.loss(label, margins))]
    for ms, wts, sub in zip(model.models, model.weights, model._subspaces):
        ms = ms if isinstance(ms, list) else [ms]
        wts = wts if isinstance(wts, list) else [wts]
        xs = slice_features(x, sub)
        step = torch.stack([m.predict(xs) for m in ms], dim=1)
        margins = margins + step * torch.tensor(
            wts, dtype=torch.float32, device=x.device).unsqueeze(0)
        out.append(dist_mean(loss.loss(label, margins)))
    return torch.tensor(out, dtype=torch.float64)


def _shape(name, est, loss, dim, fit_frame, frame, reps):
    import torch

    from spark_ensemble_amd.ops import dispatch as ops

    t_fit, model = _timed(lambda: est.fit(fit_frame))
    fused = lambda: model.evaluateEachIteration(frame)  # noqa: E731
    loop = lambda: _loop(model, frame, loss, dim)  # noqa: E731
    a, b = fused(), loop()  # warm both: packs, code objects
    info = dict(ops.last_forest_staged_info)
    torch.cuda.synchronize()
    tf, tl = [], []
    for _ in range(reps):
        tf.append(_timed(fused)[0])
        tl.append(_timed(loop)[0])
    modes = {}
    for mode in ("binned", "raw"):
        os.environ["SEA_STAGED_MODE"] = mode
        fused()
        torch.cuda.synchronize()
        modes[mode] = sorted(_timed(fused)[0] for _ in range(reps))[reps // 2]
    os.environ.pop("SEA_STAGED_MODE")
    n, f = frame["features"].shape
    med_f, med_l = sorted(tf)[reps // 2], sorted(tl)[reps // 2]
    print(json.dumps({
        "shape": name, "rows": n, "features": f, "stages": model.numModels,
        "dim": dim, "fit_s": round(t_fit, 3), "path": info.get("path"),
        "mode": info.get("mode"), "rows_per_lane": info.get("rows_per_lane"),
        "groups": info.get("groups"),
        "fused_s_median": med_f, "fused_s_min": min(tf),
        "loop_s_median": med_l, "loop_s_min": min(tl),
        "loop_over_fused": med_l / med_f,
        "fused_s_binned": modes["binned"], "fused_s_raw": modes["raw"],
        "x_gb_per_s": n * f * 4 / med_f / 1e9,
        "max_abs_diff_fused_vs_loop": float((a - b).abs().max()),
    }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--fit-rows", type=int, default=200_000)
    ap.add_argument("--stages-bin", type=int, default=100)
    ap.add_argument("--stages-k3", type=int, default=30)
    ap.add_argument("--depth", type=int, default=6)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    import spark_ensemble_amd as sea
    from spark_ensemble_amd.boosting.losses import get_classification_loss
    from spark_ensemble_amd.models import DecisionTreeRegressor
    from spark_ensemble_amd.utils.io import synthetic_classification

    tree = lambda: DecisionTreeRegressor().setMaxDepth(args.depth)  # noqa: E731
    for name, k, loss_name, stages in (
            ("bernoulli", 2, "bernoulli", args.stages_bin),
            ("logloss_k3", 3, "logloss", args.stages_k3)):
        fit_frame = synthetic_classification(
            args.fit_rows, args.features, k=k, seed=31, device="cuda")
        frame = synthetic_classification(
            args.rows, args.features, k=k, seed=31, split=1, device="cuda")
        est = (sea.GBMClassifier().setLoss(loss_name).setBaseLearner(tree())
               .setNumBaseLearners(stages))
        loss = get_classification_loss(loss_name, k)
        _shape(name, est, loss, loss.dim, fit_frame, frame, args.reps)


if __name__ == "__main__":
    main()
