"""logreg_loss_grad kernel probe: W-in-registers vs W-in-LDS at the
config-4 shape (5M x 1024, K=2).  Reports achieved TB/s (X bytes / time)
and numerics parity.  NOTE: the SEA_LOGREG_LDS switch is latched at first
launch (static), so the two arms run in separate processes."""
import json
import os
import subprocess
import sys
import time

import torch


def run_arm(name, envvars):
    env = dict(os.environ)
    env.update(envvars)
    env["SEA_ARM"] = name
    r = subprocess.run([sys.executable, __file__, "arm"], env=env,
                       capture_output=True, text=True, cwd="/root/repo")
    assert r.returncode == 0, r.stderr[-1500:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def arm():
    sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
    from spark_ensemble_amd.ops import dispatch

    m = dispatch._load_hip()
    n, F, K = 5_000_000, 1024, 2
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, F, generator=g).to("cuda:0")
    y = torch.randint(0, K, (n,), generator=g, dtype=torch.int32).to("cuda:0")
    w = torch.ones(n, device="cuda:0")
    wmat = (0.01 * torch.randn(F + 1, K, generator=g)).to("cuda:0").contiguous()

    def call():
        payload = torch.zeros(1 + (F + 1) * K, dtype=torch.float32,
                              device="cuda:0")
        m.logreg_loss_grad(payload, x, y, w, wmat, True)
        return payload

    call(); torch.cuda.synchronize()
    t0 = time.time()
    reps = 10
    for _ in range(reps):
        p = call()
    torch.cuda.synchronize()
    dt = (time.time() - t0) / reps
    bytes_x = n * F * 4
    print(json.dumps({
        "mode": os.environ.get("SEA_ARM", "?"),
        "ms": round(dt * 1000, 2),
        "tb_per_s": round(bytes_x / dt / 1e12, 2),
        "loss": float(p[0]),
        "grad_head": [float(v) for v in p[1:4]],
    }))


WIDE_SHAPES = [(2_000_000, 1024, 3), (5_000_000, 256, 26),
               (1_000_000, 1024, 32), (20_000, 16, 26)]


# shapes the narrow kernel serves too, for the dispatcher's choice between
# the two native kernels
BOTH_SHAPES = [(2_000_000, 1024, 2), (2_000_000, 1024, 4),
               (2_000_000, 768, 3), (2_000_000, 768, 5),
               (2_000_000, 512, 3), (2_000_000, 512, 8),
               (4_000_000, 256, 3), (4_000_000, 256, 8)]


def wide(reps=7, shapes=None):
    """The MFMA kernel (csrc/linear_wide.hip) against the three-pass torch
    path it replaces, and against the narrow kernel where that one serves the
    shape: same process, arms alternating, after warm-up, each call timed on
    the host around a device synchronise.  One JSON line per shape with the
    median and the min..max spread in ms and bytes/s as N*F*4 / median."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from spark_ensemble_amd.ops import dispatch, reference

    m = dispatch._load_hip()
    dev = "cuda:0"
    for n, F, K in shapes or WIDE_SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(n, F, generator=g, device=dev)
        y = torch.randint(0, K, (n,), generator=g, device=dev, dtype=torch.int32)
        w = torch.rand(n, generator=g, device=dev)
        wmat = 0.05 * torch.randn(F + 1, K, generator=g, device=dev)

        def native(fn, zero):
            def call():
                make = torch.zeros if zero else torch.empty
                payload = make(1 + (F + 1) * K, dtype=torch.float32, device=dev)
                fn(payload, x, y, w, wmat, True)
                return payload
            return call

        arms = {"wide": native(m.logreg_loss_grad_wide, False),
                "torch": lambda: reference.logreg_loss_grad(x, y, w, wmat, True)}
        if m.logreg_fused_supported(F, K):
            arms["narrow"] = native(m.logreg_loss_grad, True)
        out = {name: call() for name, call in arms.items()}  # warm-up
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(reps):
            for name, call in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = {"n": n, "F": F, "K": K,
               "geometry": list(m.logreg_wide_geometry(F, K))}
        for name, ts in times.items():
            ts.sort()
            med = ts[len(ts) // 2]
            row[name] = {"ms": round(med, 3), "min": round(ts[0], 3),
                         "max": round(ts[-1], 3),
                         "tb_per_s": round(n * F * 4 / med / 1e9, 3)}
            ref = out["torch"]
            row[name]["max_rel_vs_torch"] = float(
                (out[name] - ref).abs().max() / ref.abs().max())
        print(json.dumps(row), flush=True)
        del x, out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "arm":
        arm()
    elif len(sys.argv) > 1 and sys.argv[1] == "wide":
        wide()
    elif len(sys.argv) > 1 and sys.argv[1] == "both":
        wide(shapes=BOTH_SHAPES)
    else:
        arms = {
            "rr2_lds": {},
            "rr4_lds": {"SEA_LOGREG_RR4": "1"},
            "rr2_wreg": {"SEA_LOGREG_WREG": "1"},
        }
        out = {k: run_arm(k, v) for k, v in arms.items()}
        ref = out["rr2_lds"]["loss"]
        out["loss_match"] = all(
            abs(v["loss"] - ref) / max(abs(ref), 1e-9) < 1e-5
            for k, v in out.items() if isinstance(v, dict)
        )
        print(json.dumps(out))
