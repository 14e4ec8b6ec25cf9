"""Host-side planner of the MFMA logistic kernel (csrc/linear_wide.hip) through
``logreg_wide_geometry``, and the planted-fault check of the float64
comparator in tests/logreg_util.py.  No test here touches a device."""

import pytest
import torch

import logreg_util as U

LDS_BUDGET = 163840

# F, K -> KP, S, rows, NT, db, LDS bytes: worked out from the planner's
# arithmetic by hand, not by a copy of it
PINNED = [
    (1, 9, 16, 1, 128, 1, 1, 44032),
    (31, 9, 16, 1, 128, 2, 1, 60416),
    (31, 26, 32, 1, 128, 2, 1, 84992),
    (36, 9, 16, 1, 128, 4, 1, 76800),
    (36, 26, 32, 1, 128, 4, 1, 101376),
    (100, 9, 16, 1, 128, 8, 1, 142336),
    (100, 26, 32, 1, 128, 8, 0, 108544),
    (128, 9, 16, 1, 128, 8, 1, 158720),
    (128, 26, 32, 1, 128, 8, 0, 116736),
    (130, 26, 32, 2, 64, 8, 1, 108032),
    (240, 26, 32, 2, 64, 8, 1, 157184),
    (244, 9, 16, 2, 64, 8, 1, 148992),
    (244, 26, 32, 2, 64, 8, 0, 99328),
    (257, 26, 32, 4, 32, 8, 1, 94976),
    (512, 26, 32, 4, 32, 8, 1, 156416),
    (515, 26, 32, 8, 16, 8, 1, 88448),
    (1024, 26, 32, 8, 16, 8, 1, 151936),
]


@pytest.fixture(scope="module")
def ext():
    return pytest.importorskip("spark_ensemble_amd._hip_ops")


@pytest.mark.parametrize("f,k,kp,s,rows,nt,db,lds", PINNED)
def test_pinned_geometry(ext, f, k, kp, s, rows, nt, db, lds):
    assert ext.logreg_wide_supported(f, k)
    assert tuple(ext.logreg_wide_geometry(f, k)) == (kp, s, rows, lds, nt, db)


def test_invariants_over_every_shape(ext):
    single = set()
    for f in range(1, 1025):
        t = -(-f // 16)
        for k in range(2, 33):
            assert ext.logreg_wide_supported(f, k), (f, k)
            kp, s, rows, lds, nt, db = ext.logreg_wide_geometry(f, k)
            where = (f, k, kp, s, rows, lds, nt, db)
            assert (kp == 16) == (k <= 16) and kp in (16, 32), where
            assert s in (1, 2, 4, 8) and rows * s == 128, where
            nts = -(-t // s)
            assert nts <= 8, where
            assert nt in (1, 2, 4, 8) and nt >= nts and nt < 2 * nts, where
            assert 0 < lds <= LDS_BUDGET, where
            second_tile = rows * (16 * t + 2) * 4
            if db == 1:
                # lds already holds both tiles
                assert lds > 2 * second_tile, where
            else:
                assert db == 0 and lds + second_tile > LDS_BUDGET, where
            # two staging halves of ceil(NT/2) float4 per thread cover the tile
            assert rows * -(-f // 4) <= 512 * 2 * -(-nt // 2), where
            if db == 0:
                single.add((s, t, kp))
    assert single == {(1, 7, 32), (1, 8, 32), (2, 16, 32)}


@pytest.mark.parametrize("f,k", [(16, 1), (16, 33), (0, 9), (1025, 9)])
def test_unsupported_shapes(ext, f, k):
    assert not ext.logreg_wide_supported(f, k)
    assert tuple(ext.logreg_wide_geometry(f, k)) == (0, 0, 0, 0, 0, 0)


def test_cpu_tensors_take_the_reference():
    from spark_ensemble_amd.ops import dispatch

    x, y, w, wmat = U.inputs(7, 16, 9, True, 0.05)
    got = dispatch.logreg_loss_grad(x, y, w, wmat, True)
    assert dispatch.last_logreg_info == {
        "path": "reference", "kp": 0, "slices": 0, "rows_per_tile": 0,
        "lds_bytes": 0, "nt": 0, "db": 0}
    assert torch.equal(got, U.reference.logreg_loss_grad(x, y, w, wmat, True))
    assert dispatch.logreg_loss_grad(x, y, w, wmat, True, native_only=True) is None


# --- the comparator rejects the faults the GPU tests exist for --------------

N, F, K = 333, 100, 26


def _payload(x, y, w, wmat, *, x_margin=None, bias_in_margin=True,
             extra_class=False, rows=None):
    """The float64 payload, computed as a kernel with one planted fault
    would: ``x_margin`` replaces x in both products, ``rows`` keeps only the
    first rows, ``bias_in_margin`` False leaves the bias out of the margins,
    ``extra_class`` lets a padded class with margin 0 into the softmax."""
    x, w, wmat = x.double(), w.double(), wmat.double()
    xs = x if x_margin is None else x_margin.double()
    if rows is not None:
        xs, y, w = xs[:rows], y[:rows], w[:rows]
    raw = xs @ wmat[:F]
    if bias_in_margin:
        raw = raw + wmat[F]
    if extra_class:
        raw = torch.cat([raw, torch.zeros(raw.shape[0], 1, dtype=raw.dtype)], 1)
    logp = torch.log_softmax(raw, dim=1)
    yl = y.long().unsqueeze(1)
    loss = -(logp.gather(1, yl).squeeze(1) * w).sum()
    onehot = torch.zeros_like(logp).scatter_(1, yl, 1.0)
    gmat = ((logp.exp() - onehot) * w.unsqueeze(1))[:, :K]
    return torch.cat([loss.reshape(1), (xs.T @ gmat).reshape(-1), gmat.sum(0)])


@pytest.mark.parametrize("colscale", [False, True])
def test_comparator_rejects_planted_faults(colscale):
    x, y, w, wmat = U.inputs(N, F, K, True, 0.05, colscale)
    want, err32 = U.references(x, y, w, wmat, True)
    bound = U.bounds(err32)
    # the undamaged float32 reference stays within the bound by construction,
    # and the fault-free model above is the float64 payload
    assert all(err32[p] <= bound[p] for p in U.PARTS)
    clean = U.errors(_payload(x, y, w, wmat), want, x, w, K)
    assert all(clean[p] <= 1e-12 for p in U.PARTS), clean

    swapped = x.clone()
    swapped[:, [0, 1]] = x[:, [1, 0]]  # inside tile 0, the smallest columns
    zeroed = want.clone()
    zeroed[1:].view(F + 1, K)[0:4, 0:16] = 0.0  # features 0..3, classes 0..15
    damaged = {
        "last row dropped": _payload(x, y, w, wmat, rows=N - 1),
        "two features swapped": _payload(x, y, w, wmat, x_margin=swapped),
        "bias left out of the margins": _payload(x, y, w, wmat,
                                                 bias_in_margin=False),
        "one 4x16 accumulator block zero": zeroed,
        "padded class in the softmax": _payload(x, y, w, wmat,
                                                extra_class=True),
    }
    for name, got in damaged.items():
        err = U.errors(got, want, x, w, K)
        print(f"colscale {colscale}, {name}: " + ", ".join(
            f"{p} {err[p]:.2e} (bound {bound[p]:.2e})" for p in U.PARTS))
        assert any(err[p] > bound[p] for p in U.PARTS), (name, err, bound)
    # every fault here damages the gradient, which is where a normaliser
    # taken over the whole payload would hide it
    for name, got in damaged.items():
        assert U.errors(got, want, x, w, K)["grad"] > bound["grad"], name

    if colscale:
        # the same zeroed block under one largest-entry normaliser, as the
        # first wide-kernel test had it, passes as clean
        def global_max(p):
            return float((p[1:] - want[1:]).abs().max() / want[1:].abs().max())

        ref32 = U.reference.logreg_loss_grad(x, y, w, wmat, True).double()
        assert global_max(zeroed) <= 16 * global_max(ref32)


def test_zero_denominator_entries_must_be_zero():
    x, y, w, wmat = U.inputs(N, F, K, True, 0.05)
    w0 = torch.zeros_like(w)
    want, _ = U.references(x, y, w0, wmat, True)
    assert U.errors(want, want, x, w0, K) == {"loss": 0.0, "grad": 0.0, "bias": 0.0}
    bad = want.clone()
    bad[5] = 1e-30
    assert U.errors(bad, want, x, w0, K)["grad"] == float("inf")
