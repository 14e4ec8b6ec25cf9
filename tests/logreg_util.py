"""Helpers shared by the logistic loss+gradient tests (tests/test_logreg_plan.py,
tests/test_logreg_wide_gpu.py, tests/test_logreg_narrow_gpu.py): seeded
inputs, and one comparison of a payload with reference.logreg_loss_grad on
float64 inputs on the CPU.

Every payload entry has its own denominator, so an error confined to a
low-magnitude column or to the bias row cannot hide under the scale of the
other columns:

  loss            |float64 loss|
  grad[f][c]      D_f = sum_i |w_i * x_if|   (|p - onehot| <= 1 bounds the entry)
  grad_bias[c]    sum_i |w_i|

An entry whose denominator is 0 has to be exactly 0.  The error of a part is
the largest |got - want| / D over its entries.

The bound is the project's yardstick: 16x the error of
reference.logreg_loss_grad on the float32 inputs, with a floor of 16 * 2^-24
(the same factor on one float32 unit roundoff) for inputs where the float32
reference happens to be exact, such as a single row.
"""

import functools

import torch

from spark_ensemble_amd.ops import reference

FACTOR = 16.0
FLOOR = FACTOR * 2.0 ** -24
PARTS = ("loss", "grad", "bias")


def column_scales(f):
    """10^-3 .. 10^3, constant over each group of four features, so every
    16-feature tile holds several scales and features 0..3 the smallest."""
    return 10.0 ** ((torch.arange(f) // 4 % 7) - 3).double()


@functools.lru_cache(maxsize=None)
def inputs(n, f, k, bias, scale, colscale=False):
    """Seeded float32 (x, y, w, wmat) on the CPU; callers must not write to
    them.  ``colscale`` scales the columns of x by column_scales and the rows
    of wmat inversely, so the margins stay as they were."""
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, f, generator=g)
    y = torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
    w = torch.rand(n, generator=g)
    wmat = torch.randn(f + (1 if bias else 0), k, generator=g) * scale
    if colscale:
        cs = column_scales(f).float()
        x = x * cs
        wmat = wmat.clone()
        wmat[:f] /= cs.unsqueeze(1)
    return x, y, w, wmat


def denominators(x, w):
    """D_f [F] and the bias denominator; the loss has the float64 loss."""
    x, w = x.double(), w.double()
    return (w.abs().unsqueeze(1) * x.abs()).sum(dim=0), w.abs().sum()


def errors(got, want, x, w, k):
    """{"loss", "grad", "bias"}: largest |got - want| / D of each part of the
    payload ``got`` against the float64 payload ``want``; inf where an entry
    with denominator 0 is not exactly 0."""
    f = x.shape[1]
    got = got.detach().cpu().double()
    assert got.shape == want.shape == (1 + (f + 1) * k,)
    d_f, d_b = denominators(x, w)
    den = torch.cat([want[:1].abs(), d_f.repeat_interleave(k),
                     d_b.expand(k)])
    inf = torch.full_like(den, float("inf"))
    rel = torch.where(den > 0, (got - want).abs() / den.clamp_min(1e-300),
                      torch.where(got == 0, torch.zeros_like(den), inf))
    rel = torch.where(torch.isfinite(got), rel, inf)
    return {"loss": float(rel[0]), "grad": float(rel[1:1 + f * k].max()),
            "bias": float(rel[1 + f * k:].max())}


def references(x, y, w, wmat, bias):
    """(float64 payload, errors of the float32 reference against it)."""
    k = wmat.shape[1]
    want = reference.logreg_loss_grad(x.double(), y, w.double(), wmat.double(),
                                      bias)
    err32 = errors(reference.logreg_loss_grad(x, y, w, wmat, bias), want, x, w, k)
    return want, err32


def bounds(err32):
    return {p: max(FACTOR * err32[p], FLOOR) for p in PARTS}


def check(tag, got, x, y, w, wmat, bias):
    """Print and assert the errors of the payload ``got`` of the float32 CPU
    inputs; returns (errors, float32-reference errors)."""
    k = wmat.shape[1]
    want, err32 = references(x, y, w, wmat, bias)
    err = errors(got, want, x, w, k)
    print(f"{tag} {x.shape[0]}x{x.shape[1]}x{k}: " + ", ".join(
        f"{p} {err[p]:.2e} (f32 torch {err32[p]:.2e})" for p in PARTS))
    bound = bounds(err32)
    for p in PARTS:
        assert err[p] <= bound[p], (tag, p, err[p], bound[p])
    return err, err32
