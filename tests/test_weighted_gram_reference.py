"""CPU test of reference.weighted_gram: the blocks of G against the normal
equations LinearRegression builds from the same rows."""

import pytest
import torch


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n,f", [(1, 1), (50, 3), (333, 17)])
def test_blocks_of_weighted_gram(n, f, dtype):
    from spark_ensemble_amd.ops import dispatch, reference

    g = torch.Generator().manual_seed(n + f)
    x = torch.randn(n, f, generator=g, dtype=dtype)
    y = torch.randn(n, generator=g, dtype=dtype)
    w = torch.rand(n, generator=g, dtype=dtype) - 0.25  # some negative
    w[::7] = 0.0
    G = reference.weighted_gram(x, y, w)
    assert G.shape == (f + 2, f + 2) and G.dtype == dtype
    xa = torch.cat([x, torch.ones(n, 1, dtype=dtype)], dim=1)
    xw = xa * w.unsqueeze(1)
    tol = dict(rtol=0, atol=float(torch.finfo(dtype).eps * 64 * G.abs().max()))
    torch.testing.assert_close(G[:f + 1, :f + 1], xw.T @ xa, **tol)
    torch.testing.assert_close(G[:f + 1, f + 1], xw.T @ y, **tol)
    torch.testing.assert_close(G[f, f], w.sum(), **tol)
    torch.testing.assert_close(G[f + 1, f + 1], (w * y * y).sum(), **tol)
    # on the CPU the dispatcher is the reference, and declines native_only
    assert torch.equal(dispatch.weighted_gram(x, y, w), G)
    assert dispatch.weighted_gram(x, y, w, native_only=True) is None
    assert dispatch.last_weighted_gram_info["path"] == "reference"
