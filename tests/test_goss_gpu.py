"""``goss_weights`` on the GPU (csrc/goss.hip) against
``reference.goss_weights``.

Both compute the same f32 key, the same stable top-k and the same integer
draw, so every comparison is ``torch.equal``: there are no tolerances.  Row
counts come from ``goss_geometry``: the wave, the tile and one grid round."""

import pytest
import torch

from spark_ensemble_amd.ops import dispatch as ops
from spark_ensemble_amd.ops import reference
from test_goss import RATES, check_one_round

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = ["1", "63", "64", "65", "tile-1", "tile+1", "round+1"]


def rows(size):
    geo = ops.goss_geometry(1)
    tile = geo["tile_rows"]
    return {"tile-1": tile - 1, "tile+1": tile + 1,
            "round+1": geo["max_blocks"] * tile + 1}.get(size) or int(size)


def check(g, w, top, other, seed=3, rank=1):
    want = reference.goss_weights(g, w, top, other, seed, rank)
    got = ops.goss_weights(g.to(DEV), w.to(DEV), top, other, seed, rank)
    assert torch.equal(got.cpu(), want)
    return want


@pytest.mark.parametrize("top,other", RATES)
@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_matches_reference(size, d, unit, top, other):
    n = rows(size)
    gen = torch.Generator().manual_seed(n + d)
    # gradients on a 1/64 grid: tie groups at every threshold
    g = (torch.randn(n, d, generator=gen) * 64).round() / 64
    w = torch.ones(n) if unit else torch.tensor([0.0, 0.5, 1.0, 3.0])[
        torch.randint(0, 4, (n,), generator=gen)]
    check(g, w, top, other)


def from_bits(bits):
    return bits.to(torch.int32).view(torch.float32).unsqueeze(1)


@pytest.mark.parametrize("case", ["equal", "zero", "low_digit", "mid_digit",
                                  "straddle", "nan_inf"])
def test_crafted_keys(case):
    geo = ops.goss_geometry(1)
    tile, (b0, b1, b2) = geo["tile_rows"], geo["digit_bits"]
    n = 3 * tile + 77
    gen = torch.Generator().manual_seed(1)
    w = torch.ones(n)
    top, other = 0.2, 0.1
    one = 0x3F800000
    if case == "equal":
        g = torch.full((n, 1), 0.75)
    elif case == "zero":
        g = torch.zeros(n, 1)
    elif case == "low_digit":
        g = from_bits(one | torch.randint(0, 1 << b2, (n,), generator=gen))
    elif case == "mid_digit":
        g = from_bits(
            one | (torch.randint(0, 1 << b1, (n,), generator=gen) << b2))
    elif case == "straddle":
        # 3 rows above a tie group of 10 that lies 5 + 5 across the first
        # tile boundary; k = 10 keeps the first 7 of the group
        g = torch.rand(n, 1, generator=gen)
        g[[7, tile + 40, 2 * tile + 9]] = 5.0
        g[tile - 5:tile + 5] = 2.0
        top = 9.5 / n
    else:
        g = torch.randn(n, 1, generator=gen)
        g[tile + 3], g[5] = float("nan"), float("inf")
    want = check(g, w, top, other)
    if case == "straddle":
        assert want[tile - 5:tile + 2].eq(1).all() and want.eq(1).sum() == 10
    if case == "nan_inf":
        assert want[tile + 3] == 1 and want[5] == 1


def test_one_round_fit_gpu():
    check_one_round(DEV)
