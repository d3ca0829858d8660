"""CPU: the ratio gradient's yardstick (tests/_rate_grad_ref.py) held to the strict 8-byte oracle.

(a) its forward is the oracle's, per output within 8 * 2^-53 * sum |b x|;
(b) its gradient is the central difference of the oracle's own sum (g y) in every r_k, h = 2^-20, within 1e-7 of sum |g D| — under the
    condition, asserted, that at r +- h no phase's output count changes and no output changes its interpolation cell.  This holds the
    carry into the later blocks and the flush's share.  Worst seen over the shapes below: 7.8e-10 of sum |g D|;
(c) the kink: at ratios whose outputs land on filter boundaries the gradient of block 0 is NOT the central difference (seen: 0.65 % and
    1.5 % of sum |g D| away) but the one-sided difference on the side of the cell that floor picks."""
import numpy as np
import pytest

import _oracle as O
import _rate_grad_ref as R

BH, IN, LP = O.BH, O.INTERP, O.LOWPASS
H = 2.0 ** -20
SHAPES = [(16, 16, 0.0, BH | IN), (16, 16, 0.45, BH | IN | LP), (32, 8, 0.0, BH | IN), (32, 8, 0.45, BH | IN | LP)]
BLOCKS = [(16, 16, 9), (10,) * 5, (7,)]
SMOOTH = (1.1037, 0.8213, 1.3071, 0.9371, 1.2113)
KINKED = [(1.1, 0.8, 1.3), (0.6, 1.7, 0.9)]


def signal(blocks, seed):
    rng = np.random.default_rng(seed)
    return 0.25 * rng.standard_normal(int(sum(blocks)))


def loss(shape, blocks, ratios, x, g):
    counts, y = R.replay(*shape, blocks, ratios, x)
    return counts, float((g * y).sum()) if len(y) == len(g) else None


@pytest.mark.parametrize("blocks", BLOCKS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_forward_is_the_oracles(shape, blocks):
    ratios = SMOOTH[:len(blocks)]
    x = signal(blocks, 3)
    ref = R.clip(*shape, blocks, ratios, x)
    counts, y = R.replay(*shape, blocks, ratios, x)
    assert counts == ref.counts and len(y) == ref.ys.shape[1] and np.abs(y).max() > 0.01
    err = np.abs(ref.ys[0] - y)
    print(shape, blocks, "worst absolute error", err.max(), "worst error / bound", (err / np.maximum(8 * 2.0 ** -53 * ref.scale[0], 1e-300)).max())
    assert np.all(err <= 8 * 2.0 ** -53 * ref.scale[0])


def condition(shape, blocks, ratios, x, k):
    """at r_k +- h: the same counts, and every output in the same interpolation cell"""
    lo, hi = list(ratios), list(ratios)
    lo[k] -= H; hi[k] += H
    a, b, mid = R.clip(*shape, blocks, lo, x), R.clip(*shape, blocks, hi, x), R.clip(*shape, blocks, ratios, x)
    return a.counts == b.counts == mid.counts and np.array_equal(a.cell, b.cell), lo, hi


@pytest.mark.parametrize("blocks", BLOCKS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gradient_is_the_oracles_central_difference(shape, blocks):
    ratios = SMOOTH[:len(blocks)]
    x = signal(blocks, 5)
    M = sum(R.replay(*shape, blocks, ratios)[0])
    g = np.random.default_rng(7).standard_normal(M)
    ref = R.clip(*shape, blocks, ratios, x, g)
    assert ref.gd > 0
    for k in range(len(blocks)):
        ok, lo, hi = condition(shape, blocks, ratios, x, k)
        assert ok, ("the ratios put an output on a cell boundary within h", k)
        fd = (loss(shape, blocks, hi, x, g)[1] - loss(shape, blocks, lo, x, g)[1]) / (2 * H)
        print(shape, blocks, "block", k, "analytic", ref.grad[k], "central", fd, "difference / sum |g D|", abs(fd - ref.grad[k]) / ref.gd)
        assert abs(fd - ref.grad[k]) <= 1e-7 * ref.gd


@pytest.mark.parametrize("ratios", KINKED, ids=str)
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_on_a_filter_boundary_the_gradient_is_the_slope_of_the_cell_floor_picks(shape, ratios):
    blocks = (16, 16, 9)
    x = signal(blocks, 5)
    counts, y = R.replay(*shape, blocks, ratios, x)
    g = np.random.default_rng(7).standard_normal(len(y))
    ref = R.clip(*shape, blocks, ratios, x, g)
    lo, hi = list(ratios), list(ratios)
    lo[0] -= H; hi[0] += H
    (c_lo, l_lo), (c_hi, l_hi), (_, l_mid) = loss(shape, blocks, lo, x, g), loss(shape, blocks, hi, x, g), loss(shape, blocks, ratios, x, g)
    assert c_lo == c_hi == counts
    central, below, above = (l_hi - l_lo) / (2 * H), (l_mid - l_lo) / H, (l_hi - l_mid) / H
    # a one-sided difference also carries the curvature of n / r: h / 2 * |d2L/dr2| <= h * max (n) / min (r)^3 * sum |g D|
    slack = (1e-7 + H * ref.n.max() / min(ratios) ** 3) * ref.gd
    off = [abs(v - ref.grad[0]) / ref.gd for v in (central, below, above)]
    print(shape, ratios, "block 0: analytic", ref.grad[0], "distance / sum |g D| to central, from below, from above", off)
    assert off[0] > 1e-3, "no output of block 0 on a filter boundary?"
    assert min(off[1], off[2]) * ref.gd <= slack
    # the side: raising r_0 lowers every later position, so the cell floor picks (the one above a boundary) is the one r_0 - h stays in
    assert off[1] < off[2]
