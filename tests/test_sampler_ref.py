"""CPU: the clip sampler's yardstick (tests/_sampler_ref.py) held to the strict oracle, through the yardsticks that already are.

At p = off - T, off the positions of a tests/_rate_grad_ref.py replay of a one-block clip (a ring whose index T holds frame 0), the sampler
is the clip entries' interpolator.  For one phase in one ring segment off - T is exact in fp64 and keeps floor and frac, so
(a) cell, ys, scale and D are that module's values, and ys is the oracle's own forward within the bound tests/test_rate_grad_ref.py uses;
(b) the weight matrix A is tests/_adjoint_ref.py's dense operator (one unit impulse per frame through the oracle) at the same positions —
    interpolating, nearest filter and pass-through.
The clips stay within one ring segment per phase: asserted through artamdPlanCall."""
import ctypes as C

import numpy as np
import pytest

import audio_resampler_amd as A
from audio_resampler_amd.api import ArtamdPosition, ArtamdSegment, ResampleResult
import _adjoint_ref as AR
import _oracle as O
import _rate_grad_ref as R
import _sampler_ref as S

BH, IN, LP = O.BH, O.INTERP, O.LOWPASS
SHAPES = [(8, 4), (16, 16), (32, 7)]
RATIOS = [0.37, 1.0, 48000 / 44100, 2.5, 1.3071]


def one_segment_per_phase(taps, filters, flags, frames, ratio):
    """the process call and the flush of a fresh context's clip, planned: (segments of each, outputs of each)"""
    pos = ArtamdPosition(taps, filters, flags, taps, 0, float(taps // 2), 0.0)
    res, segs, floor = ResampleResult(), (ArtamdSegment * 8)(), C.c_int()
    plan = A.lib().artamdPlanCall
    first = plan(C.byref(pos), frames, 2 ** 30, ratio, C.byref(res), segs, 8, C.byref(floor))
    made = [res.output_generated]
    second = plan(C.byref(pos), -1, 2 ** 30, ratio, C.byref(res), segs, 8, C.byref(floor))
    return (first, second), made + [res.output_generated]


@pytest.mark.parametrize("ratio", RATIOS, ids=str)
@pytest.mark.parametrize("lowpass", [0.0, 0.45])
@pytest.mark.parametrize("taps,filters", SHAPES)
def test_at_the_clip_entries_positions_the_sampler_is_their_interpolator(taps, filters, lowpass, ratio):
    flags = BH | IN | (LP if lowpass else 0)
    N = 10 * taps
    x = 0.25 * np.random.default_rng(taps + filters).standard_normal((2, N))
    ref = [R.clip(taps, filters, lowpass, flags, (N,), (ratio,), x[c]) for c in range(2)]
    nseg, made = one_segment_per_phase(taps, filters, flags, N, ratio)
    assert nseg == (1, 1) and made == ref[0].counts, (nseg, made, ref[0].counts)
    p = S.aligned_positions(ref[0].counts, (ratio,), taps)
    assert len(p) == sum(made) > N * ratio
    for c in range(2):                                            # (a channel at a time, as that module is asked: numpy's sums then run alike)
        got = S.sample(taps, filters, lowpass, flags, x[c], p)
        assert got.live.all() and np.array_equal(got.cell + taps * filters, ref[c].cell) and np.array_equal(got.first, ref[c].ip)
        assert np.array_equal(got.ys, ref[c].ys) and np.array_equal(got.scale, ref[c].scale) and np.array_equal(got.D, ref[c].D)
        _, y = R.replay(taps, filters, lowpass, flags, (N,), (ratio,), x[c])
        err = np.abs(got.ys[0] - y)
        assert np.abs(y).max() > 0.01 and np.all(err <= 8 * 2.0 ** -53 * got.scale[0]), float((err / np.maximum(got.scale[0], 1e-300)).max())


KINDS = [("interpolating", BH | IN | LP, 0.45), ("interpolating-no-lowpass", BH | IN, 0.0), ("nearest-filter", BH | LP, 0.45), ("pass-through", BH, 0.0)]


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("ratio", [0.37, 1.0, 1.5, 48000 / 44100], ids=str)
@pytest.mark.parametrize("name,flags,lowpass", KINDS, ids=[k[0] for k in KINDS])
def test_weights_are_the_rows_of_the_oracles_operator(name, flags, lowpass, ratio, width):
    taps, filters, N = 16, 16, 48
    dense = AR.dense_operator(taps, filters, flags, N, ratio=ratio, lowpass_ratio=lowpass, width=width)
    nseg, made = one_segment_per_phase(taps, filters, flags, N, ratio)
    assert nseg == (1, 1) and sum(made) == dense.shape[0]
    p = S.aligned_positions(made, (ratio,), taps)
    got = S.sample(taps, filters, lowpass, flags, np.zeros((1, N)), p, width=width, operator=True)
    zero = dense == 0
    print(name, ratio, width, "non-zero entries", int((~zero).sum()), "entries that differ", int((got.A != dense).sum()))
    assert (~zero).sum() >= N and np.array_equal(got.A == 0, zero)
    assert np.all(np.abs(got.A - dense) <= np.where(zero, 0.0, AR.ulp_of(dense, width)))
    if name == "pass-through" and ratio in (1.0, 1.5):
        assert any(np.count_nonzero(row) == 1 and row.max() == 1.0 for row in got.A)


def test_positions_without_a_window_and_the_rounded_up_fraction():
    taps, filters, N = 8, 4, 20
    x = np.arange(1.0, N + 1.0)[None, :]
    half = taps // 2
    p = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, -(half + 1) - 2.0 ** -40, -(half + 1), N + half - 2.0 ** -40, N + half, -1e-30, 0.0, 3.25])
    got = S.sample(taps, filters, 0.0, BH | IN, x, p, gy=np.ones((1, len(p))), operator=True)
    assert got.live.tolist() == [False] * 6 + [True, True, False, True, True, True]
    assert np.all(got.ys[0, ~got.live] == 0) and np.all(got.gp[~got.live] == 0) and not got.A[~got.live].any()
    assert got.fi[9] == filters - 1 and got.frac[9] == 1.0 and got.cell[9] == -1 and got.cell[10] == 0 and got.cell[11] == 3 * filters + 1
    assert np.all(np.isfinite(got.ys)) and np.all(got.ys[0, 9:] != 0)
