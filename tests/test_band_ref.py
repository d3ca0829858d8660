"""CPU: tests/_band_ref.py, the yardstick of the band-limited sampler's tests, against tests/_sampler_ref.py — a single rung and whole levels
reproduce it exactly, the level decoding at its edges, the blend's definitions — and the anti-aliasing claim on the yardstick alone: at a step
of 2 the automatic level removes a tone above the new Nyquist that the full-band bank returns aliased at full level, and keeps one below."""
import numpy as np
import pytest

import _band_ref as BR
import _oracle as O
import _sampler_ref as S

DEFAULT = (1.0, 2 ** -0.5, 0.5, 2 ** -1.5, 0.25)


def flags():
    return O.BH | O.INTERP | O.LOWPASS


def case(seed=3, N=90, M=70, Cn=2):
    rng = np.random.default_rng(seed)
    x = 0.25 * rng.standard_normal((Cn, N))
    p = np.sort(rng.uniform(-12.0, N + 12.0, M))
    p[:3] = [-np.inf, -30.0, np.nan]                              # (no window)
    gy = rng.standard_normal((Cn, M))
    return x, p, gy


def test_decode_at_the_edges():
    K = 4
    l = np.array([-np.inf, -1.0, -0.0, 0.0, 2.0 ** -60, 1 - 2.0 ** -53, 1.0, K - 1 - 2.0 ** -40, K - 1.0, float(K), np.inf, np.nan, 1.25])
    L, lam, moves = BR.decode(l, K)
    assert L.tolist() == [0, 0, 0, 0, 0, 0, 1, K - 2, K - 1, K - 1, K - 1, 0, 1]
    assert lam.tolist() == [0, 0, 0, 0, 2.0 ** -60, 1 - 2.0 ** -53, 0, 1 - 2.0 ** -40, 0, 0, 0, 0, 0.25]
    assert moves.tolist() == [False, False, True, True, True, True, True, True, True, False, False, False, True]
    L, lam, moves = BR.decode(l, 1)
    assert not L.any() and not lam.any() and not moves.any()


@pytest.mark.parametrize("width", [32, 64])
def test_a_single_rung_and_whole_levels_are_the_sampler_yardstick(width):
    T = F = 16
    x, p, gy = case()
    rungs = BR.ladder((1.0, 0.6, 0.3), flags())
    assert rungs[0] == (0.0, flags() & ~O.LOWPASS) and rungs[1] == (0.6, flags())
    names = ("ys", "scale", "D", "slope_scale", "gp", "gp_scale", "A", "gx", "gx_scale", "entries")
    for k, (lp, fl) in enumerate(rungs):
        want = S.sample(T, F, lp, fl, x, p, gy, width, operator=True)
        for levels in (np.full(len(p), -3.0), np.full(len(p), np.nan), np.linspace(0.0, 5.0, len(p))):     # K = 1: any level
            got = BR.sample(T, F, [rungs[k]], x, p, levels, gy, width, operator=True)
            assert all(np.array_equal(getattr(got, n), getattr(want, n)) for n in names)
            assert not got.gl.any() and not got.moves.any()
        got = BR.sample(T, F, rungs, x, p, np.full(len(p), float(k)), gy, width, operator=True)
        assert all(np.array_equal(getattr(got, n), getattr(want, n)) for n in names), k
    # mixed whole levels: output m is rung L [m]'s
    levels = np.arange(len(p)) % 5 - 1.0                           # (-1 .. 3: below the ladder, on it, above it)
    got = BR.sample(T, F, rungs, x, p, levels, gy, width)
    assert got.L.tolist() == np.clip(levels, 0, 2).astype(int).tolist() and not got.lam.any()
    for k in range(3):
        assert np.array_equal(got.ys[:, got.L == k], got.rung[k].ys[:, got.L == k]) and np.array_equal(got.gp[got.L == k], got.rung[k].gp[got.L == k])
    assert np.all(got.gl[(levels < 0) | (levels > 2) | ~got.live] == 0) and np.any(got.gl != 0)
    # the closed ends pass the gradient: the difference of the end's cell
    at_top = (levels == 2) & got.live
    assert np.array_equal(got.gl[at_top], ((got.rung[2].ys - got.rung[1].ys) * np.where(got.live, gy, 0.0)).sum(0)[at_top])


def test_between_rungs_the_blend_is_linear_in_the_level():
    T = F = 16
    x, p, gy = case(5)
    rungs = BR.ladder((1.0, 0.5), flags())
    lo, mid, hi = (BR.sample(T, F, rungs, x, p, np.full(len(p), l), gy, operator=True) for l in (0.0, 0.375, 1.0))
    assert np.allclose(mid.ys, 0.625 * lo.ys + 0.375 * hi.ys, rtol=0, atol=1e-15)
    assert np.allclose(mid.A, 0.625 * lo.A + 0.375 * hi.A, rtol=0, atol=1e-15)
    assert np.allclose(mid.gl, (np.where(mid.live, gy, 0.0) * (hi.ys - lo.ys)).sum(0), rtol=0, atol=1e-15)
    assert np.array_equal(mid.gl, lo.gl) and np.array_equal(mid.gl, hi.gl)         # (one cell: one slope in the level, ends included)
    assert np.allclose(mid.gx, (np.where(mid.live, gy, 0.0)) @ mid.A) and np.allclose((mid.gx * x).sum(), (np.where(mid.live, gy, 0.0) * mid.ys).sum())


def test_the_automatic_level_removes_what_would_alias_and_keeps_what_would_not():
    T = F = 64
    N, M = 600, 300
    n = np.arange(N)
    p = 2.0 * np.arange(M)
    rungs = BR.ladder(DEFAULT, flags())
    levels = BR.auto_levels(p, M, DEFAULT)
    assert np.all(levels == 2.0)
    rms = lambda v: float(np.sqrt(np.mean(v[0, T:M - T] ** 2)))
    for tone, kept in ((0.75, False), (0.3, True)):
        x = 0.5 * np.cos(np.pi * tone * n)[None, :]
        per_rung = [S.sample(T, F, lp, fl, x, p) for lp, fl in rungs]
        full = rms(BR.sample(T, F, rungs, x, p, np.zeros(M), per_rung=per_rung).ys)
        banded = rms(BR.sample(T, F, rungs, x, p, levels, per_rung=per_rung).ys)
        print("tone", tone, "full band rms", full, "automatic levels rms", banded, "ratio", banded / full)
        assert abs(full - 0.5 / np.sqrt(2)) < 1e-3                # (the full-band bank passes both: the upper one aliased)
        assert abs(banded / full - 1.0) <= 1e-3 if kept else banded <= 1e-3 * full
    # at a step of 1.5 the level falls between two rungs: the blend still takes most of the tone away
    p15 = 1.5 * np.arange(M)
    l15 = BR.auto_levels(p15, M, DEFAULT)
    assert np.all(np.abs(l15 - 2 * np.log2(1.5)) < 1e-12)
    x = 0.5 * np.cos(np.pi * 0.75 * n)[None, :]
    ratio = rms(BR.sample(T, F, rungs, x, p15, l15).ys) / rms(BR.sample(T, F, rungs, x, p15, np.zeros(M)).ys)
    print("step 1.5, level", l15[5], "ratio", ratio)
    assert 0.0 < ratio < 0.2
