"""artamdLagProductsBatchDevice on the GPU, both widths: every sum against an exact reference within a derived bound, at every frame
count where the kernel takes another path (single accesses only, one 16-byte group, both sides of a pass and of a tile, several
tiles) and every base offset of either row; a row's bits do not depend on its company, its place, its alignment or the stream; and
the refusals change nothing.

The reference: the 4-byte build's products are exact in double, the 8-byte build's are exactly rounded (numpy's product), and
math.fsum adds them without error.  The bound is m * 2^-52 * sum |u[t] v[t-k]| for m terms: twice the first-order bound
(m - 1) * 2^-53 * sum |terms| of adding m doubles in ANY order, which leaves room for the one rounding of each product in the
8-byte build (2^-53 * sum |terms|)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import audio_resampler_amd as A

pytestmark = pytest.mark.gpu

FILL = -777.25
LAGS = [(0, 5), (1, 4), (0, 1), (3, 5)]
PAD = 3                                         # sentinel doubles on either side of a row's sums


def _tile(M):
    fn = M.lib().artamd_lag_products_tile
    fn.restype, fn.argtypes = C.c_int, []
    return fn()


def _np(M):
    return np.float64 if M.width == 64 else np.float32


def _frame_counts(M):
    t = _tile(M)
    return [1, 2, 4, 5, 8, 63, 64, 65, t - 1, t, t + 1, 2 * t + 5]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


class Row:
    """u and v of one row on the device, each `offset` samples behind a 16-byte boundary, between sentinels"""
    def __init__(self, M, u, v, ou, ov):
        self.hu, self.hv, self.n = u, v, len(u)
        dt = torch.float64 if M.width == 64 else torch.float32
        q = 16 // (M.width // 8)
        self.bu = torch.full((q + ou + self.n + 5,), 12345.5, dtype=dt, device="cuda")
        self.bv = torch.full((q + ov + self.n + 5,), 12345.5, dtype=dt, device="cuda")
        assert self.bu.data_ptr() % 16 == 0 and self.bv.data_ptr() % 16 == 0
        self.u, self.v = self.bu[q + ou:q + ou + self.n], self.bv[q + ov:q + ov + self.n]
        self.u.copy_(torch.from_numpy(u)); self.v.copy_(torch.from_numpy(v))


def _want(u, v, n, first, lags):
    """[(exact sum, sum of |terms|, number of terms)] per lag of the row"""
    out = []
    for k in range(first, first + lags):
        if k >= n:
            out.append((0.0, 0.0, 0))
            continue
        terms = u[k:n].astype(np.float64) * v[:n - k].astype(np.float64)
        out.append((math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist()), n - k))
    return out


def _call(M, rows, specs, stream=None, sums=None):
    """rows [Row], specs [(frames, first, lags)] -> (rc, sums [n, PAD + 8 + PAD] on the host)"""
    n = len(rows)
    if sums is None:
        sums = torch.full((n, PAD + 8 + PAD), FILL, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    rc = M.lag_products_batch_device([r.u.data_ptr() for r in rows], [r.v.data_ptr() for r in rows], [s[0] for s in specs],
                                     [s[1] for s in specs], [s[2] for s in specs],
                                     [sums.data_ptr() + 8 * (i * sums.shape[1] + PAD) for i in range(n)], stream=stream)
    torch.cuda.synchronize()
    return rc, sums.cpu().numpy()


# ---- 1. against an exact reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_sums_against_an_exact_reference_at_every_length_offset_and_lag_range(width):
    M = A.binding(width)
    rng = np.random.default_rng(2100 + width)
    rows, specs = [], []
    for n in _frame_counts(M):
        for first, lags in LAGS:
            for ou in range(4):
                for ov in range(4):
                    u, v = (rng.uniform(-1, 1, n).astype(_np(M)) for _ in range(2))
                    rows.append(Row(M, u, v, ou, ov)); specs.append((n, first, lags))
            # a row without frames in the middle of the list: anything in its place, its sums keep the fill value
            rows.append(rows[-1]); specs.append((0 if first else -2, first, lags))
    assert any(n <= first for n, first, _ in specs if n > 0)        # rows whose every lag is past their end: all zero
    rc, got = _call(M, rows, specs)
    assert rc == 2                                                   # the tiles' launch and the finishing one, whatever the rows
    fill = _bits(np.float64(FILL))
    for i, (r, (n, first, lags)) in enumerate(zip(rows, specs)):
        if n <= 0:
            assert np.all(_bits(got[i]) == fill), (i, n)
            continue
        assert np.all(_bits(got[i, :PAD]) == fill) and np.all(_bits(got[i, PAD + lags:]) == fill), (i, n, first, lags)
        for q, (want, mass, m) in enumerate(_want(r.hu, r.hv, n, first, lags)):
            g = float(got[i, PAD + q])
            if m == 0:
                assert g == 0.0, (i, n, first, q)
            else:
                assert abs(g - want) <= m * 2.0 ** -52 * mass, (i, n, first + q, g, want, abs(g - want), m * 2.0 ** -52 * mass)
    for r in rows:                                                   # the rows are only read
        assert torch.equal(r.u.cpu(), torch.from_numpy(r.hu)) and torch.equal(r.v.cpu(), torch.from_numpy(r.hv))
        assert bool((r.bu[-5:] == 12345.5).all()) and bool((r.bv[-5:] == 12345.5).all())


def test_neighbours_that_are_not_finite_stay_out_of_the_sums():
    """the frames before a row and at and past its end are not read into any term: NaN and infinity there leave the sums finite"""
    M = A.binding(32)
    t = _tile(M)
    rng = np.random.default_rng(7)
    for n in (5, 65, t + 3):
        full_u, full_v = (rng.uniform(-1, 1, n + 16).astype(np.float32) for _ in range(2))
        full_u[n:], full_v[n:] = np.inf, np.nan
        r = Row(M, full_u, full_v, 1, 2)
        r.bu[:4 + 1] = float("nan"); r.bv[:4 + 2] = float("inf")
        rc, got = _call(M, [r], [(n, 0, 8)])
        assert rc == 2
        for q, (want, mass, m) in enumerate(_want(full_u, full_v, n, 0, 8)):
            g = float(got[0, PAD + q])
            assert (g == 0.0) if m == 0 else abs(g - want) <= m * 2.0 ** -52 * mass, (n, q, g, want)


# ---- 2. the same row keeps its bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_a_rows_bits_do_not_depend_on_company_place_alignment_or_stream(width):
    M = A.binding(width)
    t = _tile(M)
    rng = np.random.default_rng(3100 + width)
    for n, first, lags in ((2 * t + 5, 0, 5), (t + 1, 3, 5), (65, 1, 4), (700, 0, 8)):
        u, v = (rng.uniform(-1, 1, n).astype(_np(M)) for _ in range(2))
        row = Row(M, u, v, 0, 0)
        rc, alone = _call(M, [row], [(n, first, lags)])
        assert rc == 2
        want = _bits(alone[0, PAD:PAD + lags])
        # first and last in a batch of mixed lengths, and listed twice
        others = [Row(M, *(rng.uniform(-1, 1, m).astype(_np(M)) for _ in range(2)), i % 4, (i + 1) % 4)
                  for i, m in enumerate((1, 3 * t, 63, t - 1, 700))]
        batch = [row] + others + [row]
        spec = [(n, first, lags)] + [(r.n, i % 3, 5) for i, r in enumerate(others)] + [(n, first, lags)]
        rc, got = _call(M, batch, spec)
        assert rc == 2
        assert np.array_equal(_bits(got[0, PAD:PAD + lags]), want) and np.array_equal(_bits(got[-1, PAD:PAD + lags]), want), (n, "batch")
        # every base offset of either row
        moved = [Row(M, u, v, ou, ov) for ou in range(4) for ov in range(4)]
        rc, got = _call(M, moved, [(n, first, lags)] * len(moved))
        for i in range(len(moved)):
            assert np.array_equal(_bits(got[i, PAD:PAD + lags]), want), (n, "offsets", divmod(i, 4))
        # u and v one row (an autocorrelation) is taken, and a non-default stream changes nothing
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            rc, got = _call(M, [others[1], row], [(others[1].n, 0, 5), (n, first, lags)], stream=side)
        assert rc == 2 and np.array_equal(_bits(got[1, PAD:PAD + lags]), want), (n, "stream")
        rc, got = _call(M, [row], [(n, first, lags)], stream=None)      # ... and back on the null stream, the scratch shared
        assert np.array_equal(_bits(got[0, PAD:PAD + lags]), want), (n, "null stream again")


# ---- 3. refusals on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_refusals_on_the_device_change_nothing_and_count_nothing(width):
    M = A.binding(width)
    L = M.lib()
    rng = np.random.default_rng(5)
    good = Row(M, *(rng.uniform(-1, 1, 300).astype(_np(M)) for _ in range(2)), 1, 2)
    sums = torch.full((2, PAD + 8 + PAD), FILL, dtype=torch.float64, device="cuda")
    at = lambda i: sums.data_ptr() + 8 * (i * sums.shape[1] + PAD)
    errors = L.artamdErrorCount()
    up, vp = good.u.data_ptr(), good.v.data_ptr()
    bad = {"NULL u": (None, vp, 300, 0, 5, at(1)), "NULL v": (up, None, 300, 0, 5, at(1)), "NULL sums": (up, vp, 300, 0, 5, None),
           "negative first lag": (up, vp, 300, -1, 5, at(1)), "zero lags": (up, vp, 300, 0, 0, at(1)),
           "first + num > 8": (up, vp, 300, 4, 5, at(1)), "nine lags": (up, vp, 300, 0, 9, at(1))}
    torch.cuda.synchronize()
    for what, row in bad.items():
        for rows in ([(up, vp, 300, 0, 5, at(0)), row], [row, (up, vp, 300, 0, 5, at(0))]):
            n = len(rows)
            col = lambda j, t: (t * n)(*[r[j] for r in rows])
            rc = L.artamdLagProductsBatchDevice(col(0, C.c_void_p), col(1, C.c_void_p), col(2, C.c_int), col(3, C.c_int), col(4, C.c_int),
                                                col(5, C.c_void_p), n, None)
            assert rc == -1, what
    torch.cuda.synchronize()
    assert L.artamdErrorCount() == errors
    assert np.all(_bits(sums.cpu().numpy()) == _bits(np.float64(FILL)))            # the good row of a refused call was not made either
    # the same lists are taken when they are right
    rc, got = _call(M, [good, good], [(300, 0, 5), (300, 4, 4)], sums=sums)
    assert rc == 2 and not np.any(_bits(got[:, PAD:PAD + 4]) == _bits(np.float64(FILL)))
    assert L.artamdErrorCount() == errors
