"""The yardstick of the clip sampler's tests: a clip evaluated at a position curve, restated in float64 from the strict CPU oracle's bank
(OracleResampler.bank ()) alone.

    a position p (in input frames; p = 0 is centred on frame 0) of a clip of N frames: whole = floor (p), fr = (p - whole) F,
    fi = floor (fr) and frac = fr - fi (interpolating), fi = floor (fr + 0.5) and frac = 0 (nearest filter);
    tap t reads input frame whole - half + 1 + t; frames below 0 and at and past N are silence;
    a position that is not finite, below -(half + 1) or at or past N + half has no window: its output is 0 and it has no term anywhere.
    (p - whole rounds up to 1 for a tiny negative p: fi = F is taken as fi = F - 1, frac = 1 — the same value, the cell p lies in.)

    y = s0 (1 - frac) + s1 frac with the dot products of bank rows fi and fi + 1 (the oracle's order: pairs from both ends);
    A [m, j] = (sample type)(h0 (1 - frac) + h1 frac), the weight of tests/_adjoint_ref.py (the single row's tap, or the pass-through's 1);
    D = F sum_t (bank [fi + 1][t] - bank [fi][t]) x [...]: the slope of the cell that floor picks;  gp [m] = sum_c gy [c, m] D [c, m].

tests/test_sampler_ref.py holds this file to the oracle through tests/_rate_grad_ref.py and tests/_adjoint_ref.py.  TEST INFRASTRUCTURE ONLY."""
import types

import numpy as np

import _oracle as O


def bank_of(taps, filters, lowpass, flags, width=64):
    return O.binding(width).OracleResampler(1, taps, filters, lowpass, flags, kind="strict").bank()


def sample(taps, filters, lowpass, flags, x, p, gy=None, width=64, operator=False):
    """x [C, N], p [M], gy [C, M] or None -> a namespace of float64 arrays:
    live [M] (the position has a window), cell [M] (floor (p) F + fi; 0 without a window), first [M] (frame of tap 0), fi, frac [M],
    ys [C, M], scale [C, M] (sum |b x|, lerped), D [C, M], slope_scale [C, M] (F sum |db x|); with operator: A [M, N] (entries exactly
    sample-type values); with gy: gp [M], gp_scale [M] (sum_c |gy| F sum_t |db x|), and with operator gx [C, N], gx_scale [C, N]
    (|A|^T |gy|), entries [N] (non-zero weights per column)"""
    smp = np.float64 if width == 64 else np.float32
    bank = bank_of(taps, filters, lowpass, flags, width).astype(np.float64)
    interp, lowpassed = bool(flags & O.INTERP), bool(flags & O.LOWPASS)
    x = np.atleast_2d(np.asarray(x, np.float64))
    p = np.asarray(p, np.float64)
    Cn, N = x.shape
    M, T, F, half = len(p), taps, filters, taps // 2
    with np.errstate(invalid="ignore"):
        live = np.isfinite(p) & (p >= -(half + 1)) & (p < N + half)
    q = np.where(live, p, 0.0)
    whole = np.floor(q)
    fr = (q - whole) * F
    if interp:
        fi = np.floor(fr).astype(np.int64)
        frac = fr - fi
        up = fi >= F
        fi, frac = np.where(up, F - 1, fi), np.where(up, 1.0, frac)
    else:
        fi = np.floor(fr + 0.5).astype(np.int64)
        frac = np.zeros(M)
    first = whole.astype(np.int64) - half + 1
    taps_at = first[:, None] + np.arange(T)[None, :]                # [M, T]
    ok = live[:, None] & (taps_at >= 0) & (taps_at < N)
    win = np.where(ok[None], x[:, np.clip(taps_at, 0, max(N - 1, 0))], 0.0) if N else np.zeros((Cn, M, T))      # [C, M, T]
    lo, hi = bank[fi], bank[np.minimum(fi + 1, F)]                 # [M, T]
    passing = (not interp) and (not lowpassed)
    passes = live & (fi % F == 0) if passing else np.zeros(M, bool)
    tap_of_pass = half - 1 + fi // F

    def dot(rows):                                                 # the oracle's order: pairs from both ends towards the middle
        acc = np.zeros(win.shape[:2])
        for a, b in zip(range(T // 2), range(T - 1, T // 2 - 1, -1)):
            acc = acc + (rows[None, :, a] * win[:, :, a] + rows[None, :, b] * win[:, :, b])
        return acc

    if interp:
        ys = dot(lo) * (1.0 - frac) + dot(hi) * frac
        scale = (np.abs(lo)[None] * np.abs(win)).sum(2) * (1.0 - frac) + (np.abs(hi)[None] * np.abs(win)).sum(2) * frac
        D = F * ((hi - lo)[None] * win).sum(2)
        slope_scale = F * (np.abs(hi - lo)[None] * np.abs(win)).sum(2)
    else:
        copied = win[:, np.arange(M), np.clip(tap_of_pass, 0, T - 1)]                     # [C, M]
        ys = np.where(passes[None], copied, dot(lo))
        scale = np.where(passes[None], np.abs(copied), (np.abs(lo)[None] * np.abs(win)).sum(2))
        D, slope_scale = np.zeros((Cn, M)), np.zeros((Cn, M))
    out = types.SimpleNamespace(live=live, cell=np.where(live, whole.astype(np.int64) * F + fi, 0), first=first, fi=fi, frac=frac,
                                ys=ys, scale=scale, D=D, slope_scale=slope_scale)
    if operator:
        if interp:
            W = (lo * (1.0 - frac)[:, None] + hi * frac[:, None]).astype(smp).astype(np.float64)
        else:
            W = np.where(passes[:, None], (np.arange(T)[None, :] == tap_of_pass[:, None]).astype(np.float64), lo)
        A = np.zeros((M, N))
        rows, cols = np.nonzero(ok)
        A[rows, taps_at[rows, cols]] = W[rows, cols]
        out.A = A
    if gy is not None:
        gy = np.atleast_2d(np.asarray(gy, np.float64))
        assert gy.shape == (Cn, M), (gy.shape, (Cn, M))
        g = np.where(live[None], gy, 0.0)                          # (gy of an output without a window is not read: it may be anything)
        out.gp, out.gp_scale = (g * D).sum(0), (np.abs(g) * slope_scale).sum(0)
        if operator:
            out.gx, out.gx_scale, out.entries = g @ out.A, np.abs(g) @ np.abs(out.A), (out.A != 0).sum(axis=0)
    return out


def aligned_positions(counts, ratios, taps):
    """the positions of a clip made block by block (tests/_rate_grad_ref.py's recurrence: counts [K + 1] of a replay, ratios [K]) in the
    sampler's convention: off - taps, off the position in a ring whose index `taps` holds frame 0"""
    rho = [float(v) for v in ratios] + [float(ratios[-1])]
    offset, pos = float(taps // 2), []
    for k, count in enumerate(counts):
        n = np.arange(count, dtype=np.float64)
        pos.append(offset + np.where(n > 0, n / rho[k], 0.0))
        offset = offset + (count / rho[k] if count else 0.0)
    return np.concatenate(pos) - taps
