"""The yardstick of the band-limited clip sampler's tests: tests/_sampler_ref.py's `sample` called once per rung of a ladder and blended
in float64 by the definitions of art_hip.h — never the library's own output.

    a level l on a ladder of K rungs: !(l > 0) (a NaN, -0.0, a negative): L = 0, lam = 0;  l >= K - 1: L = K - 1, lam = 0;
    else L = floor (l), lam = l - L.
    ys = a_L where lam == 0, else a_L (1.0 - lam) + a_{L+1} lam, a_k the yardstick's ys of rung k; scale, D and slope_scale blended alike;
    A [m, j] = (sample type)(w_L) where lam == 0, else (sample type)(w_L (1.0 - lam) + w_{L+1} lam), w_k = h0 (1 - frac) + h1 frac unrounded;
    gp [m] = sum_c gy D;  gl [m] = sum_c gy (a_{j+1} - a_j), j = min (L, K - 2), for 0 <= l <= K - 1 (-0.0 among them), else 0 — and 0 for
    K = 1 and without a window.

A rung is (lowpass, flags) for _sampler_ref.sample; `ladder` makes them from cut-offs as ClipBandSampler does (1.0: no low-pass).
`auto_levels` restates ClipBandSampler.levels_of in numpy.  TEST INFRASTRUCTURE ONLY."""
import types

import numpy as np

import _oracle as O
import _sampler_ref as S


def ladder(cutoffs, flags):
    """[(lowpass, flags)] per cut-off, as resampleInit normalises them: a cut-off of 1.0 is a bank without INCLUDE_LOWPASS"""
    return [(0.0, flags & ~O.LOWPASS) if c >= 1.0 else (float(c), flags | O.LOWPASS) for c in cutoffs]


def decode(levels, K):
    """levels [M] -> (L [M] int, lam [M], moves [M] bool: the level gradient is not forced to zero)"""
    l = np.asarray(levels, np.float64)
    with np.errstate(invalid="ignore"):
        low, high = ~(l > 0), l >= K - 1
        moves = (l >= 0) & (l <= K - 1) & (K >= 2)
    inner = np.where(low | high, 0.0, l)
    L = np.where(low, 0, np.where(high, K - 1, np.floor(inner))).astype(np.int64)
    lam = np.where(low | high, 0.0, inner - np.floor(inner))
    return L, lam, moves


def auto_levels(p, n_out, cutoffs, guard=1.0):
    """ClipBandSampler.levels_of for one clip: p [M], n_out <= M -> [M]"""
    p = np.asarray(p, np.float64)
    M, K = len(p), len(cutoffs)
    level = np.zeros(M)
    with np.errstate(invalid="ignore", divide="ignore"):
        for m in range(n_out):
            lo, hi = max(m - 1, 0), min(m + 1, n_out - 1)
            s = abs(p[hi] - p[lo]) / (hi - lo) if hi > lo else 1.0
            if not np.isfinite(s):
                level[m] = np.nan
                continue
            at = np.log(guard / max(s, 1.0))
            level[m] = sum(min(max((np.log(cutoffs[k]) - at) / (np.log(cutoffs[k]) - np.log(cutoffs[k + 1])), 0.0), 1.0) for k in range(K - 1))
    return level


def sample(taps, filters, rungs, x, p, levels, gy=None, width=64, operator=False, per_rung=None):
    """rungs: [(lowpass, flags)]; x [C, N], p [M], levels [M], gy [C, M] or None -> a namespace of float64 arrays: live, L, lam, moves [M],
    ys, scale, D, slope_scale [C, M], rung (the per-rung namespaces of _sampler_ref.sample); with gy: gp, gp_scale, gl, gl_scale [M]; with
    operator (and gy): A [M, N], gx, gx_scale [C, N], entries [N].  per_rung: the rungs' namespaces from an earlier call on the same x, p, gy."""
    smp = np.float64 if width == 64 else np.float32
    K = len(rungs)
    x = np.atleast_2d(np.asarray(x, np.float64))
    p = np.asarray(p, np.float64)
    rung = per_rung or [S.sample(taps, filters, lp, fl, x, p, gy, width) for lp, fl in rungs]
    L, lam, moves = decode(levels, K)
    Ln = np.minimum(L + 1, K - 1)
    live = rung[0].live
    m = np.arange(len(p))

    def pick(name, k):
        return np.stack([getattr(r, name) for r in rung])[k, :, m].T          # [C, M]

    def blend(name):
        lo, hi = pick(name, L), pick(name, Ln)
        return np.where(lam == 0, lo, lo * (1.0 - lam) + hi * lam)

    out = types.SimpleNamespace(live=live, L=L, lam=lam, moves=moves & live, rung=rung, ys=blend("ys"), scale=blend("scale"), D=blend("D"),
                                slope_scale=blend("slope_scale"))
    if gy is not None:
        g = np.where(live[None], np.atleast_2d(np.asarray(gy, np.float64)), 0.0)
        out.gp, out.gp_scale = (g * out.D).sum(0), (np.abs(g) * out.slope_scale).sum(0)
        if K >= 2:
            j = np.minimum(L, K - 2)
            out.gl = np.where(out.moves, (g * (pick("ys", j + 1) - pick("ys", j))).sum(0), 0.0)
            out.gl_scale = np.where(out.moves, (np.abs(g) * (pick("scale", j + 1) + pick("scale", j))).sum(0), 0.0)
        else:
            out.gl, out.gl_scale = np.zeros(len(p)), np.zeros(len(p))
    if operator:
        N, T, F = x.shape[1], taps, filters
        banks = [S.bank_of(taps, filters, lp, fl, width).astype(np.float64) for lp, fl in rungs]
        fi, frac, first = rung[0].fi, rung[0].frac, rung[0].first
        W = np.stack([b[fi] * (1.0 - frac)[:, None] + b[np.minimum(fi + 1, F)] * frac[:, None] for b in banks])       # [K, M, T], unrounded
        lo, hi = W[L, m], W[Ln, m]
        Wb = np.where((lam == 0)[:, None], lo, lo * (1.0 - lam)[:, None] + hi * lam[:, None]).astype(smp).astype(np.float64)
        taps_at = first[:, None] + np.arange(T)[None, :]
        ok = live[:, None] & (taps_at >= 0) & (taps_at < N)
        A = np.zeros((len(p), N))
        r, c = np.nonzero(ok)
        A[r, taps_at[r, c]] = Wb[r, c]
        out.A = A
        if gy is not None:
            out.gx, out.gx_scale, out.entries = g @ A, np.abs(g) @ np.abs(A), (A != 0).sum(axis=0)
    return out
