"""The yardstick of the ratio gradient's tests: a clip made block by block on an interpolating context, restated in float64 from the strict
CPU oracle alone — its bank (OracleResampler.bank ()), the per-phase output counts of a replay (the blocks' process calls, then a separate
flush call), and the position recurrence

    output n of phase k sits at p = o_k + n / rho_k (n ? n / rho_k : 0);  o_0 = taps / 2 in a ring whose index `taps` holds frame 0;
    o_{k+1} = o_k + n_k / rho_k;  rho_k = r_k for k < K, rho_K = r_{K-1} (the flush)

(the oracle's integer shifts of its ring do not matter).  With fi = floor (frac (p) F), y is the lerp of the dot products with bank rows fi
and fi + 1, so dy/dp = D = F sum_t (bank [fi + 1][t] - bank [fi][t]) x [ip + t] — on an exact filter boundary the slope of the cell that
floor picks — and with the counts held fixed

    S0_k = sum gy D,  S1_k = sum n gy D,  dL/d rho_k = -(S1_k + n_k sum_{m > k} S0_m) / rho_k^2,
    dL/d r_k = dL/d rho_k (k < K - 1),  dL/d r_{K-1} = dL/d rho_{K-1} + dL/d rho_K.

tests/test_rate_grad_ref.py holds this file to the oracle: its forward, central differences of the oracle's own forward, and the kink
convention.  TEST INFRASTRUCTURE ONLY."""
import types

import numpy as np

import _oracle as O


def replay(taps, filters, lowpass, flags, blocks, ratios, x=None, width=64):
    """the oracle's own run of the clip (x [N] or None for silence; one channel): (outputs of the K + 1 phases, y [M] as float64)"""
    B = O.binding(width)
    smp = np.float64 if width == 64 else np.float32
    r = B.OracleResampler(1, taps, filters, lowpass, flags, kind="strict")
    x = np.zeros(int(sum(blocks)), smp) if x is None else np.asarray(x, smp)
    at, counts, parts = 0, [], []
    for n, ratio in zip(blocks, ratios):
        cap = int((n + taps + 2) * ratio) + 64
        used, got, y = r.process(x[at:at + n].reshape(-1, 1), cap, float(ratio))
        assert used == n and got < cap
        at += n
        counts.append(got); parts.append(y[:, 0].astype(np.float64))
    cap = int((taps + 2) * ratios[-1]) + 64
    _, got, y = r.process(None, cap, float(ratios[-1]), flush=True)
    assert got < cap
    counts.append(got); parts.append(y[:, 0].astype(np.float64))
    return counts, np.concatenate(parts)


def clip(taps, filters, lowpass, flags, blocks, ratios, x, gy=None, width=64):
    """x [C, N] (N = sum (blocks)), gy [C, M] or None -> a namespace of float64 arrays:
    counts [K + 1], phase [M], n [M], ip [M] (frame of tap 0), cell [M] (floor (p) * F + fi: the interpolation cell), ys [C, M] (the forward
    restated), scale [C, M] (sum |b x|), D [C, M]; with gy: grad [K], terms [K] (sum |gy D n| + n_k sum_{m > k} sum |gy D|, over rho^2, the
    flush's with the last block's), gd (sum |gy D| over the clip)"""
    bank = O.binding(width).OracleResampler(1, taps, filters, lowpass, flags, kind="strict").bank().astype(np.float64)
    x = np.atleast_2d(np.asarray(x, np.float64))
    Cn, N = x.shape
    K, T, F, half = len(blocks), taps, filters, taps // 2
    assert N == sum(blocks) and len(ratios) == K
    counts, _ = replay(taps, filters, lowpass, flags, blocks, ratios, None, width)
    rho = [float(v) for v in ratios] + [float(ratios[-1])]
    offset, pos, phase, idx = float(half), [], [], []
    for k in range(K + 1):
        n = np.arange(counts[k], dtype=np.float64)
        pos.append(offset + np.where(n > 0, n / rho[k], 0.0))
        phase.append(np.full(counts[k], k)); idx.append(n)
        offset = offset + (counts[k] / rho[k] if counts[k] else 0.0)
    pos, phase, idx = np.concatenate(pos), np.concatenate(phase), np.concatenate(idx)
    whole = np.floor(pos)
    fr = (pos - whole) * F
    fi = np.floor(fr).astype(np.int64)
    frac = fr - fi
    first = whole.astype(np.int64) - half + 1 - T                  # input frame under tap 0
    # what a phase may read: frames of the clip up to the end of its block (the flush: all); silence in front of the clip and behind
    ends = np.concatenate([np.cumsum(blocks), [N]])[phase]
    taps_at = first[:, None] + np.arange(T)[None, :]                # [M, T]
    ok = (taps_at >= 0) & (taps_at < ends[:, None])
    win = np.where(ok[None], x[:, np.clip(taps_at, 0, N - 1)], 0.0) if N else np.zeros((Cn,) + taps_at.shape)      # [C, M, T]
    lo, hi = bank[fi], bank[fi + 1]                                # [M, T]

    def dot(rows):                                                 # the oracle's order: pairs from both ends towards the middle
        acc = np.zeros(win.shape[:2])
        for a, b in zip(range(T // 2), range(T - 1, T // 2 - 1, -1)):
            acc = acc + (rows[None, :, a] * win[:, :, a] + rows[None, :, b] * win[:, :, b])
        return acc

    ys = dot(lo) * (1.0 - frac) + dot(hi) * frac
    scale = (np.abs(lo)[None] * np.abs(win)).sum(2) * (1.0 - frac) + (np.abs(hi)[None] * np.abs(win)).sum(2) * frac
    D = F * ((hi - lo)[None] * win).sum(2)
    out = types.SimpleNamespace(counts=counts, phase=phase, n=idx, ip=first, cell=whole.astype(np.int64) * F + fi, ys=ys, scale=scale, D=D)
    if gy is not None:
        gy = np.atleast_2d(np.asarray(gy, np.float64))
        assert gy.shape == D.shape, (gy.shape, D.shape)
        gd, ad = (gy * D).sum(0), np.abs(gy * D).sum(0)
        S0 = np.array([gd[phase == k].sum() for k in range(K + 1)])
        S1 = np.array([(idx * gd)[phase == k].sum() for k in range(K + 1)])
        A0 = np.array([ad[phase == k].sum() for k in range(K + 1)])
        A1 = np.array([(idx * ad)[phase == k].sum() for k in range(K + 1)])
        behind = np.array([S0[k + 1:].sum() for k in range(K + 1)])
        abehind = np.array([A0[k + 1:].sum() for k in range(K + 1)])
        g = np.array([-(S1[k] + counts[k] * behind[k]) / rho[k] ** 2 for k in range(K + 1)])
        a = np.array([(A1[k] + counts[k] * abehind[k]) / rho[k] ** 2 for k in range(K + 1)])
        out.grad = np.concatenate([g[:K - 1], [g[K - 1] + g[K]]])
        out.terms = np.concatenate([a[:K - 1], [a[K - 1] + a[K]]])
        out.gd = float(ad.sum())
    return out
