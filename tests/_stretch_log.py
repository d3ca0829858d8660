"""The splice log of the time stretcher (include/art_hip.h, ArtamdStretchSegment) in numpy, float64: what a log says the stage computed
(replay), the same as a matrix (dense), and its transpose term by term (transpose).  TEST INFRASTRUCTURE ONLY.

A log is an int array [n, 4] of (out, count, from, to) in VALUES (frame * channels + channel); to == COPY: y[out+i] = x[from+i], else
y[out+i] = (x[from+i] (count-i) + x[to+i] i) / count; negative input indices are silence."""
import numpy as np

COPY = -2**31


def _parts(log):
    """per segment: (outputs o, [(input indices, integer weights), ...], count); a copy has one part of weight count"""
    for out, count, src, to in np.asarray(log, dtype=np.int64).reshape(-1, 4):
        i = np.arange(count)
        if to == COPY:
            yield out + i, [(src + i, np.full(count, count))], count
        else:
            yield out + i, [(src + i, count - i), (to + i, i)], count


def _take(x, idx):
    """x[idx], zero at negative indices"""
    return np.where(idx >= 0, x[np.clip(idx, 0, len(x) - 1)], 0.0) if len(x) else np.zeros(len(idx))


def n_out(log):
    """values the stage wrote: the end of the last segment"""
    log = np.asarray(log).reshape(-1, 4)
    return int(log[-1, 0] + log[-1, 1]) if len(log) else 0


def replay(log, x64, absolute=False):
    """the stage's output for the float64 input x64 (values); absolute: |weights| . |x| instead, the scale of its rounding errors"""
    x = np.abs(np.asarray(x64, dtype=np.float64)) if absolute else np.asarray(x64, dtype=np.float64)
    y = np.zeros(n_out(log))
    for o, parts, count in _parts(log):
        y[o] = sum(_take(x, idx) * w for idx, w in parts) / count
    return y


def dense(log, n_in, n_outs):
    """A [n_outs, n_in], float64 (small stages only: the matrix is full)"""
    A = np.zeros((n_outs, n_in))
    for o, parts, count in _parts(log):
        for idx, w in parts:
            ok = (idx >= 0) & (idx < n_in) & (o < n_outs)
            np.add.at(A, (o[ok], idx[ok]), w[ok] / count)
    return A


def transpose(log, n_in, g64):
    """A^T g term by term: (sum of each input value's terms, sum of their magnitudes, their number), float64 / float64 / int.  A term is
    g[o] w / count for every (o, v) the log lists, weights of zero included; outputs at or past len(g64) are dropped."""
    g = np.asarray(g64, dtype=np.float64)
    total, scale, terms = np.zeros(n_in), np.zeros(n_in), np.zeros(n_in, dtype=np.int64)
    for o, parts, count in _parts(log):
        for idx, w in parts:
            ok = (idx >= 0) & (idx < n_in) & (o < len(g))
            t = g[o[ok]] * w[ok] / count
            np.add.at(total, idx[ok], t)
            np.add.at(scale, idx[ok], np.abs(t))
            np.add.at(terms, idx[ok], 1)
    return total, scale, terms
