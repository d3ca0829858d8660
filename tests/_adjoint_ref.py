"""The yardstick of the clip adjoint's tests: the dense operator A of a whole clip (fresh context, process, flush), built from the CPU
oracle alone — one unit impulse per input frame through the strict oracle, a reset in between.  A [n, j] is then the oracle's
(float)(h0 * (1 - frac) + h1 * frac), or the single row's tap, or the pass-through's 1: the very weight the kernel is defined by.
Built once per shape and shared (callers must not write into what they get).  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import _oracle as O


@functools.lru_cache(maxsize=None)
def dense_operator(taps, filters, flags, frames, ratio=None, fixed=None, lowpass_ratio=0.0, width=32):
    """A as float64 [M, frames] (every entry exactly a sample-type value).  `fixed` = (src, dst, lowpass_freq) for a fixed-ratio
    context (the ratio argument is then ignored by the oracle, as by the library), else `ratio` with an ordinary context."""
    B = O.binding(width)
    smp = np.float64 if width == 64 else np.float32
    r = B.OracleResampler(1, taps, filters, lowpass_ratio, flags, fixed=fixed, kind="strict")
    eff = float(fixed[1]) / float(fixed[0]) if fixed is not None else float(ratio)
    cap = int((frames + taps) * eff) + 64
    cols, M = [], None
    for j in range(frames):
        r.reset()
        e = np.zeros((frames, 1), smp)
        e[j, 0] = 1.0
        used, made, y = r.process(e, cap, eff, and_flush=True)
        assert used == frames and made < cap and (M is None or made == M), (used, made, M, cap)
        M = made
        cols.append(y[:, 0].astype(np.float64))
    if M is None:                                                 # an empty clip: the flush's outputs of nothing
        r.reset()
        _, M, _ = r.process(np.zeros((0, 1), smp), cap, eff, and_flush=True)
        return np.zeros((M, 0))
    A = np.stack(cols, axis=1)
    A.setflags(write=False)
    return A


def expected_gradient(A, gy):
    """(A^T gy, |A|^T |gy|, non-zero entries per column) in float64; gy [M] or shorter (the rest counts as zero)"""
    g = np.zeros(A.shape[0])
    g[:len(gy)] = np.asarray(gy, np.float64)[:A.shape[0]]
    return A.T @ g, np.abs(A).T @ np.abs(g), (A != 0).sum(axis=0)


def ulp_of(a, width=32):
    """one unit in the last place of every entry of `a`, in the sample type"""
    smp = np.float64 if width == 64 else np.float32
    a = np.abs(np.asarray(a, smp))
    return (np.nextafter(a, smp(np.inf)) - a).astype(np.float64)
