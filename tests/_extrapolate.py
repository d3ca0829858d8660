"""End-point LPC extrapolation test cases (artamdExtrapolateBatchDevice): the known samples are regenerated from seeds here, so
only the reference's outputs are stored (tests/golden/extrapolate.npz, tests/golden/make_golden_extrapolate.py).
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import hashlib
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "extrapolate.npz")

T = 1024                                     # the window the third extras value completes (T - count)
COUNTS = (8, 9, 64, 190, 494, 495, 987, 1023)
KINDS = ("white", "two_sines", "low_sine", "dc", "zeros", "alternate", "impulse", "subnormal", "huge", "nan", "inf")
HEAD, TAIL = 192, 64                         # stored samples of the longest run (all of it when shorter than HEAD + TAIL)


def dtype(width):
    return np.float64 if width == 64 else np.float32


def extras_of(count):
    return sorted({1, count, T - count})


def signal(kind, count, width, seed=0):
    """`count` known samples, oldest first"""
    dt = dtype(width)
    rng = np.random.default_rng([seed, count, KINDS.index(kind) if kind in KINDS else 99, width])
    n = np.arange(count, dtype=np.float64)
    if kind == "white":
        x = rng.uniform(-1.0, 1.0, count)
    elif kind == "two_sines":
        x = 0.5 * np.sin(2 * np.pi * 0.0123 * n + 0.3) + 0.3 * np.sin(2 * np.pi * 0.071 * n + 1.1)
    elif kind == "low_sine":                 # low sine + faint noise: the fit runs close to its probe limit
        x = 0.8 * np.sin(2 * np.pi * 0.0021 * n + 0.7) + 1e-4 * rng.standard_normal(count)
    elif kind == "dc":
        x = np.full(count, 0.375)
    elif kind == "zeros":
        x = np.zeros(count)
    elif kind == "alternate":
        x = np.where(np.arange(count) % 2 == 0, 1.0, -1.0)
    elif kind == "impulse":
        x = np.zeros(count)
        x[count // 3] = 1.0
    elif kind == "subnormal":                # f32-subnormal amplitudes (and squares that underflow in the 4-byte build)
        x = rng.uniform(-1.0, 1.0, count) * 1e-39
    elif kind == "huge":                     # squares overflow f32: the 4-byte build's energy is inf
        x = rng.uniform(-1.0, 1.0, count) * 1e30
    elif kind in ("nan", "inf"):
        # a silent run with one non-finite sample among the first three the fit sees (the reference stops the process on a
        # non-finite quality, which a non-finite sample anywhere else produces)
        x = np.zeros(count)
        x[1] = np.nan if kind == "nan" else -np.inf
    else:
        raise ValueError(kind)
    return x.astype(dt)


def fit_order(x, backward):
    """the samples in the order the fit sees them: a backward run is fitted on the time-reversed samples"""
    return x[::-1].copy() if backward else x


def place(kind, count, width, backward):
    """the known samples as a caller holds them (oldest first), with the nan / inf sample at the fit's index 1"""
    x = signal(kind, count, width)
    return fit_order(x, backward) if kind in ("nan", "inf") else x


def digest(a):
    return np.uint64(int.from_bytes(hashlib.blake2b(np.ascontiguousarray(a).tobytes(), digest_size=8).digest(), "little"))


def key(width, kind, count, backward):
    return f"w{width}/{kind}/{count}/{'b' if backward else 'f'}"


class RefExtrapolator:
    """the reference's extrapolate_forward / extrapolate_reverse from oracle/_ref/libartref{,64}_strict.so"""

    def __init__(self, width):
        suffix = "64" if width == 64 else ""
        self.L = C.CDLL(os.path.join(REF_DIR, f"libartref{suffix}_strict.so"))
        self.dt = dtype(width)
        for name in ("extrapolate_forward", "extrapolate_reverse"):
            getattr(self.L, name).restype = C.c_double
            getattr(self.L, name).argtypes = [C.c_void_p, C.c_int, C.c_int]

    def run(self, known, extras, backward):
        """forward: the extras samples past the newest; backward: the extras samples before the oldest, nearest first"""
        count = len(known)
        buf = np.zeros(count + extras, self.dt)
        if backward:
            buf[extras:] = known
            self.L.extrapolate_reverse(buf.ctypes.data + (extras + count) * buf.itemsize, count, extras)   # (one past the newest)
            return buf[:extras][::-1].copy()
        buf[:count] = known
        self.L.extrapolate_forward(buf.ctypes.data, count, extras)
        return buf[count:].copy()


def ref_available(width=32):
    return os.path.exists(os.path.join(REF_DIR, f"libartref{'64' if width == 64 else ''}_strict.so"))
