"""The logged stretcher entry, its adjoint and the log capacity, host side (no device): the three symbols are exported, declared and
listed; the answers and refusals that need no device; artamdStretchLogCapacity; and the numpy model of a log (_stretch_log) is
consistent with itself on a hand-written log that holds every segment kind."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audio_resampler_amd as A
import _stretch as S
import _stretch_log as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("artamdStretchLogCapacity", "stretchProcessAndFlushLoggedBatchPlanarDevice", "stretchAdjointClipsPlanarDevice")


class Stretch(C.Structure):                          # include/stretch.h
    pass


Stretch._fields_ = [("num_chans", C.c_int), ("inbuff_samples", C.c_int), ("shortest", C.c_int), ("longest", C.c_int),
                    ("tail", C.c_int), ("head", C.c_int), ("fast_mode", C.c_int), ("inbuff", C.c_void_p), ("calcbuff", C.c_void_p),
                    ("results", C.c_void_p), ("outsamples_error", C.c_double), ("next", C.POINTER(Stretch)),
                    ("intermediate", C.c_void_p), ("hip", C.c_void_p)]


@pytest.mark.parametrize("width", [32, 64])
def test_symbols_are_exported_declared_and_listed(width):
    L = A.binding(width).lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "art_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert hasattr(L, name)
        assert name in A.binding(width).EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)
    assert re.search(r"typedef\s+struct\s*\{\s*int\s+out\s*,\s*count\s*,\s*from\s*,\s*to\s*;\s*\}\s*ArtamdStretchSegment\s*;", text)
    assert A.STRETCH_COPY == SL.COPY == -2**31


@pytest.mark.parametrize("width", [32, 64])
def test_answers_and_refusals_that_need_no_device(width):
    L = A.binding(width).lib()
    errors = L.artamdErrorCount()
    one, two = (C.c_void_p * 1)(None), (C.c_void_p * 2)(None, None)
    ints, dbl, made = (C.c_int * 1)(100), (C.c_double * 1)(1.0), (C.c_int * 1)(-5)
    caps, counts = (C.c_int * 2)(10 ** 6, 10 ** 6), (C.c_int * 2)(-7, -7)
    logged, adjoint = L.stretchProcessAndFlushLoggedBatchPlanarDevice, L.stretchAdjointClipsPlanarDevice
    # n <= 0
    assert logged(one, 0, one, None, ints, one, None, ints, dbl, made, two, caps, counts) == 0
    assert logged(None, -3, None, None, None, None, None, None, None, None, None, None, None) == 0
    assert adjoint(one, 0, two, caps, one, None, ints, one, None, ints) == 0
    assert adjoint(None, -1, None, None, None, None, None, None, None, None) == 0
    # NULL lists, a NULL context
    assert logged(None, 1, one, None, ints, one, None, ints, dbl, made, two, caps, counts) == -1
    assert logged(one, 1, one, None, ints, one, None, ints, dbl, made, two, caps, counts) == -1
    assert adjoint(None, 1, two, caps, one, None, ints, one, None, ints) == -1
    assert adjoint(one, 1, two, caps, one, None, ints, one, None, ints) == -1
    # a context that is none of the library's, only read up to the refusal: 24 .. 168 frames, mono, one stage
    anything = (C.c_char * 256)()
    fake = Stretch(num_chans=1, inbuff_samples=3 * 168, shortest=24, longest=168, tail=168, head=168, hip=C.addressof(anything))
    ctx = (C.c_void_p * 1)(C.addressof(fake))
    buf = (C.c_char * 64)()
    ptr, logs = (C.c_void_p * 1)(C.addressof(buf)), (C.c_void_p * 2)(C.addressof(buf), None)
    need = L.artamdStretchLogCapacity(24, 168, 0, 100, 1.0, 0)
    assert need > 0
    for args in ((None, caps, counts), (logs, None, counts), (logs, caps, None),                  # a NULL list
                 (two, caps, counts),                                                            # a NULL log
                 (logs, (C.c_int * 2)(need - 1, 0), counts)):                                    # a cap below the capacity
        assert logged(ctx, 1, ptr, None, ints, ptr, None, (C.c_int * 1)(10 ** 6), dbl, made, *args) == -1
    for args in ((None, caps), (logs, None)):
        assert adjoint(ctx, 1, *args, ptr, None, ints, ptr, None, ints) == -1
    assert adjoint(ctx, 1, logs, (C.c_int * 2)(need + 1, 0), ptr, None, ints, ptr, None, ints) == -1     # more segments than 100 frames can log
    assert adjoint(ctx, 1, logs, (C.c_int * 2)(-1, 0), ptr, None, ints, ptr, None, ints) == -1
    assert adjoint(ctx, 1, logs, (C.c_int * 2)(1, 0), ptr, None, (C.c_int * 1)(-1), ptr, None, ints) == -1
    assert adjoint(ctx, 1, logs, (C.c_int * 2)(1, 0), ptr, None, ints, ptr, None, (C.c_int * 1)(0)) == 0     # n_ins 0: nothing to launch
    assert made[0] == -5 and counts[0] == -7 and counts[1] == -7
    assert L.artamdErrorCount() == errors


def test_log_capacity_rises_with_the_clip_and_follows_the_clip_capacity():
    cap, clip = A.lib().artamdStretchLogCapacity, A.lib().artamdStretchClipCapacity
    for shortest, longest in ((24, 168), (126, 882), (342, 2400)):
        for flags in (0, S.FAST, S.DUAL, S.FAST | S.DUAL):
            for ratio in (0.25, 0.3, 0.5, 0.77, 1.0, 1.01, 1.5, 2.0, 3.1, 4.0):
                for stage in (0, 1):
                    got = [cap(shortest, longest, flags, n, ratio, stage) for n in list(range(0, 40)) + list(range(40, 40000, 997))]
                    assert all(b >= a for a, b in zip(got, got[1:])), (shortest, flags, ratio, stage)
                    if stage == 1 and not flags & S.DUAL:
                        assert set(got) == {0}                   # no second stage, no segments
                    else:
                        assert got[0] >= 5 and got[-1] > got[0]  # an empty clip still passes through once and flushes four times
    # three segments per shortest period of input, the pass-through, four flushes
    assert cap(24, 168, 0, 2400, 1.25, 0) == 3 * 100 + 1 + 4
    assert cap(25, 168, S.FAST, 2400, 1.25, 0) == 3 * 100 + 1 + 4          # fast mode rounds the shortest period down to even
    # the second stage: what the first can hand it (the clip capacity's own bound at the first stage's 2.0), fed once per step, pass-through and flush
    fed = (2400 + 3 * 168) * 2
    assert cap(24, 168, S.DUAL, 2400, 3.1, 1) == 3 * (fed // 24) + (100 + 1 + 4) + 4
    # -1 where the clip capacity is, and for what is no stage or no period
    for longest, flags, n, ratio in ((0, 0, 1000, 1.0), (2401, 0, 1000, 1.0), (2400, S.DUAL, 2 ** 30, 4.0)):
        assert clip(longest, flags, n, ratio) == -1
        assert cap(24, longest, flags, n, ratio, 0) == -1 and cap(24, longest, flags, n, ratio, 1) == -1
    assert cap(0, 168, 0, 1000, 1.0, 0) == -1 and cap(24, 168, 0, 1000, 1.0, 2) == -1 and cap(24, 168, 0, 1000, 1.0, -1) == -1


def test_the_numpy_model_of_a_log_is_its_own_transpose():
    # every segment kind, as the kernel strings them: a copy out of the leading silence (negative indices), the 1:2 fade (to = from +
    # p), the 3:2 step's copy / fade back / copy, the 2:1 fade (to = from - p), a long copy (ratio 1), the flush's copy
    p = 5
    log, out = [], 0
    for count, src, to in ((7, -4, SL.COPY), (p, 3, 3 + p), (p, 13, SL.COPY), (p, 13 + p, 13), (p, 13 + p, SL.COPY),
                           (2 * p, 23, 23 - p), (2 * p, 28, 28 - p), (11, 33, SL.COPY), (3, 44, SL.COPY)):
        log.append((out, count, src, to))
        out += count
    log = np.array(log, dtype=np.int32)
    n_in, n_out = 47, SL.n_out(log)
    assert n_out == out
    rng = np.random.default_rng(5)
    x, g = rng.standard_normal(n_in), rng.standard_normal(n_out)
    Amat = SL.dense(log, n_in, n_out)
    y = SL.replay(log, x)
    assert np.allclose(Amat @ x, y, rtol=0, atol=1e-14)
    assert abs(Amat.sum(axis=1) - 1.0)[7:].max() < 1e-15          # every row past the silence: weights that sum to 1
    total, scale, terms = SL.transpose(log, n_in, g)
    lhs, rhs = float(y @ g), float(x @ total)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))
    assert np.allclose(Amat.T @ g, total, rtol=0, atol=1e-14)
    assert terms.sum() == sum(c if t == SL.COPY else 2 * c for _, c, _, t in log) - 4      # (weights of zero count; the four values of silence do not)
    assert (scale >= np.abs(total) - 1e-15).all() and (total[terms == 0] == 0).all()
    # a truncated gradient is the full one with its tail zeroed
    cut = 31
    g0 = g.copy(); g0[cut:] = 0
    assert np.array_equal(SL.transpose(log, n_in, g[:cut])[0], SL.transpose(log, n_in, g0)[0])
