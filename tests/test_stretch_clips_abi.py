"""Whole-clip stretcher entry, host side (no device): artamdStretchClipCapacity is a true bound on what the oracle emits for a whole
clip (process call plus every flush), from a fresh context and from one that arrives mid-stream; the two new symbols are exported,
declared and listed; the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audio_resampler_amd as A
import _stretch as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [16000, 22050, 44100, 48000, 96000]
EXACT = [0.5, 1.0, 2.0, 0.25, 4.0]
_sig = {}


def signal(rate, ch):
    """0.4 s + the blocks fed in front of a mid-stream clip; made once per (rate, channels)"""
    if (rate, ch) not in _sig:
        _sig[rate, ch] = S.signal(int(rate * 0.4) + 3 * 8000, ch, rate, seed=rate % 97 + ch)
    return _sig[rate, ch]


def whole_clip(o, x, ratio):
    """the oracle's process call (skipped for an empty clip) and its flushes until one gives nothing (four at the most): total frames"""
    out = np.zeros((2 * max(o.capacity(len(x), max(ratio, 1.0)), o.capacity(0, 1.0)), x.shape[1]), x.dtype)     # (twice the reference's own per-call figure)
    total = o.feed(np.ascontiguousarray(x), out, ratio) if len(x) else 0
    for _ in range(4):
        g = o.drain(out)
        total += g
        if not g:
            break
    return total


def session(seed):
    """every mode in turn, and each of the exact ratios once in every mode (seeds 0 .. 19, again from 32 on; outside a mode's legal
    range the stage clips them); a drawn ratio otherwise; rate and channels drawn"""
    rng = np.random.default_rng(7000 + seed)
    rate = int(rng.choice(RATES))
    ch = int(rng.integers(1, 3))
    flags = [0, S.FAST, S.DUAL, S.FAST | S.DUAL][seed % 4]
    lim = (0.25, 4.0) if flags & S.DUAL else (0.5, 2.0)
    draw = lambda: float(np.exp(rng.uniform(np.log(lim[0]), np.log(lim[1]))))
    ratio = EXACT[(seed // 4) % 8] if (seed // 4) % 8 < len(EXACT) else draw()
    frames = 0 if seed % 11 == 3 else int(rng.integers(0, int(rate * 0.4) + 1))
    before = [(int(rng.integers(1, 8000)), draw()) for _ in range(int(rng.integers(1, 4)))]
    return rate, ch, flags, ratio, frames, before


@pytest.mark.parametrize("seed", range(48))
def test_clip_capacity_bounds_the_oracle_fresh_and_mid_stream(seed):
    rate, ch, flags, ratio, frames, before = session(seed)
    x = signal(rate, ch)
    ctor = (rate // 350, rate // 50, ch, flags)
    cap = A.lib().artamdStretchClipCapacity(rate // 50, flags, frames, ratio)
    # a fresh context
    made = whole_clip(S.OracleStretch(*ctor), x[:frames], ratio)
    print(f"fresh: rate {rate} ch {ch} flags {flags} ratio {ratio:.4f} frames {frames}: oracle {made}, capacity {cap}")
    assert 0 <= made <= cap
    # a context that arrives mid-stream: blocks at other ratios first, then the clip finishes the stream
    o = S.OracleStretch(*ctor)
    pos = 0
    for n, r in before:
        out = np.zeros((o.capacity(n, max(r, 1.0)), ch), x.dtype)
        o.feed(np.ascontiguousarray(x[pos:pos + n]), out, r)
        pos += n
    made = whole_clip(o, x[pos:pos + frames], ratio)
    print(f"mid-stream after {before}: oracle {made}, capacity {cap}")
    assert 0 <= made <= cap


def test_clip_capacity_is_monotone_in_the_clip_length_and_needs_no_context():
    cap = A.lib().artamdStretchClipCapacity
    for longest in (320, 882, 1920, 2400):
        for flags in (0, S.FAST, S.DUAL, S.FAST | S.DUAL):
            for ratio in (0.25, 0.3, 0.5, 0.77, 1.0, 1.01, 1.5, 1.51, 2.0, 3.1, 4.0):
                got = [cap(longest, flags, n, ratio) for n in list(range(0, 40)) + list(range(40, 40000, 997))]
                assert all(b >= a for a, b in zip(got, got[1:])), (longest, flags, ratio)
                blocks = 4 if flags & S.FAST else 3
                assert got[0] >= longest * blocks            # an empty clip can still flush a whole ring
    assert cap(882, 0, 1000, 1.0) == 1000 + 3 * 882       # nothing to stretch: the clip and the ring, at 1
    assert cap(882, 0, 1000, 1.25) == int(np.ceil((1000 + 3 * 882) * 1.5))
    assert cap(881, S.FAST, 0, 1.0) == 4 * 882             # fast mode rounds the longest period up to even
    assert cap(882, S.DUAL, 1000, 4.0) == ((1000 + 3 * 882) * 2 + 3 * 882) * 2
    assert cap(0, 0, 1000, 1.0) == -1 and cap(2401, 0, 1000, 1.0) == -1 and cap(2400, S.DUAL, 2 ** 30, 4.0) == -1


@pytest.mark.parametrize("width", [32, 64])
def test_clip_symbols_are_exported_declared_and_listed(width):
    L = A.binding(width).lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "art_hip.h")).read(), flags=re.S)
    for name in ("stretchProcessAndFlushBatchPlanarDevice", "artamdStretchClipCapacity"):
        assert hasattr(L, name)
        assert name in A.binding(width).EXPORTED_SYMBOLS
        assert re.search(r"\bint\s+" + name + r"\s*\(", text)


@pytest.mark.parametrize("width", [32, 64])
def test_clip_entry_refusals_that_need_no_device(width):
    L = A.binding(width).lib()
    one = (C.c_void_p * 1)(None)
    ints, dbl, made = (C.c_int * 1)(100), (C.c_double * 1)(1.0), (C.c_int * 1)(-5)
    assert L.stretchProcessAndFlushBatchPlanarDevice(one, 0, one, None, ints, one, None, ints, dbl, 1, made) == 0
    assert L.stretchProcessAndFlushBatchPlanarDevice(None, -3, None, None, None, None, None, None, None, 0, None) == 0
    assert L.stretchProcessAndFlushBatchPlanarDevice(one, 1, one, None, ints, one, None, ints, dbl, 1, made) == -1      # a NULL context
    assert L.stretchProcessAndFlushBatchPlanarDevice(None, 1, one, None, ints, one, None, ints, dbl, 1, made) == -1
    assert made[0] == -5
