"""The resampler at extreme ratios, against the oracle (oracle/art_oracle.c) — every other test of the suite runs between 0.18 and 6.

1. CPU: the closed-form planner (artamdPlanCall) against the oracle's literal loop at ratios from 1/60000 to 5000: counts, carried position,
   and the segment table (first_output never decreases, lin_base steps by 15 T, one segment per ring rewind + 1) — over seeded random
   sessions and over the sessions of the GPU parts below.
2. GPU: the general kernel's three LDS regimes (fir_general.hip, the span rule): (a) a tile below one pass of the four waves, (b) one output
   per tile and more than 64 KiB of LDS, (c) beyond the limit — the strict-kernel fallback (fir_dispatch.hip), float or double accumulator
   as the mode asks.
3. GPU: ring epochs without outputs and tables of more than 192 segments cut inside runs of them.
4. GPU: rational extremes (1/2048 .. 4095/1) under the matrix-core preferences.
5. GPU: strong upsampling (x 64 .. x 4500) on the general kernel, caps that cut a call between the outputs of one input frame.
6. GPU: such streams through the batch, flush-batch, planar-batch and schedule entries: the oracle's samples, the single call's bits.

The bars are the project's own: strict order bit for bit with the per-call trace (input_used, output_generated, outputOffset bits, inputIndex);
default mode within _hip.tolerance_ok (8-byte build: test_wide.within_tolerance) of the oracle's double accumulator; precise mode within one
float ulp of it.  The CPU test checks for every default-mode input that the oracle's own float loop meets that bar against its double loop."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import audio_resampler_amd as A
import _oracle
from audio_resampler_amd.api import ArtamdPosition, ArtamdSegment, ResampleResult
from _hip import HipResampler, tolerance_ok
from _oracle import BH, INTERP, LOWPASS, PRECISE, FIXED, FLUSHED, SNAP

gpu = pytest.mark.gpu
STRICT, EXTEND = A.RESAMPLE_STRICT_ORDER, A.EXTEND_CONVOLUTION_MATH
WIDTHS = [32, 64]
FILTERS = {4: 5, 8: 8, 16: 7, 64: 64, 988: 160}          # numFilters by numTaps
# (filter flags, low-pass ratio): interpolating / nearest filter, without / with a low-pass
COMBOS = [(BH | INTERP, 0.0), (BH, 0.0), (BH | INTERP | LOWPASS, 0.45), (BH | LOWPASS, 0.45)]


# ------------------------------------------------------------------------------------------------------------------
# sessions: a script of ("run", frames, cap, ratio) / ("flush", cap, ratio) calls on one stream of noise
# ------------------------------------------------------------------------------------------------------------------
def make_hip(width, ch, T, F, lowpass, flags, extra=0, kernel=0, fixed=None):
    if width == 32:
        return HipResampler(ch, T, F, lowpass, flags, fixed=fixed, extra=extra, kernel=kernel)
    r = A.wide().Resampler(ch, T, F, lowpass, flags | extra, fixed)
    if kernel:
        r.set_kernel(kernel)
    return r


def make_oracle(width, ch, T, F, lowpass, flags, extra=0, fixed=None):
    return _oracle.binding(width).OracleResampler(ch, T, F, lowpass, flags | extra, fixed=fixed)


def frames_of(script):
    return sum(c[1] for c in script if c[0] == "run")


def session_noise(width, script, ch):
    x, _ = _oracle.binding(width).noise((frames_of(script) + 8) * ch, state=0x9E3779B97F4A7C15 | 1)
    return x.reshape(-1, ch)


def play(r, x, script, adv):
    """-> ([outputs of every call], [(input_used, output_generated, outputOffset bits, inputIndex)])"""
    r.advance(adv)
    pos, ys, trace = 0, [], []
    for c in script:
        if c[0] == "flush":
            u, g, y = r.process(None, c[1], c[2], flush=True)
        else:
            u, g, y = r.process(x[pos:pos + c[1]], c[2], c[3])
            pos += u
        ys.append(np.array(y, copy=True))
        trace.append((u, g) + tuple(r.state())[:2])
    return ys, trace


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def within_bar(width, y, truth):
    """default mode against the double accumulator: the bar of the build"""
    if width == 64:
        from test_wide import within_tolerance
        return within_tolerance(y, truth)
    ok, worst, _ = tolerance_ok(y, truth)
    return ok, worst


def within_one_ulp(y, truth):
    d = np.abs(y.astype(np.float64) - truth.astype(np.float64))
    return bool(np.all(d <= np.spacing(np.abs(truth)).astype(np.float64) + 1e-45))


class Truth:
    """the oracle's side of a session: reference order (its float loop in the 4-byte build) and the double accumulator"""

    def __init__(self, width, ch, T, F, lowpass, flags, script, adv, fixed=None, x=None):
        self.x = session_noise(width, script, ch) if x is None else x
        self.ys, self.trace = play(make_oracle(width, ch, T, F, lowpass, flags, fixed=fixed), self.x, script, adv)
        self.yd, trace_d = play(make_oracle(width, ch, T, F, lowpass, flags, PRECISE, fixed=fixed), self.x, script, adv)
        assert trace_d == self.trace
        self.strict, self.double = np.concatenate(self.ys), np.concatenate(self.yd)


def check_modes(width, ch, T, F, lowpass, flags, script, adv, truth, fixed=None, kernel=0, modes=("strict", "default", "precise")):
    """the HIP library in each mode against `truth`; returns {mode: samples} and the default-mode context's last kernel"""
    got, last = {}, None
    for mode in modes:
        extra = {"strict": STRICT, "default": 0, "precise": EXTEND}[mode]
        r = make_hip(width, ch, T, F, lowpass, flags, extra=extra, kernel=0 if mode == "strict" else kernel, fixed=fixed)
        ys, trace = play(r, truth.x, script, adv)
        assert trace == truth.trace, (mode, [(a, b) for a, b in zip(trace, truth.trace) if a != b][:3])
        y = got[mode] = np.concatenate(ys)
        if mode == "strict":
            assert np.array_equal(bits(y), bits(truth.strict)), (mode, int(np.sum(bits(y) != bits(truth.strict))), y.size)
        elif mode == "default":
            ok, worst = within_bar(width, y, truth.double)
            assert ok, (mode, worst)
            last = r.last_kernel()
        elif width == 32:
            assert within_one_ulp(y, truth.double), mode
        else:                                      # (the 8-byte build has one arithmetic: the flag changes nothing)
            assert np.array_equal(bits(y), bits(got["default"])), mode
    return got, last


# ------------------------------------------------------------------------------------------------------------------
# the planner beside the oracle
# ------------------------------------------------------------------------------------------------------------------
def position_of(o):
    c = o.c
    return ArtamdPosition(c.taps, c.filters, c.flags, c.write_pos, 0, c.read_pos, c.fixed_ratio)


def plan(pos, n_in, cap, ratio):
    """artamdPlanCall, the table grown until it holds the call's segments -> (used, made, [(first_output, lin_base, base_offset)])"""
    room = 1024
    while True:
        trial = type(pos).from_buffer_copy(pos)
        res, segs = ResampleResult(), (ArtamdSegment * room)()
        n = A.lib().artamdPlanCall(C.byref(trial), n_in, cap, ratio, C.byref(res), segs, room, None)
        if n <= room:
            C.memmove(C.byref(pos), C.byref(trial), C.sizeof(trial))
            return res.input_used, res.output_generated, [(s.first_output, s.lin_base, s.base_offset) for s in segs[:n]]
        room = n + 16


def planner_follows(o, script, x=None, adv=0.0):
    """the script on the oracle `o` and on the planner, call by call"""
    o.advance(adv)
    T = o.c.taps
    pos = position_of(o)
    at = 0
    for c in script:
        flush = c[0] == "flush"
        wp, flushed = o.c.write_pos, bool(o.c.flags & FLUSHED)
        if flush:
            u, g, _ = o.process(None, c[1], c[2], flush=True)
            used, made, segs = plan(pos, -1, c[1], c[2])
        else:
            xin = np.zeros((c[1], o.channels), np.float32) if x is None else x[at:at + c[1]]
            u, g, _ = o.process(xin, c[2], c[3])
            used, made, segs = plan(pos, c[1], c[2], c[3])
            at += u
        assert (used, made) == (u, g), (c, (used, made), (u, g))
        st = o.state()
        assert np.float64(pos.outputOffset).view(np.uint64).item() == st[0] and pos.inputIndex == st[1], c
        assert (pos.flags & (FLUSHED | SNAP | FIXED)) == (st[2] & (FLUSHED | SNAP | FIXED))
        # the table: one segment per ring epoch the call touches
        assert segs[0][0] == 0 and all(a[0] <= b[0] for a, b in zip(segs, segs[1:])) and segs[-1][0] <= made
        assert all(b[1] - a[1] == 15 * T for a, b in zip(segs, segs[1:]))
        appended = u + (T // 2 if flush and not flushed else 0)
        rewinds, rest = divmod(wp + appended - o.c.write_pos, 15 * T)
        if flush and not flushed and 16 * T - wp < T // 2:
            rewinds -= 1                                       # (a flush without room for its half window rewinds first: in front of the table)
        assert rest == 0 and len(segs) == rewinds + 1, (c, len(segs), rewinds)


def log_uniform(rng, lo, hi):
    return float(math.exp(rng.uniform(math.log(lo), math.log(hi))))


@pytest.mark.parametrize("chunk", range(8))
def test_planner_equals_oracle_loop_at_extreme_ratios(chunk):
    for seed in range(chunk * 40, chunk * 40 + 40):
        rng = np.random.default_rng(77000 + seed)
        T = int(rng.choice([4, 16, 64, 988]))
        down = bool(rng.integers(0, 2))
        draw = (lambda: log_uniform(rng, 1 / 60000, 1 / 8)) if down else (lambda: log_uniform(rng, 8, 5000))
        ratio, free = draw(), bool(rng.integers(0, 2))             # free: the ratio changes every call
        interp = bool(rng.integers(0, 2))
        o = _oracle.OracleResampler(1, T, FILTERS[T], 0.0, BH | (INTERP if interp else 0))
        script = []
        for call in range(int(rng.integers(4, 9))):
            r = draw() if free else ratio
            big = 300000 if down else max(4, int(3000 / r) + 2)
            n = int(rng.choice([0, 1, int(rng.integers(0, 40)), int(log_uniform(rng, 1, big)), int(log_uniform(rng, 1, big))]))
            cap = int(rng.choice([1, int(rng.integers(1, 60)), int(log_uniform(rng, 1, 4000)), 4000]))
            script.append(("run", n, cap, r))
        script.append(("flush", int(rng.integers(1, 3000)), ratio))
        script.append(("flush", 3000, ratio))
        if script[-2][0] == "flush":                               # (the reference's own flush is out of bounds past 15.5 T: DESIGN.md)
            probe = _oracle.OracleResampler(1, T, FILTERS[T], 0.0, BH | (INTERP if interp else 0))
            probe.advance(T / 2 if seed % 3 else 0.0)
            for c in script[:-2]:
                probe.process(np.zeros((c[1], 1), np.float32), c[2], c[3])
            if probe.c.write_pos > 15 * T + T // 2:
                script = script[:-2]
        planner_follows(o, script, adv=T / 2 if seed % 3 else 0.0)


# ------------------------------------------------------------------------------------------------------------------
# 2. the LDS regimes of the general kernel
# ------------------------------------------------------------------------------------------------------------------
def lds_frames(ch, width):
    """(frames of one column group within the 64 KiB budget, within the 160 KiB - 1 KiB limit, GEN_MAX_TILE): the three constants of
    fir_general.hip's span rule, quoted once.  A tile of n outputs stages T + ceil (n / ratio) + 3 frames of CG channels."""
    LDS_BUDGET, LDS_LIMIT, GEN_MAX_TILE = 64 * 1024, 160 * 1024 - 1024, 48
    cg = 8 if ch > 4 else 4 if ch > 2 else ch
    return LDS_BUDGET // (width // 8 * cg), LDS_LIMIT // (width // 8 * cg), GEN_MAX_TILE


def regime_of(ch, T, width, ratio):
    """'ordinary' (a tile of a whole pass of the four waves at least), 'a', 'b' or 'c'"""
    budget, limit, max_tile = lds_frames(ch, width)
    tile = min(max_tile, int(math.floor((budget - T - 3) * ratio)))
    if tile >= 1:
        return "a" if tile < 8 else "ordinary"
    return "b" if T + math.ceil(1 / ratio) + 3 <= limit else "c"


def regime_ratio(ch, T, width, regime):
    """a ratio inside the regime, 20 % away from its boundaries at least"""
    budget, limit, _ = lds_frames(ch, width)
    room_b, room_l = budget - T - 3, limit - T - 3            # input frames a tile's outputs may span: within the budget, within the limit
    # (a): tile = floor (room_b * ratio) in 1 .. 7, i.e. 1 / ratio in (room_b / 8, room_b]; (b): room_b < ceil (1 / ratio) <= room_l; (c): beyond
    lo, hi = {"a": (room_b / 8, room_b), "b": (room_b, room_l), "c": (room_l, 1.5625 * room_l)}[regime]
    inv = math.sqrt(lo * hi) + 0.37
    assert 1.2 * lo <= inv <= hi / 1.2 and regime_of(ch, T, width, 1 / inv) == regime, (ch, T, width, regime, inv)
    return 1 / inv


@functools.lru_cache(maxsize=None)
def regime_script(width, ch, T, regime):
    """three calls and a flush: about 60 outputs, a call that consumes input and makes none, about 60 more — at most ~5 M samples of input"""
    ratio = regime_ratio(ch, T, width, regime)
    inv = 1 / ratio
    outs = max(6, min(60, int(5e6 / (ch * inv * 2.4))))
    flags, lowpass = combo_of(width, ch, T, regime)
    o = make_oracle(width, ch, T, FILTERS[T], lowpass, flags)
    o.advance(T / 2)
    n1 = int(outs * inv) + T
    o.process(np.zeros((n1, ch), np.float32), outs + 50, ratio)
    L, n2 = _oracle.binding(width).load_oracle(), int(0.6 * inv)
    while n2 and L.ora_resample_expected_output(o.p, n2, ratio):
        n2 //= 2
    assert n2 > 0
    return (("run", n1, outs + 50, ratio), ("run", n2, outs + 50, ratio), ("run", int(outs * inv), outs + 50, ratio), ("flush", T + 50, ratio))


def combo_of(width, ch, T, regime):
    return COMBOS[([1, 2, 3, 8, 9].index(ch) + [16, 64, 988].index(T) + "abc".index(regime) + width // 64) % 4]


REGIME_CASES = [(ch, T, regime) for ch in (1, 2, 3, 8, 9) for T in (16, 64, 988) for regime in "abc"]


def test_regime_arithmetic_matches_the_issue_examples():
    assert [regime_of(8, 64, 32, 1 / v) for v in (500, 3000, 6000)] == ["a", "b", "c"]
    assert [regime_of(8, 988, 32, 1 / v) for v in (300, 3000, 6000)] == ["a", "b", "c"]
    assert [regime_of(1, 64, 32, 1 / v) for v in (30000, 50000)] == ["b", "c"]
    assert [regime_of(8, 64, 64, 1 / v) for v in (250, 1500, 3000)] == ["a", "b", "c"]      # (the 8-byte build: half the span)
    assert regime_of(2, 380, 32, 48000 / 44100) == "ordinary"
    for width in WIDTHS:                                      # every filter / low-pass combination in every regime
        for regime in "abc":
            assert {combo_of(width, ch, T, regime) for ch, T, r in REGIME_CASES if r == regime} == set(COMBOS)


@pytest.mark.parametrize("regime", "abc")
@pytest.mark.parametrize("width", WIDTHS)
def test_regime_sessions_on_the_cpu(width, regime):
    """the sessions of part 2 without a GPU: the planner follows the oracle, the second call makes no output, and the oracle's own float
    loop meets the default mode's bar against its double loop (so the bar can be asked of the library on these inputs)"""
    for ch, T, rg in REGIME_CASES:
        if rg != regime:
            continue
        script = regime_script(width, ch, T, regime)
        flags, lowpass = combo_of(width, ch, T, regime)
        truth = Truth(width, ch, T, FILTERS[T], lowpass, flags, script, T / 2)
        assert truth.trace[1][1] == 0 and truth.trace[1][0] == script[1][1] > 0
        assert truth.trace[0][1] >= 6 and truth.trace[2][1] >= 6 and frames_of(script) * ch <= 5.5e6
        assert tolerance_ok(truth.strict, truth.double)[0]
        planner_follows(make_oracle(width, ch, T, FILTERS[T], lowpass, flags), script, truth.x, T / 2)


@gpu
@pytest.mark.parametrize("ch,T,regime", REGIME_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("width", WIDTHS)
def test_general_kernel_lds_regimes(width, ch, T, regime):
    script = regime_script(width, ch, T, regime)
    flags, lowpass = combo_of(width, ch, T, regime)
    truth = Truth(width, ch, T, FILTERS[T], lowpass, flags, script, T / 2)
    got, _ = check_modes(width, ch, T, FILTERS[T], lowpass, flags, script, T / 2, truth)
    if regime == "c" and width == 32:
        # the fallback is the strict kernel: the reference's float loop in default mode, its double loop exactly when the mode is precise
        assert np.array_equal(bits(got["default"]), bits(truth.strict))
        assert np.array_equal(bits(got["precise"]), bits(truth.double))


# ------------------------------------------------------------------------------------------------------------------
# 3. ring epochs without outputs, tables cut inside runs of them
# ------------------------------------------------------------------------------------------------------------------
MAX_SEGS = 192                                                # (art_internal.h: segments per launch)


def empty_segments(segs, made):
    firsts = [s[0] for s in segs] + [made]
    return [firsts[i + 1] == firsts[i] for i in range(len(segs))]


@functools.lru_cache(maxsize=None)
def cut_script(T, per_output):
    """A script at ratio 1 / (per_output * T), found with the planner: after a lead call, (i) + (ii) a call of more than 192 segments, most of
    them empty, whose cut at 192 lies inside a run of empty ones with outputs on both sides; (iii) a call whose last cut launch has no
    output; (iv) a call that appends more than 100 histories and makes nothing; then one that makes output.  Where the ratio leaves no
    such run (few frames per output) the same call sizes without the conditions."""
    ratio, cap, epoch = 1.0 / (per_output * T + 0.37), 100000, 15 * T
    sparse = per_output >= 100
    o = _oracle.OracleResampler(1, T, FILTERS[T], 0.0, BH | INTERP)
    o.advance(T / 2)
    start = position_of(o)

    def after(pos, n):
        p = type(pos).from_buffer_copy(pos)
        return (p,) + plan(p, n, cap, ratio)

    for lead in range(0, 220 * T, 5 * T):
        pos, script = after(start, lead)[0], [("run", lead, cap, ratio)]
        p, used, made, segs = after(pos, epoch * 420)
        if sparse:
            e = empty_segments(segs, made)
            if not (len(segs) > 2 * MAX_SEGS and sum(e) > len(segs) // 2 and e[MAX_SEGS - 2] and e[MAX_SEGS - 1] and e[MAX_SEGS]
                    and e[2 * MAX_SEGS - 1] and e[2 * MAX_SEGS] and segs[MAX_SEGS][0] > 0 and made > segs[2 * MAX_SEGS][0]):
                continue
        pos = p
        script.append(("run", epoch * 420, cap, ratio))
        for n in range(epoch * MAX_SEGS + T, epoch * (MAX_SEGS + 14), T):
            p, used, made, segs = after(pos, n)
            if not sparse or (MAX_SEGS < len(segs) <= 2 * MAX_SEGS and made > 0 and segs[MAX_SEGS][0] == made and used == n):
                break
        else:
            continue
        pos = p
        script.append(("run", n, cap, ratio))
        for n in range(151 * T, max(152, per_output - 1) * T, T):
            p, used, made, segs = after(pos, n)
            if not sparse or (made == 0 and used == n):
                break
        else:
            continue
        pos = p
        script.append(("run", n, cap, ratio))
        p, used, made, segs = after(pos, 2 * per_output * T + epoch)
        if made == 0:
            continue
        script += [("run", 2 * per_output * T + epoch, cap, ratio), ("flush", T + 50, ratio)]
        return tuple(script)
    raise AssertionError("no such script")


CUT_CASES = [(T, per, ch) for T in (4, 8, 16) for per in (4, 30, 200) for ch in (1, 2, 8)]


def test_cut_scripts_on_the_cpu():
    for T in (4, 8, 16):
        for per in (4, 30, 200):
            script = cut_script(T, per)
            o = _oracle.OracleResampler(1, T, FILTERS[T], 0.0, BH | INTERP)
            planner_follows(o, script, adv=T / 2)
            truth = Truth(32, 1, T, FILTERS[T], 0.0, BH | INTERP, script, T / 2)
            assert tolerance_ok(truth.strict, truth.double)[0]
            if per == 200:
                assert truth.trace[3][1] == 0 and truth.trace[3][0] > 100 * (T + T // 2) and truth.trace[4][1] > 0


@gpu
@pytest.mark.parametrize("T,per,ch", CUT_CASES)
@pytest.mark.parametrize("width", WIDTHS)
def test_empty_epochs_and_cut_tables(width, T, per, ch):
    script = cut_script(T, per)
    flags = BH | INTERP if (T + per + ch) % 2 else BH
    truth = Truth(width, ch, T, FILTERS[T], 0.0, flags, script, T / 2)
    check_modes(width, ch, T, FILTERS[T], 0.0, flags, script, T / 2, truth, modes=("strict", "default"))


# ------------------------------------------------------------------------------------------------------------------
# 4. rational extremes under the matrix-core preferences
# ------------------------------------------------------------------------------------------------------------------
# (name, destination rate, source rate, input frames per call)
RATIONAL = [("1/64", 1, 64, 64 * 200), ("1/2048", 1, 2048, 2048 * 40), ("3/4096", 3, 4096, 4096 * 10), ("4095/65536", 4095, 65536, 3200),
            ("64/1", 64, 1, 100), ("4095/1", 4095, 1, 3), ("4096/3", 4096, 3, 9)]
KERNEL_NAMES = {0: "none", 1: "general", 2: "matrix"}


def rational_script(dst, src, counts, fixed):
    ratio = 0.0 if fixed else dst / src
    cap = int(sum(counts) * dst / src) + 4200                  # (no cap cuts a call short)
    return tuple(("run", n, cap, ratio) for n in counts) + (("flush", cap, ratio),)


RATIONAL_CASES = [(w, c, k, f) for w in WIDTHS for c in RATIONAL for k in ((0, 2, 9) if w == 32 else (0, 2)) for f in (False, True)]


@gpu
@pytest.mark.parametrize("width,case,kernel,fixed", RATIONAL_CASES,
                         ids=[f"{w}-{c[0].replace('/', '_')}-pref{k}-{'fixed' if f else 'free'}" for w, c, k, f in RATIONAL_CASES])
def test_rational_extremes(width, case, kernel, fixed):
    """(preference 9, the cut-invariant policy, pins the f32 streaming kernel: 4-byte build only)"""
    name, dst, src, n = case
    ch, T, F = 2, 64, 512
    flags = BH | INTERP | (LOWPASS if fixed else 0)
    rates = (float(src), float(dst), 0) if fixed else None
    script = rational_script(dst, src, (n, n, n), fixed)
    truth = Truth(width, ch, T, F, 0.0, flags, script, T / 2, fixed=rates)
    assert tolerance_ok(truth.strict.astype(np.float32), truth.double.astype(np.float32))[0]
    r = make_hip(width, ch, T, F, 0.0, flags, kernel=kernel, fixed=rates)
    ys, trace = play(r, truth.x, script, T / 2)
    assert trace == truth.trace
    ok, worst = within_bar(width, np.concatenate(ys), truth.double)
    assert ok, worst
    assert A.binding(width).lib().artamdErrorCount() == 0
    print(f"RATIONAL width={width} {name} {'fixed' if fixed else 'free'} pref={kernel}: last kernel {KERNEL_NAMES.get(r.last_kernel(), r.last_kernel())}, "
          f"cut-invariant fallbacks {r.cut_invariant_fallbacks()}")
    if kernel == 9:
        # The policy's property: the same stream cut into other blocks, the same bits — of a fixed-ratio stream, whose position is put back
        # on the filter grid after every call.  A free-ratio stream carries base + made / ratio as it rounds: the reference's own outputs
        # depend on the cut there (in the last bit of a phase), so the other cut is held to the oracle on that cut instead.
        first, last = max(1, int(0.4 * n)), max(1, int(0.9 * n))
        other = rational_script(dst, src, (first, 3 * n - first - last, last), fixed)
        r2 = make_hip(width, ch, T, F, 0.0, flags, kernel=kernel, fixed=rates)
        ys2, trace2 = play(r2, truth.x, other, T / 2)
        a, b = np.concatenate(ys), np.concatenate(ys2)
        if fixed:
            assert trace2[-2][2:] == trace[-2][2:]
            assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), int(np.sum(bits(a) != bits(b)))
        else:
            truth2 = Truth(width, ch, T, F, 0.0, flags, other, T / 2, x=truth.x)
            assert trace2 == truth2.trace
            ok, worst = within_bar(width, b, truth2.double)
            assert ok, worst


# ------------------------------------------------------------------------------------------------------------------
# 5. strong upsampling on the general kernel
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("F", [1, 16, 1024])
@pytest.mark.parametrize("flags", [BH | INTERP, BH], ids=["interpolating", "nearest"])
@pytest.mark.parametrize("ratio", [64 * (1 + 3e-6), 1000.37, 4500.0], ids=["x64", "x1000", "x4500"])
@pytest.mark.parametrize("width", WIDTHS)
def test_strong_upsampling(width, ratio, flags, F):
    ch, T = (3, 16) if ratio > 2000 else (2, 64)
    big = int(41 * ratio) + 64
    # half a window to the first output, then calls of 0, 1, 2, 3 and 40 frames; caps that end a call between the outputs of one input frame,
    # the next call goes on from there
    script = (("run", T // 2, big, ratio), ("run", 0, big, ratio), ("run", 1, big, ratio), ("run", 2, int(1.5 * ratio), ratio), ("run", 2, big, ratio),
              ("run", 3, big, ratio), ("run", 40, int(7.3 * ratio), ratio), ("run", 40, 1, ratio), ("run", 40, big, ratio), ("run", 0, big, ratio),
              ("flush", big, ratio))
    truth = Truth(width, ch, T, F, 0.0, flags, script, T / 2)
    made = [t[1] for t in truth.trace]
    # (the caps did cut those calls: the outputs of the last frame taken are not all made, the next call goes on among them)
    assert made[3] == script[3][2] and made[6] == script[6][2] and truth.trace[6][0] < 40 and made[7] == 1
    assert made[1] == 0 and made[2] > 0 and made[4] > 0 and made[5] > 2 * int(ratio) and made[8] > 40 * int(ratio)
    _, last = check_modes(width, ch, T, F, 0.0, flags, script, T / 2, truth)
    assert last == 1                                           # (an irrational ratio: the general kernel)


# ------------------------------------------------------------------------------------------------------------------
# 6. the same streams through every entry
# ------------------------------------------------------------------------------------------------------------------
SENTINEL, GAP = -12345.5, 7


def mixed_streams(width):
    """(name, channels, taps, flags, ratio, frames per tick)"""
    rb, rc = regime_ratio(8, 64, width, "b"), regime_ratio(8, 988, width, "c")
    return [("regime_b", 8, 64, BH | INTERP, rb, int(6 / rb)),
            ("regime_c", 8, 988, BH | INTERP, rc, int(min(7 / rc, 40000))),          # (at most 4 ring epochs of 15 T frames per call)
            ("empty_epochs", 2, 8, BH | INTERP, 1 / (200 * 8 + 0.37), 15 * 8 * 30),
            ("x1000", 2, 64, BH, 1000.37, 40),
            ("ordinary", 2, 48, BH | INTERP, 48000 / 44100, 1500)]


class Slab:
    """every buffer of a call in one device tensor, sentinel-filled, odd gaps between them (interleaved buffers on 16-byte boundaries)"""

    def __init__(self, torch, sizes, dt, aligned):
        self.off, at = [], GAP
        for n, al in zip(sizes, aligned):
            if al:
                at = (at + 3) & ~3
            self.off.append(at)
            at += n + GAP
        self.want = np.full(at, SENTINEL, dt)
        self.torch = torch

    def upload(self):
        self.buf = self.torch.from_numpy(self.want).cuda()

    def ptr(self, i):
        return self.buf.data_ptr() + self.off[i] * self.buf.element_size()

    def intact(self):
        """everything the host's picture does not expect a call to have written is as it was"""
        self.torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        return np.array_equal(bits(got), bits(self.want))


def put(want, off, pitch, x):
    n, ch = x.shape
    if pitch:
        for c in range(ch):
            want[off + c * pitch:off + c * pitch + n] = x[:, c]
    else:
        want[off:off + n * ch] = x.reshape(-1)


def take(buf, off, pitch, n, ch):
    return np.stack([buf[off + c * pitch:off + c * pitch + n] for c in range(ch)], axis=1) if pitch else buf[off:off + n * ch].reshape(n, ch)


@gpu
@pytest.mark.parametrize("entry", ["batch", "flush_batch", "planar_batch", "planar_flush_batch"])
@pytest.mark.parametrize("width", WIDTHS)
def test_extreme_streams_through_the_batch_entries(width, entry):
    torch = pytest.importorskip("torch")
    B, O = A.binding(width), _oracle.binding(width)
    dt = np.float32 if width == 32 else np.float64
    streams = mixed_streams(width)
    n = len(streams)
    planar, and_flush = entry.startswith("planar"), "flush" in entry
    mk = lambda s: B.Resampler(s[1], s[2], FILTERS.get(s[2], s[2]), 0.0, s[3])
    batch, single = [mk(s) for s in streams], [mk(s) for s in streams]
    oracle = [O.OracleResampler(s[1], s[2], FILTERS.get(s[2], s[2]), 0.0, s[3] | PRECISE) for s in streams]
    for r, s in zip(batch + single + oracle, streams * 3):
        r.advance(s[2] / 2)
    errors, made = B.lib().artamdErrorCount(), [0] * n
    for tick in range(1 if and_flush else 3):
        frames = [s[5] + 3 * tick for s in streams]
        caps = [int(f * s[4]) + 4 + (int(s[2] / 2 * s[4]) + 4 if and_flush else 0) for f, s in zip(frames, streams)]
        x = [O.noise(f * s[1], state=(0x1234567 + 2 * (tick * n + i)) | 1)[0].reshape(f, s[1]) for i, (f, s) in enumerate(zip(frames, streams))]
        ip = [f + 5 if planar and s[1] > 1 else 0 for f, s in zip(frames, streams)]
        op = [c + 5 if planar and s[1] > 1 else 0 for c, s in zip(caps, streams)]
        sizes = [s[1] * p if p else f * s[1] for f, p, s in zip(frames, ip, streams)] + [s[1] * p if p else c * s[1] for c, p, s in zip(caps, op, streams)]
        slab = Slab(torch, sizes, dt, [p == 0 for p in ip + op])
        for i in range(n):
            put(slab.want, slab.off[i], ip[i], x[i])
        slab.upload()
        ins, outs = [slab.ptr(i) for i in range(n)], [slab.ptr(n + i) for i in range(n)]
        if planar:
            fn = B.process_and_flush_batch_planar_device if and_flush else B.process_batch_planar_device
            got = fn(batch, ins, ip, frames, outs, op, caps, [s[4] for s in streams])                 # (raises where the entry fails)
        else:
            fn = B.process_and_flush_batch_device if and_flush else B.process_batch_device
            got = fn(batch, ins, frames, outs, caps, [s[4] for s in streams])
        torch.cuda.synchronize()
        have = slab.buf.cpu().numpy()
        for i, s in enumerate(streams):
            tag = (width, entry, tick, s[0])
            uo, go, yo = oracle[i].process(x[i], caps[i], s[4], and_flush=and_flush)
            assert got[i] == (uo, go), (tag, got[i], (uo, go))
            y = take(have, slab.off[n + i], op[i], go, s[1])
            made[i] += go
            if go:
                ok, worst = within_bar(width, y, yo)
                assert ok, (tag, worst)
            # the single call: the same bits
            d_in = torch.from_numpy(x[i]).cuda()
            d_out = torch.zeros(caps[i], s[1], dtype=d_in.dtype, device="cuda")
            us, gs = single[i].process_device(d_in, frames[i], d_out, caps[i], s[4], and_flush=and_flush)
            assert (us, gs) == got[i], tag
            assert np.array_equal(bits(y), bits(d_out[:gs].cpu().numpy())), tag
            assert batch[i].state() == single[i].state(), tag
            put(slab.want, slab.off[n + i], op[i], y)
        assert slab.intact(), (width, entry, tick)
    assert min(made) > 0, made
    assert B.lib().artamdErrorCount() == errors        # (no failure was counted; the counter is the process's: 0 in a run of its own)


@gpu
@pytest.mark.parametrize("width", WIDTHS)
def test_schedule_crosses_the_regimes_and_back(width):
    torch = pytest.importorskip("torch")
    B, O = A.binding(width), _oracle.binding(width)
    dt = np.float32 if width == 32 else np.float64
    ch, T = 8, 64
    ra, rb, rc = (regime_ratio(ch, T, width, g) for g in "abc")
    ratios = [ra, ra, rb, rc, rc, rb, ra, 48000 / 44100]
    n_ins = [int(6.5 / r) for r in ratios[:-1]] + [700]
    caps = [int(f * r) + 8 for f, r in zip(n_ins, ratios)]
    mk = lambda: B.Resampler(ch, T, FILTERS[T], 0.0, BH | INTERP)
    sched, single, oracle = mk(), mk(), O.OracleResampler(ch, T, FILTERS[T], 0.0, BH | INTERP | PRECISE)
    for r in (sched, single, oracle):
        r.advance(T / 2)
    x = O.noise(sum(n_ins) * ch, state=0x7654321 | 1)[0].reshape(-1, ch)
    slab = Slab(torch, [x.size, sum(caps) * ch], dt, [True, True])
    put(slab.want, slab.off[0], 0, x)
    slab.upload()
    errors = B.lib().artamdErrorCount()
    made, res = sched.process_schedule_device(slab.ptr(0), n_ins, slab.ptr(1), caps, ratios)
    torch.cuda.synchronize()
    assert made == len(n_ins)
    have = slab.buf.cpu().numpy()
    d_x = torch.from_numpy(x).cuda()
    at = out_at = 0
    for k, (f, cap, ratio) in enumerate(zip(n_ins, caps, ratios)):
        uo, go, yo = oracle.process(x[at:at + f], cap, ratio)
        assert res[k] == (uo, go) and uo == f and go >= 4, (k, res[k], (uo, go))
        y = take(have, slab.off[1] + out_at * ch, 0, go, ch)
        ok, worst = within_bar(width, y, yo)
        assert ok, (k, worst)
        d_out = torch.zeros(cap, ch, dtype=d_x.dtype, device="cuda")
        assert single.process_device(d_x[at:], f, d_out, cap, ratio) == res[k]
        assert np.array_equal(bits(y), bits(d_out[:go].cpu().numpy())), k
        put(slab.want, slab.off[1] + out_at * ch, 0, y)
        at += f
        out_at += go
    assert sched.state() == single.state()
    assert slab.intact()
    assert B.lib().artamdErrorCount() == errors        # (no failure was counted; the counter is the process's: 0 in a run of its own)
