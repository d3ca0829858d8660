"""GPU: resampleProcessAndFlushBatchInterleavedDevice — many whole clips, the process calls and then the flushes in shared launches.

- against the ORACLE (ora_resample_interleaved_flush): counts, position and samples of every stream of a shuffled mix under the bar its
  mode has in DESIGN.md section 5 — the first and last T/2 outputs (where a wrong extrapolated end shows) compared on their own;
- equal to the loop of resampleProcessAndFlushInterleavedDevice calls on twin contexts, bit for bit: results, samples, state (), last_kernel ();
- gathering cannot hide: every context that may share a launch reports last_gathered () == 1, every other 0, and at least three quarters
  of the mix may;
- the refusals (n <= 0, a NULL or repeated context);
- last, a timing of 1,024 stereo extrapolating clips against the loop of single calls (per clip: see the comment there).
The failure path of a launch (results of the failed launch's contexts, positions not committed, -1, counted) has no test: the
ARTAMD_TEST_FAIL_FIR hook does not count batched launches, and a real fault is never provoked."""
import time

import numpy as np
import pytest

import audio_resampler_amd as A
import _oracle
from _hip import tolerance_ok

pytestmark = pytest.mark.gpu
BH, IN, LP, EXTRAP, STRICT, EXTEND = (A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS, A.EXTRAPOLATE_ENDPOINTS,
                                      A.RESAMPLE_STRICT_ORDER, A.EXTEND_CONVOLUTION_MATH)
FLUSHED, PREFILL = A.RESAMPLER_FLUSHED, 0x80
MFMA = 2                                     # resampleHipLastKernel: the matrix-core path
UP, DOWN = 48000 / 44100, 16000 / 44100


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def tonal(frames, ch, dt, seed=1):
    """a sum of a few sines and a little noise per channel: the LPC fits run long on it, as on music"""
    rng = np.random.default_rng(seed)
    n = np.arange(frames)[:, None]
    f = rng.uniform(0.001, 0.05, (1, ch))
    x = 0.5 * np.sin(2 * np.pi * f * n + rng.uniform(0, 6.3, (1, ch))) + 0.2 * np.sin(2 * np.pi * 3.1 * f * n)
    return np.ascontiguousarray((x + 1e-4 * rng.standard_normal((frames, ch))).astype(dt))


def spec(name, ch, T, flags, frames, ratio=UP, fixed=None, F=None, side=None, cap=None, adv=None):
    """side: why the context cannot share a launch (None: it can).  cap: output room of the FIRST call when it is to be too small.
    adv: position advance before the clip (default T/2: the first output is the first input frame)"""
    return dict(name=name, ch=ch, T=T, F=F or T, flags=flags, frames=frames, ratio=ratio, fixed=fixed, side=side, cap=cap,
                adv=T / 2 if adv is None else adv)


def the_mix():
    m = [
        # the ordinary case, every channel-group class and tap count, with and without extrapolated ends
        spec("mono_48_x", 1, 48, BH | IN | EXTRAP, 20000),
        spec("stereo_380_x", 2, 380, BH | IN | EXTRAP, 20000),
        spec("three_156_x", 3, 156, BH | IN | EXTRAP, 20000, ratio=DOWN),
        spec("eight_988_x", 8, 988, BH | IN | LP | EXTRAP, 20000, fixed=(44100.0, 48000.0)),
        spec("wide33_48_x", 33, 48, BH | IN | EXTRAP, 3000, ratio=DOWN),
        spec("stereo_380", 2, 380, BH | IN, 20000, ratio=DOWN),
        spec("eight_988", 8, 988, BH | IN, 5000),
        spec("wide33_156", 33, 156, BH | IN, 2000, ratio=0.731),
        # nearest filter (no interpolation), EXTEND mode
        spec("nearest_156_x", 2, 156, BH | EXTRAP, 20000, F=320),
        spec("nearest_380", 3, 380, BH, 4000, F=300, ratio=DOWN),
        spec("extend_380_x", 8, 380, BH | IN | EXTEND | EXTRAP, 6000, ratio=DOWN),
        spec("extend_48", 2, 48, BH | IN | EXTEND, 20000),
        # clips of 0 (a pure flush), 5, T/2 - 1, T/2 and T frames: no output at all, the first output made by the flush, ...
        spec("empty_380_x", 2, 380, BH | IN | EXTRAP, 0),
        spec("empty_156", 1, 156, BH | IN, 0),
        spec("empty_988_x_unadvanced", 8, 988, BH | IN | EXTRAP, 0, adv=0.0),
        spec("five_380_x", 2, 380, BH | IN | EXTRAP, 5),
        spec("five_48_x", 3, 48, BH | IN | EXTRAP, 5, ratio=DOWN),
        spec("half_less_one_380_x", 2, 380, BH | IN | EXTRAP, 189),
        spec("half_less_one_988_x", 8, 988, BH | IN | LP | EXTRAP, 493, fixed=(96000.0, 44100.0)),
        spec("half_156_x", 3, 156, BH | IN | EXTRAP, 78),
        spec("half_380", 2, 380, BH | IN, 190),
        spec("window_988_x", 1, 988, BH | IN | EXTRAP, 988, ratio=DOWN),
        spec("window_48_x", 33, 48, BH | IN | EXTRAP, 48),
        spec("five_988_x_unadvanced", 2, 988, BH | IN | EXTRAP, 5, adv=0.0),
        # the output room too small to finish: early return, no flush; a second batched call finishes the clip
        spec("short_room_380_x", 2, 380, BH | IN | EXTRAP, 20000, cap=9000),
        spec("short_room_156", 3, 156, BH | IN, 20000, ratio=DOWN, cap=100),
        # contexts whose calls are made on the side
        spec("strict_380_x", 2, 380, BH | IN | EXTRAP | STRICT, 3000, side="strict"),
        spec("strict_48", 3, 48, BH | IN | STRICT, 3000, ratio=DOWN, side="strict"),
        spec("sharded_988_x", 8, 988, BH | IN | EXTRAP | A.RESAMPLE_MULTITHREADED, 3000, side="sharded"),
        spec("other_stream_380_x", 2, 380, BH | IN | EXTRAP, 3000, side="stream"),
        spec("flushed_156_x", 2, 156, BH | IN | EXTRAP, 0, side="flushed"),
    ]
    return m


def make(B, s, env):
    fixed = None if s["fixed"] is None else (s["fixed"][0], s["fixed"][1], 0)
    if s["side"] == "sharded":
        env.setenv("ARTAMD_SHARDS", "4")
    r = B.Resampler(s["ch"], s["T"], s["F"], 0.0, s["flags"], fixed)
    if s["side"] == "sharded":
        env.delenv("ARTAMD_SHARDS")
        assert len(r.shards()) == 4
    r.advance(s["adv"])
    return r


def make_oracle(O, s, width):
    fixed = None if s["fixed"] is None else (s["fixed"][0], s["fixed"][1], 0)
    # (default mode is measured against the double-accumulate result; strict and EXTEND against their own)
    flags = (s["flags"] & ~STRICT & ~A.RESAMPLE_MULTITHREADED) | (_oracle.PRECISE if width == 32 and not s["flags"] & STRICT else 0)
    o = O.OracleResampler(s["ch"], s["T"], s["F"], 0.0, flags, fixed)
    o.advance(s["adv"])
    return o


def within_bar(s, width, y, truth, whole=False):
    """DESIGN.md section 5, with the parity tests' own helpers (whole: all of a stream's samples — EXTEND mode's bar has a rate, which
    is the stream's, not a part's)"""
    if s["flags"] & STRICT:
        return np.array_equal(bits(y), bits(truth)), "strict: exact"
    if width == 64:
        from test_wide import within_tolerance
        return within_tolerance(y, truth)
    if s["flags"] & EXTEND:                 # (test_gpu_parity.test_precise_mode_matches_double_accumulate_reference)
        diff = y.view(np.int32).astype(np.int64) - truth.view(np.int32).astype(np.int64)
        same = np.signbit(y) == np.signbit(truth)
        ok = np.all(np.abs(diff[same]) <= 1) and np.all(np.abs(y[~same] - truth[~same]) < 1e-30) and (not whole or np.mean(diff != 0) < 1e-3)
        return bool(ok), int(np.abs(diff[same]).max()) if same.any() else 0
    ok, worst, _ = tolerance_ok(y, truth)
    return ok, worst


def ratio_of(s):
    return s["fixed"][1] / s["fixed"][0] if s["fixed"] else s["ratio"]


def room_of(s, frames):
    return int(frames * ratio_of(s) * 1.01) + 3 * s["T"] + 64


def matrix_path_clip(B, width, dt, torch):
    """the shortest power-of-two clip of the 8-channel 988-tap 44.1 -> 48 kHz stream whose process call takes the matrix-core path"""
    for frames in (32768, 65536, 131072, 262144, 524288):
        s = spec("long_988_x", 8, 988, BH | IN | LP | EXTRAP, frames, fixed=(44100.0, 48000.0))
        r = make(B, s, None)
        x = torch.zeros(frames, 8, dtype=torch.float32 if width == 32 else torch.float64, device="cuda")
        y = torch.zeros(room_of(s, frames), 8, dtype=x.dtype, device="cuda")
        r.process_device(x, frames, y, y.shape[0], UP)
        torch.cuda.synchronize()
        if r.last_kernel() == MFMA:
            return s
    pytest.fail("no clip up to 524,288 frames takes the matrix-core path")


@pytest.mark.parametrize("width", [32, 64])
def test_mixed_clips_equal_the_oracle_and_the_loop_and_are_gathered(width, monkeypatch):
    torch = pytest.importorskip("torch")
    B, O = A.binding(width), _oracle.binding(width)
    dt, tdt = (np.float32, torch.float32) if width == 32 else (np.float64, torch.float64)
    mix = the_mix() + [matrix_path_clip(B, width, dt, torch)]
    order = np.random.default_rng(2024 + width).permutation(len(mix))
    mix = [mix[i] for i in order]
    # (the lead context, whose stream and device the shared launches use, must itself be one that can share them)
    lead = next(i for i, s in enumerate(mix) if s["side"] is None)
    mix[0], mix[lead] = mix[lead], mix[0]
    n = len(mix)

    batch, loop, ora = [make(B, s, monkeypatch) for s in mix], [make(B, s, monkeypatch) for s in mix], [make_oracle(O, s, width) for s in mix]
    other = torch.cuda.Stream()
    for i, s in enumerate(mix):
        if s["side"] == "stream":
            batch[i].set_stream(other.cuda_stream); loop[i].set_stream(other.cuda_stream)
    x = [tonal(max(s["frames"], 1), s["ch"], dt, seed=100 + i)[:s["frames"]] for i, s in enumerate(mix)]
    d_x = [torch.from_numpy(v).cuda() if len(v) else None for v in x]
    room = [room_of(s, s["frames"]) for s in mix]
    d_b = [torch.zeros(c, s["ch"], dtype=tdt, device="cuda") for c, s in zip(room, mix)]
    d_l = [torch.zeros(c, s["ch"], dtype=tdt, device="cuda") for c, s in zip(room, mix)]
    ratios = [ratio_of(s) for s in mix]
    torch.cuda.synchronize()

    # the already flushed contexts: flushed by a single call before the batch, all three alike
    for i, s in enumerate(mix):
        if s["side"] == "flushed":
            want = ora[i].process(None, room[i], ratios[i], flush=True)
            for r, d in ((batch[i], d_b[i]), (loop[i], d_l[i])):
                assert r.process_device(None, -1, d, room[i], ratios[i]) == want[:2]
                assert r.c.flags & FLUSHED

    pos, made = [0] * n, [0] * n
    truth = [np.zeros((0, s["ch"]), dt) for s in mix]
    gatherable = [s["side"] is None for s in mix]
    assert sum(gatherable) >= 0.75 * n, (sum(gatherable), n)
    kinds = set()
    for call in range(2):
        live = [i for i in range(n) if call == 0 or mix[i]["cap"] is not None]
        caps = [mix[i]["cap"] if call == 0 and mix[i]["cap"] is not None else room[i] - made[i] for i in live]
        n_in = [mix[i]["frames"] - pos[i] for i in live]
        ins = [None if d_x[i] is None else d_x[i][pos[i]:] for i in live]
        before = [bool(batch[i].c.flags & PREFILL) for i in live]
        got = B.process_and_flush_batch_device([batch[i] for i in live], ins, n_in, [d_b[i][made[i]:] for i in live], caps, [ratios[i] for i in live])
        torch.cuda.synchronize()
        for k, i in enumerate(live):
            s, tag = mix[i], (width, call, mix[i]["name"])
            single = loop[i].process_device(ins[k], n_in[k], d_l[i][made[i]:], caps[k], ratios[i], and_flush=True)
            torch.cuda.synchronize()
            uo, go, yo = ora[i].process(x[i][pos[i]:], caps[k], ratios[i], and_flush=True)
            # the loop, bit for bit
            assert got[k] == single, tag
            u, g = got[k]
            assert np.array_equal(bits(d_b[i][made[i]:made[i] + g].cpu().numpy()), bits(d_l[i][made[i]:made[i] + g].cpu().numpy())), tag
            assert batch[i].state() == loop[i].state(), tag
            assert batch[i].last_kernel() == loop[i].last_kernel(), tag
            assert loop[i].last_gathered() == 0, tag
            # the oracle: counts and position exactly
            assert (u, g) == (uo, go), tag
            so, sb = ora[i].state(), batch[i].state()
            assert sb[:2] == so[:2] and (sb[2] & FLUSHED) == (so[2] & FLUSHED), (tag, sb, so)
            truth[i] = np.concatenate([truth[i], yo])
            flushed_now = bool(sb[2] & FLUSHED) and s["side"] != "flushed"
            if flushed_now:
                assert batch[i].last_gathered() == (1 if gatherable[i] else 0), tag
                kinds.add("no_output" if made[i] + g == 0 else "first_by_flush" if before[k] and s["flags"] & EXTRAP and u < s["T"] // 2 and g else "ordinary")
                if s["name"].startswith("long_"):
                    kinds.add("matrix_then_gathered_flush")
                    assert batch[i].last_gathered() == 1, tag
            else:
                kinds.add("early_return" if s["side"] is None else "side_unflushed")
                if s["side"] is not None:
                    assert batch[i].last_gathered() == 0, tag
            pos[i] += u; made[i] += g
    # every clip is finished, and every case the mix is there for has occurred
    assert all(batch[i].c.flags & FLUSHED for i in range(n))
    assert {"no_output", "first_by_flush", "ordinary", "early_return", "matrix_then_gathered_flush"} <= kinds, kinds

    # the oracle's samples: the two ends on their own, so that a failure names the end
    bad = []
    for i, s in enumerate(mix):
        y, t, half = d_b[i][:made[i]].cpu().numpy(), truth[i], s["T"] // 2
        assert y.shape == t.shape, s["name"]
        parts = {"whole": (y, t)} if made[i] <= 2 * half else {"first T/2": (y[:half], t[:half]), "last T/2": (y[-half:], t[-half:]), "between": (y[half:-half], t[half:-half])}
        if s["flags"] & EXTEND:
            parts["every sample"] = (y, t)
        for part, (a, b) in parts.items():
            if a.size:
                ok, worst = within_bar(s, width, a, b, whole=part in ("whole", "every sample"))
                print(f"width {width} {s['name']:28s} {part:10s} frames {a.shape[0]:6d}  {'ok' if ok else 'OUT OF BAR'}  worst {worst}")
                if not ok:
                    bad.append((s["name"], part, worst))
    assert not bad, bad


@pytest.mark.parametrize("width", [32, 64])
def test_long_clip_was_processed_on_the_matrix_cores_by_the_twin(width):
    """(what the mix relies on: the long clip's process call is the matrix-core path's, its flush the general kernel's)"""
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    dt, tdt = (np.float32, torch.float32) if width == 32 else (np.float64, torch.float64)
    s = matrix_path_clip(B, width, dt, torch)
    r = make(B, s, None)
    x = torch.from_numpy(tonal(s["frames"], 8, dt, seed=3)).cuda()
    y = torch.zeros(room_of(s, s["frames"]), 8, dtype=tdt, device="cuda")
    got = B.process_and_flush_batch_device([r], [x], [s["frames"]], [y], [y.shape[0]], [UP])
    torch.cuda.synchronize()
    assert got[0][0] == s["frames"] and r.c.flags & FLUSHED and r.last_gathered() == 1


@pytest.mark.parametrize("width", [32, 64])
def test_refusals_enqueue_nothing(width):
    import ctypes as C
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    L = B.lib()
    dt, tdt = (np.float32, torch.float32) if width == 32 else (np.float64, torch.float64)
    ch, T = 2, 380
    rs = [B.Resampler(ch, T, T, 0.0, BH | IN | EXTRAP) for _ in range(3)]
    for r in rs:
        r.advance(T / 2)
    x = torch.from_numpy(tonal(2000, ch, dt)).cuda()
    sentinel = -12345.5
    ys = [torch.full((4000, ch), sentinel, dtype=tdt, device="cuda") for _ in rs]
    states = [r.state() for r in rs]
    errors = L.artamdErrorCount()
    res = (B.ResampleResult * 3)()
    arr = lambda ps: (C.c_void_p * 3)(*ps)
    ins, outs = arr([x.data_ptr()] * 3), arr([y.data_ptr() for y in ys])
    nin, caps, ratios = (C.c_int * 3)(2000, 2000, 2000), (C.c_int * 3)(4000, 4000, 4000), (C.c_double * 3)(UP, UP, UP)
    p = [C.cast(r.p, C.c_void_p).value for r in rs]
    assert L.resampleProcessAndFlushBatchInterleavedDevice(arr(p), 0, ins, nin, outs, caps, ratios, res) == 0
    assert L.resampleProcessAndFlushBatchInterleavedDevice(arr(p), -1, ins, nin, outs, caps, ratios, res) == 0
    assert L.resampleProcessAndFlushBatchInterleavedDevice(arr([p[0], p[1], p[0]]), 3, ins, nin, outs, caps, ratios, res) == -1
    assert L.resampleProcessAndFlushBatchInterleavedDevice(arr([p[0], None, p[2]]), 3, ins, nin, outs, caps, ratios, res) == -1
    torch.cuda.synchronize()
    assert [r.state() for r in rs] == states
    assert all(bool((y == sentinel).all()) for y in ys)
    assert L.artamdErrorCount() == errors
    # ... and the same lists, in order, are then made
    assert L.resampleProcessAndFlushBatchInterleavedDevice(arr(p), 3, ins, nin, outs, caps, ratios, res) == 0
    torch.cuda.synchronize()
    assert all(r.c.flags & FLUSHED and r.last_gathered() == 1 for r in rs)
    assert all(res[i].input_used == 2000 and res[i].output_generated > 2000 for i in range(3))


# The timing: 1,024 stereo 380-tap EXTRAPOLATE_ENDPOINTS clips of 4,000 tonal frames, 44.1 -> 16 kHz, wall medians of 5 repetitions behind a
# warm-up, contexts re-armed (reset, advance) outside the timed window.
# The loop of single calls is serial on its stream and costs two rounds of LPC fits per clip, 65 to 210 ms with the clips' samples, the same at
# 16 and at 64 clips, with the parent commit's library and with this tree's (profiles/flush_batch.txt) — 1,024 clips are 1.1 to 3.5
# minutes a repetition, up to 21 minutes for this test.  So the loop is timed over the first LOOP_CLIPS clips of the same 1,024 and the two are compared per
# clip; the batched call is timed over all 1,024.  (The in-test loop stands in for the parent commit's: the single-call path is what it
# was, and the profile shows the two loops side by side.)
# Measured on one MI355X (gfx950, 256 CUs; profiles/flush_batch.txt, the same shape): loop 140.5 ms per clip with the parent commit's
# library and 140.6 with this tree's (64 clips), batched 0.298 ms per clip (1,024 clips): 471 x.  FACTOR is below half of that, with room for
# the fits' dependence on the clips' samples (this test's own clips on the same kind of box: loop 64.9 ms per clip, batched 0.097 ms: 670 x).
CLIPS, LOOP_CLIPS, CLIP_FRAMES, REPS = 1024, 64, 4000, 5
FACTOR = 100.0


def test_z_timing_1024_stereo_extrapolating_clips_against_the_loop():
    torch = pytest.importorskip("torch")
    B = A.binding(32)
    ch, T = 2, 380
    rs = [B.Resampler(ch, T, T, 0.0, BH | IN | EXTRAP) for _ in range(CLIPS)]
    base = torch.from_numpy(tonal(CLIP_FRAMES + CLIPS, ch, np.float32, seed=5)).cuda()
    xs = [base[i:i + CLIP_FRAMES] for i in range(CLIPS)]              # (clip i: frames [i, i + 4000) of one signal — every clip ends on other samples)
    cap = int(CLIP_FRAMES * DOWN) + 2 * T
    ys = [torch.zeros(cap, ch, device="cuda") for _ in range(CLIPS)]
    yl = [torch.zeros(cap, ch, device="cuda") for _ in range(LOOP_CLIPS)]

    def arm(count):
        for r in rs[:count]:
            r.reset(); r.advance(T / 2)
        torch.cuda.synchronize()

    def batched():
        return B.process_and_flush_batch_device(rs, xs, [CLIP_FRAMES] * CLIPS, ys, [cap] * CLIPS, [DOWN] * CLIPS)

    def looped():
        return [r.process_device(x, CLIP_FRAMES, y, cap, DOWN, and_flush=True) for r, x, y in zip(rs[:LOOP_CLIPS], xs, yl)]

    times = {"batched": [], "loop": []}
    results = {}
    for rep in range(REPS + 1):                         # (one warm-up round each)
        for name, fn, count in (("batched", batched, CLIPS), ("loop", looped, LOOP_CLIPS)):
            arm(count)
            t0 = time.perf_counter()
            results[name] = fn()
            torch.cuda.synchronize()
            if rep:
                times[name].append(time.perf_counter() - t0)
    assert results["batched"][:LOOP_CLIPS] == results["loop"]
    made = results["loop"][0][1]
    assert all(np.array_equal(bits(ys[i][:made].cpu().numpy()), bits(yl[i][:made].cpu().numpy())) for i in range(LOOP_CLIPS))
    tb, tl = float(np.median(times["batched"])) / CLIPS, float(np.median(times["loop"])) / LOOP_CLIPS
    print(f"per clip: batched {tb * 1e3:.3f} ms ({CLIPS} clips), loop {tl * 1e3:.3f} ms ({LOOP_CLIPS} clips), ratio {tl / tb:.1f}")
    assert tl / tb >= FACTOR, (tl, tb)
