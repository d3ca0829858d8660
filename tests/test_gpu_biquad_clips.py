"""biquadBankApplyClipsPlanarDevice: many banks' calls, the long time-parallel ones in shared launches.  Everything is bit-exact:
the twin of every item is its own single planar call on a twin bank (which test_gpu_biquad_planar.py pins to the interleaved entry
and that one's tests to the oracle), and the comparison is equality of bytes, of the state biquadBankRead returns and of the growth
of biquadBankRepairs.

The shapes follow each filter's own chunk length L (pcm_host.c: forget_length, spec_chunk), which _chunk mirrors on the host; a call
is time-parallel from 2 L frames on, and gathered into the shared launches above the batch entry's serial bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import audio_resampler_amd as A
import test_gpu_biquad_batch as TB
import test_gpu_biquad_planar as TP
from _oracle import load_oracle, Biquad as OBiquad, BiquadCoeffs as OCoeffs, f32p

pytestmark = pytest.mark.gpu

Planes, _bits, _state, _signal, _dtype, _width = TP.Planes, TB._bits, TB._state, TP._signal, TP._dtype, TP._width
ROUND_LAUNCHES = 1 + 3                          # a round of one class: the copy launch, then spec, check and commit (art_hip.h)
_forget_cache = {}


def _forget(sec, wide):
    """pcm_host.c, forget_length: frames until every unit state of the recursive part has decayed below 2^-40 (2^-70 wide), + 16;
    0 beyond 1,024"""
    env = os.environ.get("ARTAMD_BIQUAD_WARMUP")
    order = sec.order
    if not 1 <= order <= 4:
        return 0
    if env:
        return int(env)
    key = (wide, order, tuple(sec.b))
    if key not in _forget_cache:
        floor, worst = 2.0 ** (-70 if wide else -40), 0
        for j in range(order):
            y, last = [0.0] * 4, 0
            y[j] = 1.0
            for n in range(1, 1024 + 64 + 1):
                v = 0.0
                for k in range(1, order + 1):
                    v -= float(sec.b[k]) * y[k - 1]
                y = [v, y[0], y[1], y[2]]
                if not abs(v) <= floor:
                    last = n
            worst = max(worst, last)
        _forget_cache[key] = 0 if worst > 1024 else worst + 16
    return _forget_cache[key]


def _chunk(M, secs, S):
    """the chunk length of a bank's time-parallel form (spec_chunk of the largest warm-up of its sections); 0: serial kernels only"""
    W = 1
    for sec in secs:
        w = _forget(sec, _width(M) == 64)
        if not w:
            return 0
        W = max(W, w)
    return min(max((4 * S * W + 7) & ~7, 128), 8192)


def _spec(M, ch, S, kind, frames, planar=True, extra=0, offset=0, odd=False):
    """frames: a number, or a function of (L, serial bound); odd: the pitch (frames + extra) made odd by one more sample"""
    L, smax = _chunk(M, TB._sections(M, ch, S, kind), S), TB._serial_max(M)
    n = frames(L, smax) if callable(frames) else frames
    extra += odd and not (n + extra) % 2
    return dict(ch=ch, S=S, kind=kind, frames=n, planar=planar, extra=extra, offset=offset, L=L,
                gathered=bool(L) and n >= 2 * L and n > smax)


def _bank(M, s, multi=False):
    return M.BiquadBank(TB._sections(M, s["ch"], s["S"], s["kind"]), s["ch"], s["S"], multi=multi)


def _mixed_specs(M):
    two, two1, ragged, below = (lambda L, m: 2 * L), (lambda L, m: 2 * L + 1), (lambda L, m: 5 * L + 3), (lambda L, m: 2 * L - 1)
    over = lambda L, m: m + 1
    return [
        _spec(M, 2, 1, "pre", two, extra=1), _spec(M, 3, 1, "hand", ragged, extra=7, offset=1), _spec(M, 1, 1, "post", two1, offset=1),
        _spec(M, 8, 1, "hp", two, planar=False),
        _spec(M, 2, 2, "pre", ragged, extra=3, offset=1, odd=True), _spec(M, 8, 2, "post", two, planar=False, offset=1), _spec(M, 33, 2, "hp", two1, extra=5, odd=True),
        _spec(M, 2, 2, "pre", below, extra=1), _spec(M, 2, 2, "post", 441, extra=2), _spec(M, 3, 1, "pre", over, extra=1),
        _spec(M, 2, 2, "narrow", 3000, extra=1),
        _spec(M, 3, 3, "pre", two, extra=2), _spec(M, 2, 3, "hand", ragged, planar=False), _spec(M, 33, 3, "post", two1, extra=1, offset=1),
        _spec(M, 8, 4, "hand", ragged, extra=9), _spec(M, 2, 4, "post", ragged, extra=1), _spec(M, 2, 4, "pre", two, planar=False),
        _spec(M, 2, 4, "hand", 1, extra=4), _spec(M, 2, 1, "pre", 0), _spec(M, 3, 3, "hand", 1),
    ]


def _corner_specs(M):
    return [_spec(M, 2, 2, "pre", lambda L, m: 2 * L, extra=0), _spec(M, 3, 2, "pre", lambda L, m: 5 * L + 3, extra=7, offset=1, odd=True),
            _spec(M, 8, 3, "post", lambda L, m: 2 * L + 1, planar=False, offset=1), _spec(M, 2, 1, "hand", lambda L, m: 5 * L + 3, extra=1),
            _spec(M, 2, 2, "post", 441, extra=1), _spec(M, 2, 2, "narrow", 700)]


def _clips_call(M, round_bytes=0):
    """the entry, or its private form with a byte bound per round"""
    if not round_bytes:
        return M.biquad_clips_planar_device
    fn = M.lib().artamd_biquad_clips_planar
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_long]

    def call(banks, bufs, pitches, frames, from_start=False):
        n = len(banks)
        rc = fn((C.c_void_p * n)(*[b.p for b in banks]), n, (C.c_void_p * n)(*[int(p) for p in bufs]),
                (C.c_long * n)(*[int(p) for p in pitches]), (C.c_int * n)(*[int(f) for f in frames]), int(from_start), round_bytes)
        assert rc >= 0
        return rc
    return call


def _lay(s, x):
    """an item's buffer: planes, or interleaved frames between sentinels (one plane, transposed)"""
    if s["planar"]:
        return Planes(x, s["frames"] + s["extra"], s["offset"])
    return Planes(x.t().contiguous().view(1, -1), s["frames"] * s["ch"], s["offset"])


def _clips_equal_loop(M, specs, call=None, ticks=2, from_start=False, banks=None, twins=None, seed=0):
    """the entry on one set of banks against the loop of single planar calls on twins (reset first with from_start): bytes, padding,
    states and the growth of the repairs, tick after tick.  Returns the return values and the repairs' growth per tick."""
    call = call or M.biquad_clips_planar_device
    own = banks is None
    banks = banks or [_bank(M, s) for s in specs]
    twins = twins or [_bank(M, s) for s in specs]
    frames = [s["frames"] for s in specs]
    pitch = lambda s, p: p.pitch if s["planar"] else 0
    rcs, grown = [], []
    for tick in range(ticks):
        xs = [_signal(s["ch"], s["frames"], seed + 100 * tick + i, _dtype(M)) for i, s in enumerate(specs)]
        mine, loop = [_lay(s, x) for s, x in zip(specs, xs)], [_lay(s, x) for s, x in zip(specs, xs)]
        before = [(b.repairs(), t.repairs()) for b, t in zip(banks, twins)]
        torch.cuda.synchronize()                 # (a bank on a stream of its own: the buffers are filled)
        rcs.append(call(banks, [p.ptr for p in mine], [pitch(s, p) for s, p in zip(specs, mine)], frames, from_start=from_start))
        for s, t, p in zip(specs, twins, loop):
            if from_start:
                t.reset()
            t.apply_planar_device(p.ptr, pitch(s, p), s["frames"])
        torch.cuda.synchronize()
        grown.append([])
        for i, s in enumerate(specs):
            what = (_width(M), tick, i, s)
            assert mine[i].padding_untouched() and loop[i].padding_untouched(), what
            assert torch.equal(_bits(mine[i].buf), _bits(loop[i].buf)), what
            assert _state(banks[i]) == _state(twins[i]), what
            g, w = banks[i].repairs() - before[i][0], twins[i].repairs() - before[i][1]
            assert g == w, what
            grown[-1].append(g)
    if own:
        for b in banks + twins:
            b.close()
    return rcs, grown


def _assert_the_mixed_specs_have_every_case(M, specs):
    smax = TB._serial_max(M)
    assert {s["S"] for s in specs} == {1, 2, 3, 4} and {s["ch"] for s in specs} >= {1, 2, 3, 8, 33}
    assert {s["kind"] for s in specs} == {"pre", "post", "hp", "hand", "narrow"}
    tp = [s for s in specs if s["gathered"]]
    for S in (1, 2, 3, 4):                       # lanes of items with different L and K in one launch
        mine = [s for s in tp if s["S"] == S]
        assert len(mine) >= 2 and len({(s["L"], -(-s["frames"] // s["L"])) for s in mine}) >= 2, S
    assert any(s["frames"] == 2 * s["L"] for s in tp) and any(s["frames"] == 2 * s["L"] + 1 for s in tp)
    assert any(s["frames"] == 5 * s["L"] + 3 for s in tp)
    assert any(s["L"] and s["frames"] == 2 * s["L"] - 1 and s["frames"] > smax and not s["gathered"] for s in specs)     # serial whatever the bound
    assert any(s["frames"] == smax + 1 and s["gathered"] for s in specs)           # the first count the batch entry leaves aside
    assert {0, 1, 441} <= {s["frames"] for s in specs}
    assert any(s["kind"] == "narrow" and s["L"] == 0 and s["frames"] == 3000 for s in specs)
    assert any(s["planar"] and s["ch"] > 1 and (s["frames"] + s["extra"]) % 2 and s["gathered"] for s in specs)     # odd pitch
    assert any(s["planar"] and s["offset"] == 1 and s["gathered"] for s in specs)   # base off 16 bytes by one sample
    assert any(not s["planar"] and s["ch"] > 1 and s["gathered"] for s in specs) and any(s["ch"] == 1 and s["gathered"] for s in specs)


def test_the_host_mirror_of_the_chunk_length_is_the_librarys():
    """two stereo planar items of one shape: the gathered launches (a round of one class) from 2 L frames on and above the serial
    bound, one serial launch below; one such item alone is its single call, one launch either way"""
    smax = TB._serial_max(A)
    for S, kind in ((1, "pre"), (2, "pre"), (2, "post"), (3, "hp"), (4, "hand"), (2, "narrow")):
        for frames in (lambda L, m: max(2 * L, m + 1), lambda L, m: max(2 * L - 1, 1) if 2 * L - 1 > m else m):
            s = _spec(A, 2, S, kind, frames, extra=1)
            assert s["gathered"] == (s["frames"] > smax and s["L"] > 0 and s["frames"] >= 2 * s["L"])
            banks = [_bank(A, s), _bank(A, s)]
            ps = [_lay(s, _signal(2, s["frames"], k, torch.float32)) for k in range(2)]
            rc = A.biquad_clips_planar_device(banks, [p.ptr for p in ps], [p.pitch for p in ps], [s["frames"]] * 2)
            alone = A.biquad_clips_planar_device(banks[:1], [ps[0].ptr], [ps[0].pitch], [s["frames"]])
            torch.cuda.synchronize()
            assert rc == (ROUND_LAUNCHES if s["gathered"] else 1) and alone == 1, s
            for b in banks:
                b.close()


def test_mixed_batch_equals_the_loop_of_single_planar_calls():
    specs = _mixed_specs(A)
    _assert_the_mixed_specs_have_every_case(A, specs)
    rcs, _ = _clips_equal_loop(A, specs, ticks=2)
    classes = {(s["S"], s["planar"] and s["ch"] > 1) for s in specs if s["gathered"]}
    serial = {s["S"] for s in specs if s["frames"] > 0 and not s["gathered"]}
    assert rcs == [1 + 3 * len(classes) + len(serial)] * 2


def test_verification_and_repair(monkeypatch):
    """a warm-up far too short: nearly every chunk boundary mismatches and is repaired, on both sides alike"""
    monkeypatch.setenv("ARTAMD_BIQUAD_WARMUP", "2")
    over = lambda L, m: m + 1 + 3 * L + 5                  # L is the 128-frame floor here: several chunks, above the serial bound
    specs = [_spec(A, 2, 1, "pre", over, extra=1), _spec(A, 3, 2, "pre", over, extra=2, offset=1), _spec(A, 8, 2, "hp", over, planar=False),
             _spec(A, 2, 3, "post", over), _spec(A, 33, 4, "hand", over, extra=3), _spec(A, 1, 2, "post", over)]
    assert all(s["L"] == 128 and s["gathered"] for s in specs)
    banks, twins = [_bank(A, s) for s in specs], [_bank(A, s) for s in specs]
    monkeypatch.delenv("ARTAMD_BIQUAD_WARMUP")
    _, grown = _clips_equal_loop(A, specs, ticks=2, banks=banks, twins=twins)
    assert all(g > 0 for tick in grown for g in tick), grown
    for b in banks + twins:
        b.close()


def test_from_start():
    specs = [_spec(A, 2, 2, "pre", lambda L, m: 5 * L + 3, extra=1), _spec(A, 3, 1, "post", lambda L, m: 2 * L, extra=2),
             _spec(A, 2, 2, "post", 441, extra=1), _spec(A, 8, 1, "pre", lambda L, m: m + 1, planar=False), _spec(A, 2, 2, "narrow", 600),
             _spec(A, 2, 4, "hand", 1), _spec(A, 2, 2, "pre", 0)]
    assert sum(s["gathered"] for s in specs) == 3
    banks, twins = [_bank(A, s) for s in specs], [_bank(A, s) for s in specs]
    fresh = [_state(b) for b in banks]
    # dirty them: the skipped item's bank too (by a call of its own)
    _clips_equal_loop(A, specs, ticks=1, banks=banks, twins=twins)
    for b in (banks[-1], twins[-1]):
        b.apply_device(_signal(2, 50, 3, torch.float32).t().contiguous(), 50)
    assert all(_state(b) != f for b, f in zip(banks, fresh))
    # continuing: equal to the continuing twins
    _clips_equal_loop(A, specs, ticks=1, banks=banks, twins=twins, seed=7)
    assert _state(banks[-1]) != fresh[-1]
    # from the start: equal to fresh banks (and to the reset twins)
    news = [_bank(A, s) for s in specs]
    _clips_equal_loop(A, specs, ticks=1, from_start=True, banks=banks, twins=news, seed=11)
    _clips_equal_loop(A, specs, ticks=1, from_start=True, banks=banks, twins=twins, seed=13)
    assert _state(banks[-1]) == fresh[-1]                  # skipped, and reset all the same
    for b in banks + twins + news:
        b.close()


def test_launch_count_does_not_grow_with_the_batch():
    rcs = []
    for n in (40, 2):
        specs = [_spec(A, 2, 2, "pre", lambda L, m: 5 * L, extra=i % 3) for i in range(n)]
        assert all(s["gathered"] for s in specs)
        rcs.append(_clips_equal_loop(A, specs, ticks=1, from_start=True)[0][0])
    assert rcs[0] == rcs[1] <= ROUND_LAUNCHES
    got = []
    for B in (8, 2):
        cf = A.ClipFilter(2, TP.ART_P)
        cf(_signal(B * 2, 3000, B, torch.float32).view(B, 2, 3000))
        got.append(cf.launches)
        cf.close()
    assert got[0] == got[1] and 0 < got[0] <= ROUND_LAUNCHES


def test_side_calls_and_refusals(monkeypatch):
    long = lambda L, m: max(2 * L, m + 1) + 5
    specs = [_spec(A, 2, 2, "pre", long, extra=1), _spec(A, 8, 2, "pre", long, extra=1), _spec(A, 2, 1, "post", long, extra=2),
             _spec(A, 2, 2, "post", 300, extra=1), _spec(A, 3, 2, "post", long, extra=1)]
    assert [s["gathered"] for s in specs] == [True, True, True, False, True]       # (two of them on the side all the same)
    monkeypatch.setenv("ARTAMD_SHARDS", "4")
    banks = [_bank(A, specs[0]), _bank(A, specs[1], multi=True)] + [_bank(A, s) for s in specs[2:]]
    monkeypatch.delenv("ARTAMD_SHARDS")
    assert banks[1].shards() == 4
    twins = [_bank(A, s) for s in specs]
    other = torch.cuda.Stream()
    banks[2].set_stream(other.cuda_stream)
    for from_start in (False, True):
        rcs, _ = _clips_equal_loop(A, specs, ticks=1, from_start=from_start, banks=banks, twins=twins, seed=int(from_start))
        assert rcs == [1 + 1 + ROUND_LAUNCHES + 1]          # two on the side, one gathered round (its copy resets the serial bank), one serial
    # refusals: nothing enqueued, nothing counted, nothing changed
    L = A.lib()
    ps = [_lay(s, _signal(s["ch"], s["frames"], 9 + i, torch.float32)) for i, s in enumerate(specs)]
    before, states, errors = [p.buf.clone() for p in ps], [_state(b) for b in banks], L.artamdErrorCount()
    ptrs, pitches, frames = [p.ptr for p in ps], [p.pitch for p in ps], [s["frames"] for s in specs]
    for from_start in (False, True):
        with pytest.raises(RuntimeError):
            A.biquad_clips_planar_device(banks + banks[:1], ptrs + ptrs[:1], pitches + pitches[:1], frames + frames[:1], from_start=from_start)
        n = 2
        assert L.biquadBankApplyClipsPlanarDevice((C.c_void_p * n)(banks[0].p, None), n, (C.c_void_p * n)(*ptrs[:2]), (C.c_long * n)(*pitches[:2]),
                                                  (C.c_int * n)(*frames[:2]), int(from_start)) == -1
    torch.cuda.synchronize()
    assert L.artamdErrorCount() == errors and [_state(b) for b in banks] == states
    for p, b in zip(ps, before):
        assert torch.equal(_bits(p.buf), _bits(b))
    for b in banks + twins:
        b.close()


def test_eight_art_low_pass_clips_against_the_oracle():
    """ART's two-section pre-filter on eight stereo clips of differing lengths above 2 L; every plane against the reference's recurrence"""
    OL = load_oracle()
    ch = 2
    s0 = _spec(A, ch, 2, "pre", 0)
    lengths = [2 * s0["L"] + 1 + 397 * i for i in range(8)]
    assert s0["L"] and min(lengths) > max(2 * s0["L"], TB._serial_max(A)) and len(set(lengths)) == 8
    co, oc = A.BiquadCoefficients(), OCoeffs()
    A.lib().biquad_lowpass(C.byref(co), TB.PRE)
    OL.ora_biquad_lowpass(C.byref(oc), TB.PRE)
    secs = (A.Biquad * (ch * 2))()
    for k in range(ch * 2):
        A.lib().biquad_init(C.byref(secs[k]), C.byref(co), 1.0)
    banks = [A.BiquadBank(secs, ch, 2) for _ in lengths]
    xs = [np.ascontiguousarray(np.random.default_rng(40 + i).random((ch, n), dtype=np.float32) * 2 - 1) for i, n in enumerate(lengths)]
    ps = [Planes(torch.from_numpy(x.copy()).cuda(), n + 1 + i, i % 2) for i, (x, n) in enumerate(zip(xs, lengths))]
    assert A.biquad_clips_planar_device(banks, [p.ptr for p in ps], [p.pitch for p in ps], lengths, from_start=True) == ROUND_LAUNCHES
    torch.cuda.synchronize()
    hist = lambda q, arr: [arr[(q.index - i) & 3] for i in range(4)]
    for i, (x, n) in enumerate(zip(xs, lengths)):
        osecs = [OBiquad() for _ in range(ch * 2)]
        for k in range(ch * 2):
            OL.ora_biquad_init(C.byref(osecs[k]), C.byref(oc), 1.0)
        for c in range(ch):
            for s in range(2):
                OL.ora_biquad_buffer(C.byref(osecs[c * 2 + s]), C.cast(x.ctypes.data + 4 * n * c, f32p), n, 1)
        assert np.array_equal(ps[i].clip().cpu().numpy().view(np.uint32), x.view(np.uint32)), i
        assert ps[i].padding_untouched(), i
        st = banks[i].read()
        for k in range(ch * 2):
            assert hist(st[k], st[k].x) == hist(osecs[k], osecs[k].x) and hist(st[k], st[k].y) == hist(osecs[k], osecs[k].y), (i, k)
    for b in banks:
        b.close()


def test_wide_build_corners_and_repairs(monkeypatch):
    W = A.wide()
    specs = _corner_specs(W)
    assert sum(s["gathered"] for s in specs) == 4 and any(not s["planar"] and s["gathered"] for s in specs)
    assert any(s["gathered"] and s["frames"] == 2 * s["L"] for s in specs) and any(s["gathered"] and s["frames"] % s["L"] for s in specs)
    assert any(s["gathered"] and s["planar"] and (s["frames"] + s["extra"]) % 2 for s in specs)
    _clips_equal_loop(W, specs, ticks=2)
    monkeypatch.setenv("ARTAMD_BIQUAD_WARMUP", "2")
    over = lambda L, m: m + 1 + 3 * L + 5
    specs = [_spec(W, 2, 2, "pre", over, extra=1, offset=1), _spec(W, 3, 3, "post", over, planar=False), _spec(W, 8, 1, "hand", over, extra=2)]
    banks, twins = [_bank(W, s) for s in specs], [_bank(W, s) for s in specs]
    monkeypatch.delenv("ARTAMD_BIQUAD_WARMUP")
    _, grown = _clips_equal_loop(W, specs, ticks=1, banks=banks, twins=twins)
    assert all(g > 0 for g in grown[0]), grown
    for b in banks + twins:
        b.close()


def test_three_scratch_rounds_equal_one(monkeypatch):
    """the byte bound per round lowered (the library's private form): the same batch in three rounds, with repairs on the way"""
    monkeypatch.setenv("ARTAMD_BIQUAD_WARMUP", "2")
    n = TB._serial_max(A) + 1 + 3 * 128
    specs = [_spec(A, 2, 2, "pre", n + 8 * i, extra=i % 2, offset=i % 2) for i in range(5)] + [_spec(A, 2, 2, "post", 200, extra=1)]
    ones, threes, twins = ([_bank(A, s) for s in specs] for _ in range(3))
    monkeypatch.delenv("ARTAMD_BIQUAD_WARMUP")
    item = 2 * (n + 8 * 4 + 4) * 4                          # bytes set aside for the largest item, at most
    one, g1 = _clips_equal_loop(A, specs, ticks=2, banks=ones, twins=twins)
    for t in twins:
        t.reset()
    three, g3 = _clips_equal_loop(A, specs, _clips_call(A, 2 * item), ticks=2, from_start=False, banks=threes, twins=twins)
    assert one == [ROUND_LAUNCHES + 1] * 2 and three == [3 * ROUND_LAUNCHES + 1] * 2       # (+ 1: the serial item's launch)
    assert g1 == g3 and all(g > 0 for g in g1[0][:5])
    for a, b in zip(ones, threes):
        assert _state(a) == _state(b)
    for b in ones + threes + twins:
        b.close()
