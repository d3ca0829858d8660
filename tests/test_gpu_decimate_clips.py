"""GPU: decimateProcessClipsPlanarLEDevice — many contexts' clips from a fresh start in the batch entry's shared launches, with a
clip count per item written by the launches.  Everything is exact — bytes, sentinels around the written runs, per-item counts,
running totals, host mirrors, and what the next calls make of the state — against fresh twin Decimators making the single planar
calls (which tests/test_gpu_decimate_planar.py and tests/test_gpu_parity.py pin to the reference's goldens)."""
import ctypes as C

import numpy as np
import pytest
import torch

import audio_resampler_amd as A
from test_gpu_decimate_planar import Buffers, SENTINEL, _dtype, _mirrors
from test_oracle_golden import decimate_input

pytestmark = pytest.mark.gpu

S1, S3, SATH = A.SHAPING_1ST_ORDER, A.SHAPING_3RD_ORDER, A.SHAPING_ATH_CURVE
HP, FLAT, LP = A.DITHER_HIGHPASS, A.DITHER_FLAT, A.DITHER_LOWPASS

# One list, ten contexts, eight classes: time-parallel without / with dither (items 0, 6 / 1), the serial wave without shaping for
# calls under 64 frames without / with dither (8 / 2, 7), 1st order + flat dither (3), ATH + high-pass dither (4, 9), 3rd order without
# dither (5).  Frames: every count of {0, 1, 31, 33, 63, 64, 65, 97, 4099} (item 9 has 0 frames in the second round).  Gains: 3.0
# clips the input (|x| up to 0.95 and two runs of 1.5), 0.25 cannot.
SPECS = [
    dict(ch=2, bits=16, nbytes=2, flags=0, frames=4099, gain=3.0, rate=48000, sides="pp"),
    dict(ch=3, bits=24, nbytes=3, flags=FLAT, frames=97, gain=1.0, rate=48000, sides="pi"),
    dict(ch=1, bits=8, nbytes=1, flags=HP, frames=63, gain=3.0, rate=48000, sides="ii"),
    dict(ch=2, bits=20, nbytes=3, flags=FLAT | S1, frames=65, gain=1.0, rate=96000, sides="ip"),
    dict(ch=3, bits=16, nbytes=2, flags=HP | SATH, frames=4099, gain=3.0, rate=44100, sides="pp"),
    dict(ch=2, bits=24, nbytes=4, flags=S3, frames=33, gain=0.25, rate=48000, sides="pp"),
    dict(ch=1, bits=16, nbytes=2, flags=0, frames=64, gain=1.0, rate=48000, sides="ii"),
    dict(ch=2, bits=24, nbytes=3, flags=LP, frames=31, gain=3.0, rate=48000, sides="pp"),
    dict(ch=3, bits=8, nbytes=1, flags=0, frames=1, gain=1.0, rate=48000, sides="pi"),
    dict(ch=2, bits=16, nbytes=2, flags=HP | SATH, frames=65, gain=3.0, rate=44100, sides="pp"),
]
ZERO_IN_B = 9                                      # this item has no frames in the second round: its context is only put back


def _specs(rnd):
    out = [dict(s) for s in SPECS]
    if rnd == "B":
        out[ZERO_IN_B]["frames"] = 0
    return out


_INPUT = {}


def _data(M, rnd, specs):
    """item i's planes [C, T]: a run of the decimator golden's input (decimate_input), from a place of its own per round and item"""
    dt = _dtype(M)
    if dt not in _INPUT:
        _INPUT[dt] = torch.from_numpy(decimate_input()[2]).to(dt).cuda()
    base = _INPUT[dt]
    out = []
    for i, s in enumerate(specs):
        n = s["ch"] * max(s["frames"], 1)
        at = (ord(rnd[0]) * 977 + len(rnd) * 389 + i * 131) % 1000
        idx = (at + torch.arange(n, device="cuda")) % base.numel()
        out.append(base[idx].view(s["ch"], -1)[:, :s["frames"]])
    return out


def _make(M, specs):
    return [M.Decimator(s["ch"], s["bits"], s["nbytes"], s["gain"], s["rate"], s["flags"]) for s in specs]


def _twins_call(twins, specs, xs):
    b = Buffers(specs, xs)
    for i, d in enumerate(twins):
        d.process_planar_device(b.ins[i], b.ipitch[i], specs[i]["frames"], b.outs[i], b.opitch[i])
    return b


def _pool_call(M, pool, specs, xs, from_start, counts=None, sync=False):
    a = Buffers(specs, xs)
    if sync:                                       # (the buffers are filled on the default stream: for a context on another one)
        torch.cuda.synchronize()
    rc = M.decimate_clips_planar_device(pool, a.ins, a.ipitch, [s["frames"] for s in specs], a.outs, a.opitch, from_start=from_start,
                                        d_clip_counts=counts)
    return a, rc


def _raw_mirrors(d):
    """the host mirrors as they stand (no call in between)"""
    p, ch = d.p.contents, d.channels
    out = [np.ctypeslib.as_array(p.feedback, (ch,)).copy().view(np.uint8)]
    if p.tpdf_generators:
        out.append(np.ctypeslib.as_array(p.tpdf_generators, (ch,)).copy().view(np.uint8))
    if p.noise_shapers:
        out.append(np.frombuffer(C.string_at(p.noise_shapers, C.sizeof(A.Biquad) * ch), np.uint8).copy())
    return out


def _equal_mirrors(us, vs):
    return len(us) == len(vs) and all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(us, vs))


def _same_bytes(a, b, what):
    torch.cuda.synchronize()
    assert a.untouched_outside() and b.untouched_outside(), what
    assert torch.equal(a.slab, b.slab), what       # (the same layout on both sides: the written runs and the sentinels around them)


def _three_rounds(M, warm):
    """warm: rounds on data A before the from-start round (the second one continues the first, so the time-parallel contexts stand
    with either of their two generator arrays live)"""
    pool = _make(M, SPECS)
    counts = torch.full((len(SPECS),), 7, dtype=torch.int64, device="cuda")
    twins_a = _make(M, SPECS)
    for k in range(warm):                          # ---- round 1: dirties the pool
        specs, rnd = _specs("A"), "A" * (k + 1)
        xs = _data(M, rnd, specs)
        a, rc = _pool_call(M, pool, specs, xs, from_start=(k == 0), counts=counts if k == 0 else None)
        _same_bytes(a, _twins_call(twins_a, specs, xs), (warm, rnd))
        assert rc >= 1
        for d in pool + twins_a:                   # (a host-pointer call: the host mirrors are no fresh context's any more)
            _mirrors(d)
    total_a = [d.clipped() for d in twins_a]
    assert [d.clipped() for d in pool] == total_a
    assert sum(t > 0 for t in total_a) >= 2

    twins_b = _make(M, SPECS)                      # ---- round 2: from the start again, on a dirty pool
    specs = _specs("B")
    xs = _data(M, "B", specs)
    a, rc = _pool_call(M, pool, specs, xs, from_start=True, counts=counts)
    _same_bytes(a, _twins_call(twins_b, specs, xs), (warm, "B"))
    clips_b = [d.clipped() for d in twins_b]
    live = [c for c, s in zip(clips_b, specs) if s["frames"] > 0]
    assert sum(c > 0 for c in live) >= 2 and any(c == 0 for c in live), clips_b      # (the twins: clipped items and one with none)
    assert clips_b[ZERO_IN_B] == 0
    assert counts.tolist() == clips_b, (warm, counts.tolist(), clips_b)
    assert [d.clipped() for d in pool] == [x + y for x, y in zip(total_a, clips_b)]
    for i, (d, t) in enumerate(zip(pool, twins_b)):
        assert _equal_mirrors(_raw_mirrors(d), _raw_mirrors(t)), (warm, i)

    specs = _specs("C")                            # ---- round 3: the state goes on as the twins' does
    xs = _data(M, "C", specs)
    a, rc3 = _pool_call(M, pool, specs, xs, from_start=False, counts=counts)
    _same_bytes(a, _twins_call(twins_b, specs, xs), (warm, "C"))
    clips_c = [d.clipped() - b for d, b in zip(twins_b, clips_b)]
    assert counts.tolist() == clips_c, (warm, counts.tolist(), clips_c)
    assert [d.clipped() for d in pool] == [x + y + z for x, y, z in zip(total_a, clips_b, clips_c)]
    specs = _specs("D")                            # ... and once more through the batch entry itself (neither fromStart nor counts)
    xs = _data(M, "D", specs)
    a, rc4 = _pool_call(M, pool, specs, xs, from_start=False)
    _same_bytes(a, _twins_call(twins_b, specs, xs), (warm, "D"))
    assert rc3 == rc4 + 1                          # (clearing the counts is the one operation more)
    for i, (d, t) in enumerate(zip(pool, twins_b)):         # the device state, through a host-pointer call that reads it back
        assert _equal_mirrors(_mirrors(d), _mirrors(t)), (warm, i)
    for d in pool + twins_a + twins_b:
        d.close()


@pytest.mark.parametrize("warm", [1, 2])
def test_three_rounds_equal_fresh_twins(warm):
    _three_rounds(A, warm)


def test_three_rounds_equal_fresh_twins_wide_build():
    _three_rounds(A.wide(), 1)


def test_side_contexts_and_their_counts(monkeypatch):
    """a context on another stream and a DECIMATE_MULTITHREADED context in two shards, between gathered ones: their own reset, their
    single call, their count uploaded"""
    specs = [dict(ch=2, bits=16, nbytes=2, flags=HP | SATH, frames=97, gain=3.0, rate=48000, sides="pp"),
             dict(ch=3, bits=24, nbytes=3, flags=FLAT | S1, frames=65, gain=3.0, rate=48000, sides="pp"),
             dict(ch=4, bits=20, nbytes=3, flags=FLAT, frames=4099, gain=3.0, rate=48000, sides="pp"),
             dict(ch=2, bits=16, nbytes=2, flags=0, frames=64, gain=3.0, rate=48000, sides="ip")]
    pool = _make(A, specs[:2])
    monkeypatch.setenv("ARTAMD_SHARDS", "2")
    pool.append(A.Decimator(4, 20, 3, 3.0, 48000, FLAT | A.DECIMATE_MULTITHREADED))
    monkeypatch.delenv("ARTAMD_SHARDS")
    assert pool[2].shards() == 2
    pool += _make(A, specs[3:])
    side = torch.cuda.Stream()
    pool[1].set_stream(side.cuda_stream)
    counts = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    totals = [0] * 4
    for rnd in ("A", "B"):
        twins = _make(A, specs)
        xs = _data(A, rnd, specs)
        a, rc = _pool_call(A, pool, specs, xs, from_start=True, counts=counts, sync=True)
        side.synchronize()
        _same_bytes(a, _twins_call(twins, specs, xs), rnd)
        clips = [d.clipped() for d in twins]
        assert sum(c > 0 for c in clips) >= 2, clips
        assert counts.tolist() == clips, rnd
        totals = [t + c for t, c in zip(totals, clips)]
        assert [d.clipped() for d in pool] == totals, rnd
        for i, (d, t) in enumerate(zip(pool, twins)):
            assert _equal_mirrors(_raw_mirrors(d), _raw_mirrors(t)), (rnd, i)
        for d in twins:
            d.close()
    for d in pool:
        d.close()


def test_launch_count_does_not_grow_with_the_list():
    s = dict(ch=2, bits=16, nbytes=2, flags=HP | SATH, frames=97, gain=1.0, rate=44100, sides="pp")
    made = {}
    for n in (2, 40):
        specs = [dict(s) for _ in range(n)]
        pool = _make(A, specs)
        xs = _data(A, "A", specs)
        counts = torch.zeros(n, dtype=torch.int64, device="cuda")
        a = Buffers(specs, xs)
        batch = A.decimate_batch_planar_device(pool, a.ins, a.ipitch, [97] * n, a.outs, a.opitch)
        _, plain = _pool_call(A, pool, specs, xs, from_start=True)
        _, counted = _pool_call(A, pool, specs, xs, from_start=True, counts=counts)
        torch.cuda.synchronize()
        made[n] = (batch, plain, counted)
        for d in pool:
            d.close()
    assert made[2] == made[40], made
    batch, plain, counted = made[2]
    assert batch == 1 and plain == batch and counted == batch + 1, made


def test_duplicate_context_is_refused_and_nothing_moves():
    specs = [dict(SPECS[4]), dict(SPECS[1])]
    pool, twins = _make(A, specs), _make(A, specs)
    xs = _data(A, "A", specs)
    a, _ = _pool_call(A, pool, specs, xs, from_start=True)
    _same_bytes(a, _twins_call(twins, specs, xs), "A")
    totals = [d.clipped() for d in pool]
    before = [_raw_mirrors(d) for d in pool]
    counts = torch.full((3,), 7, dtype=torch.int64, device="cuda")
    errors = A.lib().artamdErrorCount()
    dup = Buffers(specs + specs[:1], xs + xs[:1])
    with pytest.raises(RuntimeError):
        A.decimate_clips_planar_device(pool + pool[:1], dup.ins, dup.ipitch, [s["frames"] for s in specs + specs[:1]], dup.outs, dup.opitch,
                                       from_start=True, d_clip_counts=counts)
    torch.cuda.synchronize()
    assert bool(torch.all(dup.slab == SENTINEL)) and counts.tolist() == [7, 7, 7]
    assert A.lib().artamdErrorCount() == errors
    assert [d.clipped() for d in pool] == totals
    for d, m in zip(pool, before):
        assert _equal_mirrors(_raw_mirrors(d), m)
    xs = _data(A, "C", specs)                       # the contexts go on from where round A left them
    a, _ = _pool_call(A, pool, specs, xs, from_start=False)
    _same_bytes(a, _twins_call(twins, specs, xs), "C")
    for d in pool + twins:
        d.close()


def test_clip_decimator_launches_do_not_grow_with_the_batch():
    made = {}
    for B in (2, 40):
        x = torch.rand(B, 2, 300, generator=torch.Generator(device="cuda").manual_seed(B), device="cuda") * 3.0 - 1.5
        cd = A.ClipDecimator(2, 16, 2, 1.0, 48000, HP | SATH)
        pcm, clipped = cd(x)
        assert clipped.dtype == torch.int64 and not clipped.is_cuda and int(clipped.sum()) > 0
        made[B] = cd.launches
        pcm2, clipped2 = cd(x)                      # the pool starts afresh
        assert torch.equal(pcm, pcm2) and torch.equal(clipped, clipped2) and cd.launches == made[B]
        cd.close()
    assert made[2] == made[40] == 2, made           # the clearing of the counts and one serial class
