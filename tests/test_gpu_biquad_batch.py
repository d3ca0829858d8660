"""biquadBankApplyBatchInterleavedDevice: many biquad banks in one launch per section count.  Every bank's samples and state
afterwards are those of its own single device call on a twin bank, byte for byte, and the reference's recurrence (the oracle) holds
for ART's -p filters run batched."""
import ctypes as C
import statistics
import time

import numpy as np
import pytest
import torch

import audio_resampler_amd as A
from _oracle import load_oracle, Biquad as OBiquad, BiquadCoeffs as OCoeffs, f32p

pytestmark = pytest.mark.gpu

GAP = 37                                        # samples between two banks' buffers in the shared one
SENTINEL = 12345.5
PRE, POST = 44100 * 0.45 / 96000, 44100 * 0.45 / 48000       # ART's -p cut-offs, 96 -> 44.1 kHz and 44.1 -> 48 kHz
HAND = {1: dict(a0=0.2, a1=0.15, b1=-0.5),      # stable sections of every order (as test_gpu_biquad_parallel.py)
        2: dict(a0=0.2, a1=0.15, a2=0.1, b1=-0.5, b2=0.2),
        3: dict(a0=0.2, a1=0.15, a2=0.1, a3=-0.05, b1=-0.5, b2=0.2, b3=-0.1),
        4: dict(a0=0.2, a1=0.15, a2=0.1, a3=-0.05, a4=0.02, b1=-0.5, b2=0.2, b3=-0.1, b4=0.03)}


def _serial_max(M):
    fn = M.lib().artamd_biquad_batch_serial_max
    fn.restype, fn.argtypes = C.c_int, []
    return fn()


def _sections(M, ch, S, kind):
    """(M.Biquad * (ch * S)), channel-major.  kind: 'pre' / 'post' (ART's low-pass), 'hp' (a high-pass), 'narrow' (a low-pass that
    never forgets within the time-parallel form's cap: no warm-up), 'hand' (orders 1-4 by channel and section)"""
    L = M.lib()
    secs = (M.Biquad * (ch * S))()
    for c in range(ch):
        for s in range(S):
            co = M.BiquadCoefficients()
            if kind == "hand":
                co = M.BiquadCoefficients(**HAND[1 + (c + s) % 4])
            elif kind == "hp":
                L.biquad_highpass(C.byref(co), 0.02)
            else:
                L.biquad_lowpass(C.byref(co), {"pre": PRE, "post": POST, "narrow": 0.004}[kind])
            L.biquad_init(C.byref(secs[c * S + s]), C.byref(co), 0.9 if kind == "hand" else 1.0)
    return secs


def _pair(M, spec, multi=False):
    secs = _sections(M, spec["ch"], spec["S"], spec["kind"])
    return M.BiquadBank(secs, spec["ch"], spec["S"], multi=multi), M.BiquadBank(secs, spec["ch"], spec["S"])


class Layout:
    """every bank's buffer in one device buffer, with sentinel gaps between them"""
    def __init__(self, sizes, dtype):
        self.off, pos = [], GAP
        for s in sizes:
            self.off.append(pos)
            pos += s + GAP
        self.sizes = list(sizes)
        self.buf = torch.full((pos,), SENTINEL, dtype=dtype, device="cuda")

    def part(self, i):
        return self.buf[self.off[i]:self.off[i] + self.sizes[i]]

    def gaps_untouched(self):
        mask = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        for o, s in zip(self.off, self.sizes):
            mask[o:o + s] = False
        return bool(torch.all(self.buf[mask] == SENTINEL))


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _state(bank):
    return bytes(memoryview(bank.read()))


def _specs(M):
    """one bank per row: section counts 1-4, ART's filters, a high-pass, a narrow filter and hand-made orders 1-4, 1 to 33 channels;
    frame counts by tick (0 to 960 and one call just above the library's bound, which a narrow filter keeps in the batch)"""
    over = _serial_max(M) + 1
    chans = [1, 2, 6, 8, 33]
    kinds = ["pre", "post", "hp", "narrow", "hand", "hand"]
    frames = [0, 1, 3, 63, 64, 441, 960, 441, 960]
    out = []
    for i in range(30):
        f = [frames[(i + t) % 9] for t in range(4)]
        if i == 6:
            f[0] = max(over, 1200)               # ART's pre-filter, 3 sections: a time-parallel single call, made on the side
        if i == 9:
            f[1] = over                          # narrow: the single call is serial too, so it stays in the batch
        out.append(dict(ch=chans[i % 5], S=1 + i % 4, kind=kinds[i % 6], frames=f))
    return out


def _inputs(spec_frames, chans, tick, dtype):
    g = torch.Generator(device="cuda").manual_seed(4321 + tick)
    return [torch.rand(max(f, 1) * c, generator=g, device="cuda", dtype=dtype) * 2 - 1 for f, c in zip(spec_frames, chans)]


def _batch_equals_twins(M, dtype, specs, batch_call=None, ticks=4, single_ticks=(2,)):
    """ticks of the batch call on one set of banks against single calls on their twins; on the ticks in single_ticks the batch's
    banks take single calls too (batch and single calls alternating on the same banks)"""
    batch_call = batch_call or M.biquad_batch_device
    pairs = [_pair(M, s) for s in specs]
    banks, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    chans = [s["ch"] for s in specs]
    for tick in range(ticks):
        frames = [s["frames"][tick % len(s["frames"])] for s in specs]
        xs = _inputs(frames, chans, tick, dtype)
        lay = Layout([f * c for f, c in zip(frames, chans)], dtype)
        for i, x in enumerate(xs):
            lay.part(i).copy_(x[:lay.sizes[i]])
        wants = [x.clone() for x in xs]
        if tick in single_ticks:
            for i, b in enumerate(banks):
                b.apply_device(lay.part(i), frames[i])
        else:
            rc = batch_call(banks, [lay.part(i) for i in range(len(specs))], frames)
            present = {s["S"] for s, f in zip(specs, frames) if f > 0}
            assert 1 <= rc <= len(present) + sum(1 for f in frames if f > _serial_max(M)), rc
        for t, w, f in zip(twins, wants, frames):
            t.apply_device(w, f)
        torch.cuda.synchronize()
        assert lay.gaps_untouched(), tick
        for i, (w, f) in enumerate(zip(wants, frames)):
            assert torch.equal(_bits(lay.part(i)), _bits(w[:lay.sizes[i]])), (tick, i, specs[i])
        for i, (b, t) in enumerate(zip(banks, twins)):
            assert _state(b) == _state(t), (tick, i, specs[i])
    for b in banks + twins:
        b.close()


def _with_lanes(M, lanes, serial_max=-1):
    """the batch call with every class packed `lanes` lanes to a workgroup (the library's private form of the call)"""
    fn = M.lib().artamd_biquad_batch
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def call(banks, bufs, frames):
        n = len(banks)
        rc = fn((C.c_void_p * n)(*[b.p for b in banks]), n, (C.c_void_p * n)(*[t.data_ptr() for t in bufs]),
                (C.c_int * n)(*[int(f) for f in frames]), lanes, serial_max)
        if rc < 0:
            raise RuntimeError("artamd_biquad_batch failed")
        return rc
    return call


def test_mixed_batch_equals_single_call_twins_byte_for_byte():
    _batch_equals_twins(A, torch.float32, _specs(A), ticks=5, single_ticks=(2,))


def test_art_filters_against_the_oracle():
    """ART's pre-filter (960-frame ticks) and post-filter (441-frame ticks) banks, 64 stereo streams each, 5 ticks; every stream
    against the reference's recurrence on its own copy of the input"""
    OL = load_oracle()
    ch, n, ticks = 2, 64, 5
    banks, oracles, frames = [], [], []
    for j in range(2 * n):
        freq, f = (PRE, 960) if j < n else (POST, 441)
        co, oc = A.BiquadCoefficients(), OCoeffs()
        A.lib().biquad_lowpass(C.byref(co), freq)
        OL.ora_biquad_lowpass(C.byref(oc), freq)
        secs = (A.Biquad * (ch * 2))()
        osecs = [OBiquad() for _ in range(ch * 2)]
        for k in range(ch * 2):
            A.lib().biquad_init(C.byref(secs[k]), C.byref(co), 1.0)
            OL.ora_biquad_init(C.byref(osecs[k]), C.byref(oc), 1.0)
        banks.append(A.BiquadBank(secs, ch, 2))
        oracles.append(osecs)
        frames.append(f)
    rng = np.random.default_rng(99)
    for tick in range(ticks):
        xs = [(rng.random((f, ch), dtype=np.float32) * 2 - 1) for f in frames]
        bufs = [torch.from_numpy(x.copy()).cuda() for x in xs]
        side = sum(1 for f in frames if f > _serial_max(A))                # (a pre-filter call above the bound: its single call)
        assert A.biquad_batch_device(banks, bufs, frames) == 1 + side     # one class (2 sections) for the rest
        for x, osecs, f in zip(xs, oracles, frames):
            for k in range(ch):
                for s in range(2):
                    OL.ora_biquad_buffer(C.byref(osecs[k * 2 + s]), C.cast(x.ctypes.data + 4 * k, f32p), f, ch)
        torch.cuda.synchronize()
        for j, (b, x) in enumerate(zip(bufs, xs)):
            assert np.array_equal(b.cpu().numpy().view(np.uint32), x.view(np.uint32)), (tick, j)
    hist = lambda q, arr: [arr[(q.index - i) & 3] for i in range(4)]
    for b, osecs in zip(banks, oracles):
        st = b.read()
        for k in range(ch * 2):
            assert hist(st[k], st[k].x) == hist(osecs[k], osecs[k].x) and hist(st[k], st[k].y) == hist(osecs[k], osecs[k].y)
        b.close()


@pytest.mark.parametrize("lanes", [1, 3, 8, 64])
def test_forced_lane_counts_equal_twins(lanes):
    """lanes of different banks, section orders and frame counts in one serial wave; banks cut across workgroups (3), empty lanes
    padding the last workgroup, the 64-lane LDS layout"""
    _batch_equals_twins(A, torch.float32, _specs(A), _with_lanes(A, lanes), ticks=3, single_ticks=())


def test_large_class_under_the_lane_rule_equals_twins():
    """one class of more than 8,192 lanes: the rule packs 32 lanes to a workgroup"""
    kinds, frames, chans = ["pre", "post", "hand"], [441, 960, 1, 64, 300, 0], [2, 2, 3]
    specs, total, i = [], 0, 0
    while total <= 8300:
        specs.append(dict(ch=chans[i % 3], S=2, kind=kinds[i % 3], frames=[frames[(i + t) % 6] for t in range(2)]))
        total += chans[i % 3] if specs[-1]["frames"][0] > 0 else 0
        i += 1
    assert A.lib().arthip_biquad_batch_lanes(total) == 32
    _batch_equals_twins(A, torch.float32, specs, ticks=2, single_ticks=())


def test_side_calls_count_one_launch_each(monkeypatch):
    """a sharded bank, a bank on another stream and a call above the bound that its single call makes time-parallel are made on the
    side: the return value counts one launch per present class plus one per side call, and every result equals its twin's"""
    over = max(_serial_max(A) + 1, 800)         # (and at least twice the pre-filter's chunk: the single call is time-parallel)
    monkeypatch.setenv("ARTAMD_SHARDS", "4")
    specs = [dict(ch=2, S=2, kind="pre"), dict(ch=8, S=2, kind="pre"), dict(ch=2, S=2, kind="post"), dict(ch=2, S=2, kind="pre"),
             dict(ch=6, S=1, kind="hand"), dict(ch=2, S=3, kind="hp")]
    pairs = [_pair(A, s, multi=(i == 1)) for i, s in enumerate(specs)]
    banks, twins = [p[0] for p in pairs], [p[1] for p in pairs]
    assert banks[1].shards() == 4
    side = torch.cuda.Stream()                  # (non-blocking: ordered after the current stream by hand below)
    banks[2].set_stream(side.cuda_stream)
    frames = [441, 441, 441, over, 441, 441]
    for tick in range(2):
        xs = _inputs(frames, [s["ch"] for s in specs], tick, torch.float32)
        bufs = [x.clone() for x in xs]
        side.wait_stream(torch.cuda.current_stream())      # the side bank's input comes first
        assert A.biquad_batch_device(banks, bufs, frames) == 3 + 3
        for t, x, f in zip(twins, xs, frames):
            t.apply_device(x, f)
        torch.cuda.synchronize()
        for i in range(len(specs)):
            assert torch.equal(_bits(bufs[i]), _bits(xs[i])), (tick, specs[i])
            assert _state(banks[i]) == _state(twins[i]), (tick, specs[i])
    for b in banks + twins:
        b.close()


def test_edges_empty_duplicate_and_null():
    L = A.lib()
    assert L.biquadBankApplyBatchInterleavedDevice(None, 0, None, None) == 0
    specs = [dict(ch=2, S=2, kind="post"), dict(ch=6, S=1, kind="hand")]
    banks = [_pair(A, s)[0] for s in specs]
    frames = [441, 300]
    xs = _inputs(frames, [s["ch"] for s in specs], 0, torch.float32)
    bufs = [x.clone() for x in xs]
    assert A.biquad_batch_device(banks, bufs, [0, 0]) == 0
    assert A.biquad_batch_device(banks, bufs, [-5, 0]) == 0
    before, states = L.artamdErrorCount(), [_state(b) for b in banks]
    with pytest.raises(RuntimeError):
        A.biquad_batch_device([banks[0], banks[1], banks[0]], bufs + bufs[:1], frames + frames[:1])
    n = 2
    rc = L.biquadBankApplyBatchInterleavedDevice((C.c_void_p * n)(banks[0].p, None), n,
                                                 (C.c_void_p * n)(*[b.data_ptr() for b in bufs]), (C.c_int * n)(*frames))
    assert rc == -1
    torch.cuda.synchronize()
    assert L.artamdErrorCount() == before               # refused calls are not launch failures
    for b, x in zip(bufs, xs):
        assert torch.equal(_bits(b), _bits(x))
    assert [_state(b) for b in banks] == states
    for b in banks:
        b.close()


def test_wide_build_mixed_batch_equals_twins():
    W = A.binding(64)
    _batch_equals_twins(W, torch.float64, _specs(W), ticks=4, single_ticks=(2,))
    _batch_equals_twins(W, torch.float64, _specs(W), _with_lanes(W, 64), ticks=2, single_ticks=())


def test_biquad_batch_bench_beats_the_loop():
    n, frames, ticks = 1024, 441, 15
    secs = _sections(A, 2, 2, "post")
    loop = [A.BiquadBank(secs, 2, 2) for _ in range(n)]
    batch = [A.BiquadBank(secs, 2, 2) for _ in range(n)]
    x = torch.rand(n, frames * 2, device="cuda") * 2 - 1
    xs = [x[i] for i in range(n)]

    def tick_loop():
        for i, b in enumerate(loop):
            b.apply_device(xs[i], frames)

    def tick_batch():
        A.biquad_batch_device(batch, xs, [frames] * n)

    def median(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(ticks):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return statistics.median(t)

    t_loop, t_batch = median(tick_loop), median(tick_batch)
    print(f"biquad tick, 1,024 stereo x 441 frames, 2 sections: loop {t_loop * 1e3:.3f} ms, batch {t_batch * 1e3:.3f} ms, "
          f"{t_loop / t_batch:.1f}x")
    assert t_batch * 10 <= t_loop, (t_loop, t_batch)
    for b in loop + batch:
        b.close()
