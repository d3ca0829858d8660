"""Whole clips through the stretcher in one launch (stretchProcessAndFlushBatchPlanarDevice, ClipStretcher): every output bit, every
frame count and the context state against the oracle and against the equivalent single calls, in both layouts on both sides, at the
edge lengths, on reused contexts and on streams that earlier calls began; nothing outside the produced frames is written; the
refusals; a flushed context returns."""
import ctypes as C

import numpy as np
import pytest

import _stretch as S

pytestmark = pytest.mark.gpu

RATE = 44100
CTOR = (RATE // 350, RATE // 50)                     # ART's periods: 126 and 882 frames
SENTINEL = -777.25
WIDTHS = [(32, np.float32), (64, np.float64)]
_sig, _ora = {}, {}


class Stretch(C.Structure):                          # include/stretch.h
    pass


Stretch._fields_ = [("num_chans", C.c_int), ("inbuff_samples", C.c_int), ("shortest", C.c_int), ("longest", C.c_int),
                    ("tail", C.c_int), ("head", C.c_int), ("fast_mode", C.c_int), ("inbuff", C.c_void_p), ("calcbuff", C.c_void_p),
                    ("results", C.c_void_p), ("outsamples_error", C.c_double), ("next", C.POINTER(Stretch)),
                    ("intermediate", C.c_void_p), ("hip", C.c_void_p)]


def mirrors(p):
    """the host mirrors of a context and of its second stage"""
    out, s = [], C.cast(p, C.POINTER(Stretch))
    while s:
        out.append((s.contents.tail, s.contents.head, np.float64(s.contents.outsamples_error).view(np.uint64).item()))
        s = s.contents.next
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def clip(frames, ch, dt, start=0):
    """`frames` frames of the pitched test signal, from frame `start` on (one signal per channel count and type, made once)"""
    if (ch, dt) not in _sig:
        _sig[ch, dt] = S.signal(int(RATE * 0.8), ch, RATE, seed=40 + ch, dtype=dt)
    return np.ascontiguousarray(_sig[ch, dt][start:start + frames])


def oracle(width, dt, ch, flags, ratio, frames, start=0):
    """(samples [frames, ch], total frames) a fresh oracle makes of the clip: process call, then the drains.  Made once, shared."""
    key = (width, ch, flags, ratio, frames, start)
    if key not in _ora:
        y, counts = S.OracleStretch(*CTOR, ch, flags, width=width).run(clip(frames, ch, dt, start), [max(frames, 1)], [ratio])
        _ora[key] = (y, sum(counts))
    return _ora[key]


class Batch:
    """device buffers of a batch in chosen layouts: "ii" interleaved on both sides, "pp" tight planes, "pad" planes with an odd padded
    pitch (T + 3 in, cap + 3 out), "pi" planes in and interleaved out, "ip" the reverse; everything outside the input samples holds SENTINEL"""

    def __init__(self, torch, A, width, dt, ctxs, xs, layouts, ratios, caps=None):
        self.torch, self.B, self.ctxs, self.xs, self.layouts, self.ratios = torch, A.binding(width), ctxs, xs, layouts, ratios
        tdt = torch.float32 if width == 32 else torch.float64
        L = self.B.lib()
        self.caps = caps or [L.artamdStretchClipCapacity(CTOR[1], c.flags, len(x), r) for c, x, r in zip(ctxs, xs, ratios)]
        self.ins, self.outs, self.in_pitch, self.out_pitch = [], [], [], []
        for x, lay, cap in zip(xs, layouts, self.caps):
            T, ch = x.shape
            if lay in ("ii", "ip"):
                self.ins.append(torch.from_numpy(x).to("cuda").reshape(-1) if T else torch.full((4,), SENTINEL, dtype=tdt, device="cuda"))
                self.in_pitch.append(0)
            else:
                P = T + 3 if lay == "pad" else T
                buf = torch.full((max(ch * P, 4),), SENTINEL, dtype=tdt, device="cuda")
                for c in range(ch):
                    buf[c * P: c * P + T] = torch.from_numpy(np.ascontiguousarray(x[:, c])).to("cuda")
                self.ins.append(buf); self.in_pitch.append(P)
            Q = 0 if lay in ("ii", "pi") else (cap + 3 if lay == "pad" else cap)      # ("ip": interleaved in, tight planes out)
            self.outs.append(torch.full(((Q or cap) * ch,), SENTINEL, dtype=tdt, device="cuda"))
            self.out_pitch.append(Q)

    def call(self, from_start, lengths=None):
        lengths = [len(x) for x in self.xs] if lengths is None else lengths
        return self.B.stretch_clips_batch_planar_device(self.ctxs, self.ins, self.in_pitch, lengths, self.outs, self.out_pitch,
                                                        self.caps, self.ratios, from_start=from_start)

    def result(self, i, g):
        """(the first g frames of clip i as [g, ch], everything else of its output buffer)"""
        ch, Q, cap = self.xs[i].shape[1], self.out_pitch[i], self.caps[i]
        o = self.outs[i].cpu().numpy()
        if not Q:
            return o[:g * ch].reshape(g, ch), o[g * ch:]
        return np.stack([o[c * Q: c * Q + g] for c in range(ch)], axis=1), np.concatenate([o[c * Q + g: (c + 1) * Q] for c in range(ch)])

    def check(self, i, made, want, count):
        got, rest = self.result(i, made)
        assert made == count, (i, made, count)
        assert np.array_equal(bits(got), bits(want)), i
        assert (rest == SENTINEL).all(), i                # padding between the planes and everything past the produced frames


def contexts(A, width, kinds):
    return [A.binding(width).Stretcher(*CTOR, ch, flags) for ch, flags in kinds]


def single_calls(torch, L, p, x, ratio, cap, tdt):
    """stretchProcessDevice (skipped for an empty clip), then stretchFlushDevice until it returns 0, on an interleaved copy"""
    d_out = torch.zeros(cap * x.shape[1], dtype=tdt, device="cuda")
    ys = []
    if len(x):
        d_in = torch.from_numpy(x).to("cuda")
        g = L.stretchProcessDevice(p, d_in.data_ptr(), len(x), d_out.data_ptr(), ratio)
        ys.append(d_out[:g * x.shape[1]].cpu().numpy())
    for _ in range(4):
        g = L.stretchFlushDevice(p, d_out.data_ptr())
        ys.append(d_out[:g * x.shape[1]].cpu().numpy())
        if not g:
            break
    return np.concatenate(ys).reshape(-1, x.shape[1])


# (channels, flags, ratio, layout): mono and stereo; normal, fast, dual, fast + dual; the layouts mixed in the one call
EIGHT = [(1, 0, 0.5, "ii"), (2, 0, 0.8, "pp"), (2, 0, 1.0, "pad"), (1, S.FAST, 1.25, "pad"), (2, S.FAST, 2.0, "pi"),
         (2, S.DUAL, 0.3, "pp"), (1, S.DUAL, 3.1, "ii"), (2, S.FAST | S.DUAL, 3.1, "pad")]


@pytest.mark.parametrize("width,dt", WIDTHS)
def test_one_launch_of_eight_clips_equals_the_oracle_bit_for_bit(width, dt):
    torch = pytest.importorskip("torch")
    import audio_resampler_amd as A
    T = int(RATE * 0.3)
    tdt = torch.float32 if width == 32 else torch.float64
    ctxs = contexts(A, width, [(ch, fl) for ch, fl, _, _ in EIGHT])
    twins = contexts(A, width, [(ch, fl) for ch, fl, _, _ in EIGHT])
    xs = [clip(T, ch, dt) for ch, _, _, _ in EIGHT]
    b = Batch(torch, A, width, dt, ctxs, xs, [lay for *_, lay in EIGHT], [r for _, _, r, _ in EIGHT])
    made = b.call(from_start=True)
    L = A.binding(width).lib()
    for i, (ch, fl, r, lay) in enumerate(EIGHT):
        want, count = oracle(width, dt, ch, fl, r, T)
        print(f"clip {i}: {ch} ch flags {fl} ratio {r} {lay}: made {made[i]}, oracle {count}, capacity {b.caps[i]}")
        b.check(i, made[i], want, count)
        # the same clip by single calls on a twin context: the same samples, the same state afterwards
        y = single_calls(torch, L, twins[i].p, xs[i], r, b.caps[i], tdt)
        assert np.array_equal(bits(y), bits(want))
        assert mirrors(ctxs[i].p) == mirrors(twins[i].p), i


def test_a_one_second_stereo_clip_in_every_layout_pair():
    """a clip long enough to hold the test signal's noise burst and the way out of its silent gap, the same clip in the four
    combinations of layouts in one call"""
    torch = pytest.importorskip("torch")
    import audio_resampler_amd as A
    x = np.ascontiguousarray(S.signal(RATE + 1024, 2, RATE, seed=3)[:RATE])
    want, counts = S.OracleStretch(*CTOR, 2, 0).run(x, [RATE], [0.8])
    layouts = ["ii", "pp", "pi", "ip"]
    b = Batch(torch, A, 32, np.float32, contexts(A, 32, [(2, 0)] * 4), [x] * 4, layouts, [0.8] * 4)
    made = b.call(from_start=True)
    for i in range(4):
        b.check(i, made[i], want, sum(counts))


@pytest.mark.parametrize("flags", [0, S.FAST | S.DUAL])
def test_edge_lengths_in_one_batch(flags):
    torch = pytest.importorskip("torch")
    import audio_resampler_amd as A
    ring = CTOR[1] * (4 if flags & S.FAST else 3)
    # nothing at all; shorter than one longest period (everything comes from the drains); exactly the ring; the ring and one frame
    lengths, ratios = [0, 500, ring, ring + 1], [1.3, 0.7, 1.3, 2.0]
    ctxs = contexts(A, 32, [(2, flags)] * 4)
    b = Batch(torch, A, 32, np.float32, ctxs, [clip(n, 2, np.float32, 900) for n in lengths], ["pp", "pad", "pp", "pad"], ratios)
    made = b.call(from_start=True)
    for i, (n, r) in enumerate(zip(lengths, ratios)):
        want, count = oracle(32, np.float32, 2, flags, r, n, 900)
        print(f"{n} frames at {r}: made {made[i]}, oracle {count}")
        b.check(i, made[i], want, count)
    assert made[0] == 0 and made[1] == 500


def test_pool_reuse_from_the_start_and_finishing_a_stream_that_single_calls_began():
    torch = pytest.importorskip("torch")
    import audio_resampler_amd as A
    kinds = [(1, 0), (2, S.FAST), (2, S.DUAL)]
    ctxs = contexts(A, 32, kinds)
    T = int(RATE * 0.25)
    # the same contexts twice, on different clips at different ratios: the first call leaves a length error behind, which
    # stretchReset would keep; fromStart does not
    for start, ratios in ((0, [1.25, 0.8, 3.1]), (3000, [0.7, 1.6, 0.3])):
        b = Batch(torch, A, 32, np.float32, ctxs, [clip(T, ch, np.float32, start) for ch, _ in kinds], ["ii", "pad", "pp"], ratios)
        made = b.call(from_start=True)
        for i, (ch, fl) in enumerate(kinds):
            want, count = oracle(32, np.float32, ch, fl, ratios[i], T, start)
            b.check(i, made[i], want, count)
    # fromStart = 0: three blocks by stretchProcessDevice, then the entry finishes the stream: with a last block, and with none
    L = A.lib()
    blocks, block_ratios = [5000, 37, 4000], [1.3, 0.9, 1.7]
    for last in (3000, 0):
        fresh = contexts(A, 32, kinds)
        oras = [S.OracleStretch(*CTOR, ch, fl) for ch, fl in kinds]
        for i, (ch, fl) in enumerate(kinds):
            pos = 0
            for n, r in zip(blocks, block_ratios):
                x = clip(n, ch, np.float32, pos)
                out = np.zeros((oras[i].capacity(n, 2.0), ch), np.float32)
                d_in, d_out = torch.from_numpy(x).to("cuda"), torch.zeros(out.size, device="cuda")
                g = oras[i].feed(x, out, r)
                assert L.stretchProcessDevice(fresh[i].p, d_in.data_ptr(), n, d_out.data_ptr(), r) == g
                assert np.array_equal(bits(d_out[:g * ch].cpu().numpy()), bits(out[:g].reshape(-1)))
                pos += n
        pos, ratios = sum(blocks), [1.1, 0.6, 2.7]
        xs = [clip(last, ch, np.float32, pos) for ch, _ in kinds]
        b = Batch(torch, A, 32, np.float32, fresh, xs, ["pp", "pi", "pad"], ratios)
        made = b.call(from_start=False)
        for i, (ch, fl) in enumerate(kinds):
            out = np.zeros((b.caps[i], ch), np.float32)
            ys = []
            if last:
                g = oras[i].feed(xs[i], out, ratios[i]); ys.append(out[:g].copy())
            for _ in range(4):
                g = oras[i].drain(out); ys.append(out[:g].copy())
                if not g:
                    break
            want = np.concatenate(ys)
            b.check(i, made[i], want, len(want))


def test_a_cap_one_frame_short_and_a_context_listed_twice_are_refused_with_nothing_done():
    torch = pytest.importorskip("torch")
    import audio_resampler_amd as A
    T, kinds, ratios = int(RATE * 0.25), [(2, 0), (1, S.DUAL)], [1.25, 3.1]
    ctxs = contexts(A, 32, kinds)
    xs = [clip(T, ch, np.float32) for ch, _ in kinds]
    b = Batch(torch, A, 32, np.float32, ctxs, xs, ["pad", "ii"], ratios)
    before = [mirrors(c.p) for c in ctxs]
    errors = A.lib().artamdErrorCount()
    good = list(b.caps)
    b.caps = [good[0], good[1] - 1]
    with pytest.raises(RuntimeError):
        b.call(from_start=True)
    b.caps = good
    b.ctxs = [ctxs[0], ctxs[0]]
    with pytest.raises(RuntimeError):
        b.call(from_start=True)
    b.ctxs = ctxs
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == SENTINEL).all() for o in b.outs)          # nothing enqueued
    assert [mirrors(c.p) for c in ctxs] == before and A.lib().artamdErrorCount() == errors
    made = b.call(from_start=True)
    for i, (ch, fl) in enumerate(kinds):
        want, count = oracle(32, np.float32, ch, fl, ratios[i], T)
        b.check(i, made[i], want, count)


def test_a_flushed_context_arriving_without_from_start_returns():
    """A flushed context is terminal until a reset; fed again its ring can be full with nothing processable, where the reference's
    loop never ends.  The whole-clip kernel keeps feed's full-ring break and makes at most four drain rounds, so it returns, and what
    it wrote stays inside the capacity."""
    torch = pytest.importorskip("torch")
    import audio_resampler_amd as A
    kinds, ratios = [(1, 0), (2, S.FAST | S.DUAL)], [1.3, 3.1]
    ctxs = contexts(A, 32, kinds)
    b = Batch(torch, A, 32, np.float32, ctxs, [clip(20000, ch, np.float32) for ch, _ in kinds], ["ii", "pp"], ratios)
    b.call(from_start=True)                          # leaves both contexts flushed
    for _ in range(2):
        b = Batch(torch, A, 32, np.float32, ctxs, [clip(int(RATE * 0.6), ch, np.float32) for ch, _ in kinds], ["ii", "pad"], ratios)
        made = b.call(from_start=False)
        for i in range(len(kinds)):
            assert 0 <= made[i] <= b.caps[i]
            assert (b.result(i, made[i])[1] == SENTINEL).all()
    # ... and from the start the same contexts work again
    T = int(RATE * 0.25)
    b = Batch(torch, A, 32, np.float32, ctxs, [clip(T, ch, np.float32) for ch, _ in kinds], ["pp", "pi"], ratios)
    made = b.call(from_start=True)
    for i, (ch, fl) in enumerate(kinds):
        want, count = oracle(32, np.float32, ch, fl, ratios[i], T)
        b.check(i, made[i], want, count)


def test_clip_stretcher_ragged_batch_with_both_pools_and_a_mono_clip():
    torch = pytest.importorskip("torch")
    import audio_resampler_amd as A
    T = int(RATE * 0.3)
    lengths, ratios = [T, 9000, 0, 12345, 700], [1.25, 2.6, 0.8, 0.4, 2.0]          # straddling 2.0 and 0.5: both pools
    x = torch.from_numpy(np.ascontiguousarray(np.stack([clip(T, 2, np.float32, 200 * i).T for i in range(5)]))).to("cuda")
    cs = A.ClipStretcher(2, RATE, max_batch=2)       # (three single-stage clips through a pool of two: chunked)
    y, out_lengths = cs(x, ratios, lengths=lengths)
    assert sorted(cs.pools) == [0, S.DUAL] and y.shape[:2] == (5, 2) and y.shape[2] == int(out_lengths.max())
    yh = y.cpu().numpy()
    for i, (n, r) in enumerate(zip(lengths, ratios)):
        want, count = oracle(32, np.float32, 2, 0 if 0.5 <= r <= 2.0 else S.DUAL, r, n, 200 * i)
        assert int(out_lengths[i]) == count, i
        assert np.array_equal(bits(yh[i, :, :count].T), bits(want)), i
        assert not yh[i, :, count:].any(), i
    # a second call reuses the pools and gives the same again
    y2, l2 = cs(x, ratios, lengths=lengths)
    assert torch.equal(y, y2) and torch.equal(out_lengths, l2)
    with pytest.raises(ValueError):
        cs(x, 5.0)
    cs.close()
    mono = A.ClipStretcher(1, RATE)
    xm = torch.from_numpy(clip(T, 1, np.float32).T.copy()).to("cuda")              # [1, T]
    ym, lm = mono(xm, 1.25)
    want, count = oracle(32, np.float32, 1, 0, 1.25, T)
    assert ym.shape == (1, 1, count) and int(lm[0]) == count and np.array_equal(bits(ym[0, 0].cpu().numpy()), bits(want[:, 0]))
    with pytest.raises(ValueError):
        A.ClipStretcher(3, RATE)
    mono.close()
