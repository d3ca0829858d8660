"""GPU: resampleProcessAndFlushClipsPlanarDevice — a pool of used contexts takes a list of clips from a fresh start: one zeroing launch
puts every gathered context's history back, no memset per context.  Counts and samples are bit for bit those of fresh contexts on
each clip alone (tests/test_gpu_clip_resampler.py's alone()); with fromStart 0 the call is the batch entry."""
import numpy as np
import pytest
import torch

import audio_resampler_amd as A
from test_gpu_clip_resampler import alone

pytestmark = pytest.mark.gpu
BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
FLAGS = BH | IN | LP
SRC, DST, T = 44100.0, 16000.0, 380                # 570 frames of history (a filter length and a half)
RATIO = DST / SRC
LONG = 3000
BIG = 263200                                       # x 2 channels x 380 taps = 2e8: the single planar call stages it for the matrix cores


def _dtype(M):
    return torch.float64 if getattr(M, "width", 32) == 64 else torch.float32


def _cap(frames):
    return int(frames * DST / SRC) + T + 64


def _alone(M, x, frames, flags):
    """alone() of tests/test_gpu_clip_resampler.py in either build: the clip on a context of its own, the process call and the flush"""
    if M is A:
        return alone(x, frames, flags)
    ch = x.shape[0]
    r = M.Resampler(ch, T, T, 0.0, flags, (SRC, DST, 0))
    cap = _cap(frames)
    y = torch.zeros(ch, cap, device="cuda", dtype=x.dtype)
    xc = x.contiguous()
    u, g = r.process_planar_device(xc if frames else None, max(frames, 1), frames, y, cap, cap, 0.0)
    assert u == frames
    _, more = r.process_planar_device(None, 0, -1, y[:, g:], cap, cap - g, 0.0)
    r.synchronize()
    out = y[:, :g + more].cpu().numpy()
    r.close()
    return out


def _noise(M, seed, ch, frames):
    x = (0.25 * np.random.default_rng(seed).standard_normal((ch, frames))).astype(np.float32)
    return torch.from_numpy(x).to(_dtype(M)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


class Clips:
    """one call's buffers: planar items are rows of a wider tensor (pitch: its row length), interleaved items frames x channels"""
    def __init__(self, M, pool, xs, lengths, planar):
        self.pool, self.lengths, self.planar = pool, lengths, planar
        self.keep, self.ins, self.ipitch, self.outs, self.opitch, self.caps, self.ys = [], [], [], [], [], [], []
        for r, x, n, pl in zip(pool, xs, lengths, planar):
            ch, cap = r.channels, _cap(n)
            if pl:
                y = torch.zeros(ch, cap + 3, device="cuda", dtype=x.dtype)
                self.ins.append(x.data_ptr()); self.ipitch.append(x.stride(0) if ch > 1 else 0)
                self.outs.append(y.data_ptr()); self.opitch.append(y.stride(0) if ch > 1 else 0)
            else:
                xi = x[:, :max(n, 1)].t().contiguous()
                y = torch.zeros(cap, ch, device="cuda", dtype=x.dtype)
                self.keep.append(xi)
                self.ins.append(xi.data_ptr()); self.ipitch.append(0)
                self.outs.append(y.data_ptr()); self.opitch.append(0)
            self.caps.append(cap); self.ys.append(y)

    def args(self):
        return (self.pool, self.ins, self.ipitch, self.lengths, self.outs, self.opitch, self.caps, [RATIO] * len(self.pool))

    def made(self, i, g):
        """item i's first g output frames as [C, g]"""
        y = self.ys[i]
        return (y[:, :g] if self.planar[i] else y[:g].t()).cpu().numpy()

    def rest_is_zero(self, i, g):
        y = self.ys[i]
        return bool((y[:, g:] == 0).all()) if self.planar[i] else bool((y[g:] == 0).all())


def _use(r, x, frames, calls=1, flush=False):
    """dirties a context: `calls` appending process calls of a long clip (and a flush behind the last one)"""
    ch = r.channels
    cap = _cap(frames)
    y = torch.zeros(ch, cap, device="cuda", dtype=x.dtype)
    for k in range(calls):
        fn = r.process_and_flush_planar_device if flush and k == calls - 1 else r.process_planar_device
        u, g = fn(x, x.stride(0) if ch > 1 else 0, frames, y, y.stride(0) if ch > 1 else 0, cap, RATIO)
        assert u == frames and g > 0
    r.synchronize()


def _check_fresh(M, clips, got, xs, flags, what):
    torch.cuda.synchronize()
    for i, n in enumerate(clips.lengths):
        want = _alone(M, xs[i][:, :n], n, flags[i])
        u, g = got[i]
        assert u == n and g == want.shape[1], (what, i, got[i], want.shape)
        assert np.array_equal(_bits(clips.made(i, g)), _bits(want)), (what, i)
        assert clips.rest_is_zero(i, g), (what, i)


def _scenario(M, with_big):
    """round 1 leaves every context used in its own way; round 2 takes clips shorter than, as long as and longer than the 570-frame
    history from the start"""
    chans = [2, 2, 1, 3, 2, 2] + ([2] if with_big else [])
    flags = [FLAGS, FLAGS, FLAGS | A.EXTRAPOLATE_ENDPOINTS, FLAGS, FLAGS, FLAGS] + ([FLAGS] if with_big else [])
    lengths = [1, 0, 100, 569, 571, 3000] + ([BIG] if with_big else [])
    planar = [True, True, True, True, True, False] + ([True] if with_big else [])
    pool = [M.Resampler(ch, T, T, 0.0, f, (SRC, DST, 0)) for ch, f in zip(chans, flags)]
    loud = [_noise(M, 20 + i, ch, LONG) * 3.0 for i, ch in enumerate(chans)]
    _use(pool[0], loud[0], LONG, calls=1)          # an odd ...
    _use(pool[1], loud[1], LONG, calls=2)          # ... and an even number of appending calls: both current-buffer indices
    _use(pool[2], loud[2], LONG, calls=1)          # (extrapolating: its prefill is due again after the reset)
    _use(pool[3], loud[3], LONG, calls=1, flush=True)
    assert pool[3].c.flags & A.RESAMPLER_FLUSHED   # re-armed by the call
    _use(pool[4], loud[4], LONG, calls=1)
    pool[4].advance(2.25)
    _use(pool[5], loud[5], LONG, calls=3)
    if with_big:
        _use(pool[6], loud[6], LONG, calls=1)
    xs = [_noise(M, 40 + i, ch, max(n, 1) + 7) for i, (ch, n) in enumerate(zip(chans, lengths))]
    clips = Clips(M, pool, xs, lengths, planar)
    got = M.process_and_flush_clips_planar_device(*clips.args(), from_start=True)
    _check_fresh(M, clips, got, xs, flags, "round 2")
    for r in pool:
        assert r.c.flags & A.RESAMPLER_FLUSHED
    # once more, the pool now flushed throughout, with other lengths
    lengths2 = lengths[1:] + lengths[:1] if not with_big else lengths[1:6] + lengths[:1] + [600]
    xs2 = [_noise(M, 60 + i, ch, max(n, 1) + 7) for i, (ch, n) in enumerate(zip(chans, lengths2))]
    clips = Clips(M, pool, xs2, lengths2, planar)
    got = M.process_and_flush_clips_planar_device(*clips.args(), from_start=True)
    _check_fresh(M, clips, got, xs2, flags, "round 3")
    for r in pool:
        r.close()


def test_used_pool_from_the_start_equals_fresh_contexts():
    _scenario(A, with_big=True)


def test_used_pool_from_the_start_equals_fresh_contexts_wide_build():
    _scenario(A.wide(), with_big=False)


def test_side_contexts_get_their_own_reset(monkeypatch):
    """another stream, strict order (made one by one on the lead's stream), two shards: between gathered contexts"""
    flags = [FLAGS, FLAGS, FLAGS | A.RESAMPLE_STRICT_ORDER, FLAGS | A.RESAMPLE_MULTITHREADED, FLAGS]
    chans = [2, 2, 2, 4, 1]
    lengths = [571, 100, 569, 3000, 1]
    pool = [A.Resampler(ch, T, T, 0.0, f, (SRC, DST, 0)) for ch, f in zip(chans[:3], flags[:3])]
    monkeypatch.setenv("ARTAMD_SHARDS", "2")
    pool.append(A.Resampler(4, T, T, 0.0, flags[3], (SRC, DST, 0)))
    monkeypatch.delenv("ARTAMD_SHARDS")
    assert len(pool[3].shards()) == 2
    pool.append(A.Resampler(1, T, T, 0.0, flags[4], (SRC, DST, 0)))
    for i, r in enumerate(pool):
        _use(r, _noise(A, 80 + i, chans[i], LONG) * 3.0, LONG, calls=1 + i % 2)
    side = torch.cuda.Stream()
    pool[1].set_stream(side.cuda_stream)
    xs = [_noise(A, 90 + i, ch, n + 7) for i, (ch, n) in enumerate(zip(chans, lengths))]
    clips = Clips(A, pool, xs, lengths, [True] * 5)
    torch.cuda.synchronize()                       # (the buffers are made on the default stream)
    got = A.process_and_flush_clips_planar_device(*clips.args(), from_start=True)
    side.synchronize()
    _check_fresh(A, clips, got, xs, flags, "side")
    for r in pool:
        r.close()


def test_not_from_the_start_is_the_batch_entry():
    chans, lengths = [2, 1, 3], [700, 100, 1500]
    pools = [[A.Resampler(ch, T, T, 0.0, FLAGS, (SRC, DST, 0)) for ch in chans] for _ in range(2)]
    for pool in pools:
        for i, r in enumerate(pool):
            _use(r, _noise(A, 100 + i, chans[i], LONG), LONG, calls=1 + i % 2)
    xs = [_noise(A, 110 + i, ch, n) for i, (ch, n) in enumerate(zip(chans, lengths))]
    a, b = Clips(A, pools[0], xs, lengths, [True, True, False]), Clips(A, pools[1], xs, lengths, [True, True, False])
    got = A.process_and_flush_clips_planar_device(*a.args(), from_start=False)
    want = A.process_and_flush_batch_planar_device(*b.args())
    torch.cuda.synchronize()
    assert got == want
    for i in range(3):
        assert torch.equal(a.ys[i], b.ys[i]), i
        assert pools[0][i].state() == pools[1][i].state(), i
    fresh = alone(xs[0], lengths[0], FLAGS)        # (and the history was NOT cleared: a used context's clip is no fresh one's)
    g = got[0][1]
    assert g != fresh.shape[1] or not np.array_equal(_bits(a.made(0, g)), _bits(fresh))
    for r in pools[0] + pools[1]:
        r.close()


def test_duplicate_context_is_refused_before_any_reset():
    pool = [A.Resampler(2, T, T, 0.0, FLAGS, (SRC, DST, 0)) for _ in range(2)]
    for i, r in enumerate(pool):
        _use(r, _noise(A, 120 + i, 2, LONG), LONG)
    before = [(r.state(), r.position()) for r in pool]
    xs = [_noise(A, 130 + i, 2, 500) for i in range(3)]
    clips = Clips(A, pool + pool[:1], xs, [500, 500, 500], [True] * 3)
    errors = A.lib().artamdErrorCount()
    with pytest.raises(RuntimeError):
        A.process_and_flush_clips_planar_device(*clips.args(), from_start=True)
    torch.cuda.synchronize()
    assert [(r.state(), r.position()) for r in pool] == before
    assert all(bool((y == 0).all()) for y in clips.ys)
    assert A.lib().artamdErrorCount() == errors
    for r in pool:
        r.close()
