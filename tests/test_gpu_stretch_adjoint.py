"""The splice log of whole stretched clips, its adjoint and ClipStretcher's autograd (stretchProcessAndFlushLoggedBatchPlanarDevice,
stretchAdjointClipsPlanarDevice): the logged forward is the plain one bit for bit; the log is well formed, and replayed in float64 it
is the output the oracle already pins; the adjoint is the log's transpose, value by value, within the rounding its contract allows;
it does not depend on the batch, the layout or a truncated gradient; the refusals; autograd through ClipStretcher and on into
ClipResampler.  No finite differences: a step across a boundary of the period search is not a derivative.

Small periods (24 and 168 frames: MIN_PERIOD and seven times it, the ratio of ART's bounds) keep a clip of 3,000 .. 5,000 frames at
twenty to a hundred steps, one workgroup, well under a second.  One batch per sample width and channel count is run once and shared."""
import ctypes as C

import numpy as np
import pytest

import _stretch as S
import _stretch_log as SL

pytestmark = pytest.mark.gpu

RATE = 8400
CTOR = (RATE // 350, RATE // 50)                     # 24 and 168 frames
SENTINEL = -777.25
WIDTHS = [(32, np.float32), (64, np.float64)]
U = {32: 2.0 ** -24, 64: 2.0 ** -53}
# (flags, ratio, frames): every step kind; fast mode (two fades per 2:1 step); cascaded pairs; then the smallest clips
CASES = [(0, 0.5, 4000), (0, 0.8, 5000), (0, 1.0, 3000), (0, 1.25, 4500), (0, 1.7, 3700), (0, 2.0, 3100),
         (S.FAST, 1.4, 4100), (S.FAST, 2.0, 3300), (S.DUAL, 0.3, 5000), (S.DUAL, 3.1, 3000),
         (0, 1.25, 0), (0, 0.8, 1), (S.DUAL, 3.1, 167), (0, 1.25, 169)]
_sig, _runs = {}, {}


class Stretch(C.Structure):                          # include/stretch.h
    pass


Stretch._fields_ = [("num_chans", C.c_int), ("inbuff_samples", C.c_int), ("shortest", C.c_int), ("longest", C.c_int),
                    ("tail", C.c_int), ("head", C.c_int), ("fast_mode", C.c_int), ("inbuff", C.c_void_p), ("calcbuff", C.c_void_p),
                    ("results", C.c_void_p), ("outsamples_error", C.c_double), ("next", C.POINTER(Stretch)),
                    ("intermediate", C.c_void_p), ("hip", C.c_void_p)]


def mirrors(p):
    out, s = [], C.cast(p, C.POINTER(Stretch))
    while s:
        out.append((s.contents.tail, s.contents.head, np.float64(s.contents.outsamples_error).view(np.uint64).item()))
        s = s.contents.next
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def clip(frames, ch, dt):
    """the first `frames` frames of 5,000 of the pitched test signal: the silent gap is at 1,666 .. 2,086, the noise burst at 2,500"""
    if (ch, dt) not in _sig:
        _sig[ch, dt] = S.signal(5000, ch, RATE, seed=40 + ch, dtype=dt)
    return np.ascontiguousarray(_sig[ch, dt][:frames])


def put(torch, a, planar, room=None):
    """a [T, ch] on the device with SENTINEL around it: interleaved (pitch 0), or planes `room` + 3 samples apart (room: T at least)"""
    T, ch = a.shape
    room = T if room is None else room
    t = torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    if not planar:
        buf = torch.full((max(room * ch, 4),), SENTINEL, dtype=t.dtype, device="cuda")
        buf[:T * ch] = t.reshape(-1)
        return buf, 0
    P = room + 3
    buf = torch.full((ch * P,), SENTINEL, dtype=t.dtype, device="cuda")
    for c in range(ch):
        buf[c * P: c * P + T] = t[:, c]
    return buf, P


def get(buf, pitch, T, ch):
    """(the first T frames as [T, ch], everything else of the buffer)"""
    o = buf.cpu().numpy()
    if not pitch:
        return o[:T * ch].reshape(T, ch).copy(), o[T * ch:]
    return np.stack([o[c * pitch: c * pitch + T] for c in range(ch)], axis=1), np.concatenate([o[c * pitch + T: (c + 1) * pitch] for c in range(ch)])


def log_caps(L, flags, ratio, frames):
    return [L.artamdStretchLogCapacity(*CTOR, flags, frames, ratio, s) for s in (0, 1)]


def run(width, ch):
    """CASES at this width and channel count: the plain entry on one set of contexts, the logged entry on another, in layouts that
    alternate on both sides; everything the tests need, made once.  Logs come back as numpy and stay on the device too."""
    if (width, ch) in _runs:
        return _runs[width, ch]
    import torch
    import audio_resampler_amd as A
    B, dt = A.binding(width), dict(WIDTHS)[width]
    L = B.lib()
    r = type("Run", (), {})()
    r.B, r.L, r.dt, r.ch = B, L, dt, ch
    r.xs = [clip(frames, ch, dt) for _, _, frames in CASES]
    r.ratios = [ratio for _, ratio, _ in CASES]
    r.ctxs = [B.Stretcher(*CTOR, ch, flags) for flags, _, _ in CASES]
    twins = [B.Stretcher(*CTOR, ch, flags) for flags, _, _ in CASES]
    r.caps = [L.artamdStretchClipCapacity(CTOR[1], flags, frames, ratio) for flags, ratio, frames in CASES]
    r.log_caps = [log_caps(L, *case) for case in CASES]
    lengths = [len(x) for x in r.xs]
    sides = [(i % 2 == 1, i % 4 >= 2) for i in range(len(CASES))]                  # (planar in, planar out)
    ins = [put(torch, x, p_in) for x, (p_in, _) in zip(r.xs, sides)]
    made, outs = [], []
    for logged, ctxs in ((False, twins), (True, r.ctxs)):
        bufs = [put(torch, np.zeros((0, ch), dt), p_out, room=cap) for cap, (_, p_out) in zip(r.caps, sides)]
        args = (ctxs, [b for b, _ in ins], [p for _, p in ins], lengths, [b for b, _ in bufs], [p for _, p in bufs], r.caps, r.ratios)
        if logged:
            r.d_logs = [tuple(torch.full((max(cap, 1), 4), -1, dtype=torch.int32, device="cuda") if s == 0 or flags & S.DUAL else None
                              for s, cap in enumerate(caps)) for caps, (flags, _, _) in zip(r.log_caps, CASES)]
            got, r.counts = B.stretch_clips_logged_batch_planar_device(*args, r.d_logs, r.log_caps)
        else:
            got = B.stretch_clips_batch_planar_device(*args, from_start=True)
        made.append(got)
        outs.append([get(b, p, g, ch) for (b, p), g in zip(bufs, got)])
    r.made_plain, r.made = made
    r.out_plain, r.out = outs
    r.state_plain, r.state = [mirrors(c.p) for c in twins], [mirrors(c.p) for c in r.ctxs]
    r.raw_logs = [[None if t is None else t.cpu().numpy() for t in pair] for pair in r.d_logs]
    r.logs = [[raw[:n] for raw, n in zip(pair, cnt) if raw is not None] for pair, cnt in zip(r.raw_logs, r.counts)]
    for c in twins:
        c.close()
    _runs[width, ch] = r
    return r


GRID = [(w, ch) for w, _ in WIDTHS for ch in (1, 2)]


# ---- 1. the logged forward is the plain forward ------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,ch", GRID)
def test_logged_entry_gives_the_plain_entry_bit_for_bit(width, ch):
    r = run(width, ch)
    assert r.made == r.made_plain and r.state == r.state_plain
    for i, ((y, rest), (y0, rest0)) in enumerate(zip(r.out, r.out_plain)):
        assert np.array_equal(bits(y), bits(y0)), i
        assert (rest == SENTINEL).all() and (rest0 == SENTINEL).all(), i
    assert r.made[10] == 0 and r.made[11] == 1 and all(m > 0 for m in r.made[:10])     # (an empty clip has nothing to flush)


# ---- 2. the log is well formed ------------------------------------------------------------------------------------------------------
def kinds(log, hi):
    """the step kinds a log shows: which fades, a whole-step copy (two longest periods at a ratio of 1), consecutive 2:1 fades"""
    seen = set()
    fades = [(o, n, f, t) for o, n, f, t in log.tolist() if t != SL.COPY]
    for o, n, f, t in fades:
        seen.add("1:2" if t == f + n else "3:2" if t == f - n else "2:1" if 2 * (f - t) == n else "?")
    for (o, n, f, t), (o2, n2, f2, t2) in zip(log.tolist(), log.tolist()[1:]):
        if t != SL.COPY and t2 != SL.COPY and 2 * (f - t) == n and o2 == o + n and f2 == f + n // 2:
            seen.add("2:1 twice")
    if any(t == SL.COPY and n == 2 * hi for o, n, f, t in log.tolist()):
        seen.add("1:1")
    return seen


@pytest.mark.parametrize("width,ch", GRID)
def test_the_log_is_well_formed_and_shows_every_step_kind(width, ch):
    r = run(width, ch)
    hi = CTOR[1] * ch
    seen = {"plain": set(), "fast": set()}
    for i, ((flags, ratio, frames), logs, cnt, caps, raws) in enumerate(zip(CASES, r.logs, r.counts, r.log_caps, r.raw_logs)):
        assert len(logs) == (2 if flags & S.DUAL else 1) and (flags & S.DUAL or cnt[1] == 0), i
        n_in = frames * ch
        for s, log in enumerate(logs):
            assert 0 <= cnt[s] <= caps[s] and (cnt[s] > 0) == (frames > 0), (i, s, cnt, caps)
            assert (raws[s][cnt[s]:] == -1).all(), (i, s)        # nothing written past the count
            if not cnt[s]:
                continue
            out, count, src, to = (log[:, k].astype(np.int64) for k in range(4))
            assert out[0] == 0 and (count > 0).all() and (out[1:] == (out + count)[:-1]).all(), (i, s)
            assert (np.diff(src) >= 0).all(), (i, s)              # `from` never falls: what the adjoint's bisection stands on
            fade = to != SL.COPY
            assert (src >= -hi).all() and (src + count <= n_in).all(), (i, s)
            assert (to[fade] >= -hi).all() and ((to + count)[fade] <= n_in).all(), (i, s)
            n_in = SL.n_out(log)                                  # the next stage's input stream is this one's output
        assert n_in == r.made[i] * ch, i
        if not flags & S.DUAL and frames > 1000:
            seen["fast" if flags & S.FAST else "plain"] |= kinds(logs[0], hi)
    print(seen)
    assert seen["plain"] - {"2:1 twice"} == {"1:2", "1:1", "3:2", "2:1"}      # (two 2:1 steps in a row may find one period)
    assert {"2:1 twice", "2:1"} <= seen["fast"] and "?" not in seen["fast"]
    # fast mode at 2.0: every step is two 2:1 fades at one period, the second a period further on
    fades = [row for row in r.logs[7][0].tolist() if row[3] != SL.COPY]
    assert len(fades) >= 8 and len(fades) % 2 == 0
    for (o, n, f, t), (o2, n2, f2, t2) in zip(fades[0::2], fades[1::2]):
        assert n2 == n and 2 * (f - t) == n and 2 * (f2 - t2) == n and f2 == f + n // 2 and o2 == o + n


# ---- 3. the log is the kernel's map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,ch", GRID)
def test_the_log_replayed_in_float64_is_the_output(width, ch):
    """a fade is two products, a sum and a quotient: 4 u (|a| (n - i) + |b| i) / n covers their roundings; a copy is exact.  Two stages:
    9 u |A2| |A1| |x|, the first stage's error carried through the second and the second's own."""
    r = run(width, ch)
    u = U[width]
    for i, ((flags, ratio, frames), logs) in enumerate(zip(CASES, r.logs)):
        x = r.xs[i].reshape(-1).astype(np.float64)
        y = r.out[i][0].reshape(-1).astype(np.float64)
        want, scale = x, np.abs(x)
        for log in logs:
            want, scale = SL.replay(log, want), SL.replay(log, scale, absolute=True)
        assert len(want) == len(y), i
        err, bound = np.abs(want - y), (4 if len(logs) == 1 else 9) * u * scale
        print(f"clip {i} flags {flags} ratio {ratio}: worst error / bound {np.max(err / np.maximum(bound, 1e-300), initial=0):.3f}")
        assert (err <= bound).all(), i
        if len(logs) == 1:                                        # copies, to the bit
            for o, n, f, t in logs[0].tolist():
                if t == SL.COPY:
                    src = np.arange(f, f + n)
                    assert np.array_equal(y[o:o + n], np.where(src >= 0, x[np.clip(src, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)), (i, o)


# ---- 4. the adjoint is the transpose -------------------------------------------------------------------------------------------------
def adjoint(r, items, gys, n_outs, n_ins, planar_gy, planar_gx):
    """one stretchAdjointClipsPlanarDevice call: item k is clip items[k] of the run, with gradient gys[k] [frames, ch].  Returns (launches,
    [gx [n_in, ch]], [the rest of each gx buffer])"""
    import torch
    g = [put(torch, gy, planar_gy) for gy in gys]
    x = [put(torch, np.zeros((0, r.ch), r.dt), planar_gx, room=n) for n in n_ins]
    rc = r.B.stretch_adjoint_clips_planar_device(
        [r.ctxs[i] for i in items], [r.d_logs[i] for i in items], [r.counts[i] for i in items],
        [b for b, _ in g], [p for _, p in g], n_outs, [b for b, _ in x], [p for _, p in x], n_ins)
    torch.cuda.synchronize()
    got = [get(b, p, n, r.ch) for (b, p), n in zip(x, n_ins)]
    return rc, [a for a, _ in got], [b for _, b in got]


def grads(r, seed=3):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((m, r.ch)).astype(r.dt) for m in r.made]


def full_adjoint(r):
    """every clip of the run in one call, random gradients: made once per run"""
    if not hasattr(r, "gx"):
        r.gys = grads(r)
        r.launches, r.gx, r.gx_rest = adjoint(r, range(len(CASES)), r.gys, r.made, [len(x) for x in r.xs], False, True)
    return r.gx


@pytest.mark.parametrize("width,ch", GRID)
def test_the_adjoint_is_the_transpose_of_the_log(width, ch):
    """per value: K terms of two roundings each and K - 1 additions: (K + 2) u sum |terms|.  Two stages: the second stage's bound e2 on the
    intermediate gradient goes through |A1|^T, and the first stage's own bound is taken on |g_mid| + e2."""
    r = run(width, ch)
    u = U[width]
    gx = full_adjoint(r)
    assert r.launches == 2                                        # the stage that wrote the output of every clip; the pairs' first stage
    for i, ((flags, ratio, frames), logs) in enumerate(zip(CASES, r.logs)):
        got = gx[i].reshape(-1).astype(np.float64)
        assert (r.gx_rest[i] == SENTINEL).all(), i                # nothing past n_ins, nothing between the planes
        g = r.gys[i].reshape(-1).astype(np.float64)
        n_ins = [frames * ch] + [SL.n_out(log) for log in logs[:-1]]
        want, scale, terms = SL.transpose(logs[-1], n_ins[-1], g)
        bound = (terms + 2) * u * scale
        if len(logs) == 2:
            _, carried, _ = SL.transpose(logs[0], n_ins[0], bound)
            want1, scale1, terms1 = SL.transpose(logs[0], n_ins[0], want)
            _, scale_up, _ = SL.transpose(logs[0], n_ins[0], np.abs(want) + bound)
            want, bound, terms = want1, carried + (terms1 + 2) * u * scale_up, terms1
        err = np.abs(got - want)
        print(f"clip {i} flags {flags} ratio {ratio}: worst error / bound {np.max(err / np.maximum(bound, 1e-300), initial=0):.3f}, "
              f"values no segment reads {int((terms == 0).sum())} of {len(terms)}")
        assert (err <= bound).all(), i
        assert (bits(gx[i].reshape(-1)[terms == 0]) == 0).all(), i           # exactly +0


@pytest.mark.parametrize("width,ch", GRID)
def test_unit_impulses_give_a_row_of_the_map(width, ch):
    """gy = e_o at the first and the last output of one segment of each kind: gx is that row — a copy's 1, a fade's (n - i) / n and i / n,
    each one division away from exact — and zero elsewhere.  One call: the one log listed once per impulse."""
    r = run(width, ch)
    u = U[width]
    for clip_at, want_kind in ((0, "1:2"), (3, "3:2"), (5, "2:1"), (2, "copy")):
        log, frames = r.logs[clip_at][0], CASES[clip_at][2]
        pick = next((o, n, f, t) for o, n, f, t in log.tolist()[3:] if (t == SL.COPY) == (want_kind == "copy") and
                    (want_kind == "copy" or {"1:2": t == f + n, "3:2": t == f - n, "2:1": 2 * (f - t) == n}[want_kind]))
        o, n, f, t = pick
        made = r.made[clip_at]
        spots = [o, o + n - 1]
        gys = []
        for spot in spots:
            gy = np.zeros(made * ch, r.dt); gy[spot] = 1
            gys.append(gy.reshape(made, ch))
        rc, gx, _ = adjoint(r, [clip_at] * 2, gys, [made] * 2, [frames] * 2, True, False)
        assert rc == 1
        for spot, got in zip(spots, gx):
            i = spot - o
            want = np.zeros(frames * ch)
            if t == SL.COPY:
                want[f + i] = 1.0
            else:
                want[f + i] += (n - i) / n
                want[t + i] += i / n
            got = got.reshape(-1).astype(np.float64)
            assert (np.abs(got - want) <= u * np.abs(want)).all(), (want_kind, spot)
            assert np.count_nonzero(got) == np.count_nonzero(want), (want_kind, spot)


# ---- 5. invariance -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,ch", GRID)
def test_the_gradient_does_not_depend_on_batch_layout_or_truncation(width, ch):
    r = run(width, ch)
    gx = full_adjoint(r)
    lengths = [len(x) for x in r.xs]
    # thirty-three items of mixed lengths (the clips, listed again and again: the contexts and the logs are only read), the other layouts
    items = [k % len(CASES) for k in range(33)]
    rc, many, _ = adjoint(r, items, [r.gys[i] for i in items], [r.made[i] for i in items], [lengths[i] for i in items], True, False)
    assert rc == 2
    for k, i in enumerate(items):
        assert np.array_equal(bits(many[k]), bits(gx[i])), (k, i)
    # alone
    for i in (1, 3, 9, 12):
        rc, alone, _ = adjoint(r, [i], [r.gys[i]], [r.made[i]], [lengths[i]], i % 2 == 0, i % 3 == 0)
        assert rc == (2 if CASES[i][0] & S.DUAL else 1), i
        assert np.array_equal(bits(alone[0]), bits(gx[i])), i
    # n_outs cut short: the full run with the tail of gy zeroed
    items = [1, 4, 8, 9]
    cut = [r.made[i] * 2 // 3 for i in items]
    zeroed = []
    for i, c in zip(items, cut):
        gy = r.gys[i].copy(); gy[c:] = 0
        zeroed.append(gy)
    _, short, _ = adjoint(r, items, [r.gys[i] for i in items], cut, [lengths[i] for i in items], True, True)
    _, whole, _ = adjoint(r, items, zeroed, [r.made[i] for i in items], [lengths[i] for i in items], True, True)
    for k, i in enumerate(items):
        assert np.array_equal(bits(short[k]), bits(whole[k])), i
        assert not np.array_equal(bits(short[k]), bits(gx[i])), i


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_refusals_enqueue_nothing(width):
    import torch
    r = run(width, 2)
    errors = r.L.artamdErrorCount()
    i = 3
    frames, made, gy = CASES[i][2], r.made[i], grads(r)[i]
    g, gp = put(torch, gy, True)
    x, xp = put(torch, np.zeros((0, 2), r.dt), True, room=frames)
    before = x.clone()
    call = lambda counts, gp_, n_out, xp_, n_in: r.L.stretchAdjointClipsPlanarDevice(
        (C.c_void_p * 1)(r.ctxs[i].p), 1, (C.c_void_p * 2)(r.d_logs[i][0].data_ptr(), None), (C.c_int * 2)(*counts),
        (C.c_void_p * 1)(g.data_ptr()), (C.c_long * 1)(gp_), (C.c_int * 1)(n_out), (C.c_void_p * 1)(x.data_ptr()), (C.c_long * 1)(xp_), (C.c_int * 1)(n_in))
    top = r.L.artamdStretchLogCapacity(*CTOR, 0, frames, 2.0, 0)
    assert call((top + 1, 0), gp, made, xp, frames) == -1         # a log count above its cap
    assert call(r.counts[i], made - 1, made, xp, frames) == -1    # a planar pitch below the clip, on either side
    assert call(r.counts[i], gp, made, frames - 1, frames) == -1
    assert call(r.counts[i], gp, made, xp, 0) == 0                # no frames: no launch
    # the forward: a log cap below the capacity
    xin, xpitch = put(torch, r.xs[i], True)
    out, opitch = put(torch, np.zeros((0, 2), r.dt), True, room=r.caps[i])
    out_before = out.clone()
    with pytest.raises(RuntimeError):
        r.B.stretch_clips_logged_batch_planar_device([r.ctxs[i]], [xin], [xpitch], [frames], [out], [opitch], [r.caps[i]], [r.ratios[i]],
                                                     [r.d_logs[i]], [[r.log_caps[i][0] - 1, 0]])
    torch.cuda.synchronize()
    assert torch.equal(x, before) and torch.equal(out, out_before)
    assert mirrors(r.ctxs[i].p) == r.state[i] and r.L.artamdErrorCount() == errors
    assert call(r.counts[i], gp, made, xp, frames) == 1           # the same lists are taken when they are right
    torch.cuda.synchronize()
    assert np.array_equal(bits(get(x, xp, frames, 2)[0]), bits(adjoint(r, [i], [gy], [made], [frames], False, False)[1][0]))


# ---- 7. autograd ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,ch", GRID)
def test_clip_stretcher_is_attached_to_the_graph_and_its_gradient_is_the_adjoint(width, ch):
    import torch
    r = run(width, ch)
    B = r.B
    picks = [1, 9, 3, 8, 5]                                       # ratios 0.8, 3.1, 1.25, 0.3, 2.0: both pools in the one call
    T = 5000
    lengths = [CASES[i][2] for i in picks]
    ratios = [CASES[i][1] for i in picks]
    x0 = torch.from_numpy(np.ascontiguousarray(clip(T, ch, r.dt).T)).to("cuda").unsqueeze(0).repeat(len(picks), 1, 1)
    cs = B.ClipStretcher(ch, RATE, segments=True)
    with torch.no_grad():
        y0, len0, maps0 = cs(x0.clone().requires_grad_(), ratios, lengths)
    plain = B.ClipStretcher(ch, RATE)
    y1, len1 = plain(x0, ratios, lengths)
    assert y0.grad_fn is None and y1.grad_fn is None
    x = x0.clone().requires_grad_()
    y, out_lengths, maps = cs(x, ratios, lengths)
    assert y.grad_fn is not None and not out_lengths.requires_grad
    assert torch.equal(y.detach(), y0) and torch.equal(y0, y1) and out_lengths.tolist() == len0.tolist() == len1.tolist() == [r.made[i] for i in picks]
    for k, i in enumerate(picks):                                 # the time map: the records of the direct call
        assert len(maps[k]) == len(r.logs[i]) == len(maps0[k])
        for a, b, c in zip(maps[k], r.logs[i], maps0[k]):
            assert a.dtype == np.int32 and np.array_equal(a, b) and np.array_equal(a, c), i
        assert np.array_equal(bits(y[k, :, :r.made[i]].detach().cpu().numpy().T), bits(r.out[i][0])), i
    gy = torch.from_numpy(np.random.default_rng(11).standard_normal(tuple(y.shape)).astype(r.dt)).to("cuda")
    y.backward(gy)
    torch.cuda.synchronize()
    assert x.grad.shape == x.shape
    _, want, _ = adjoint(r, picks, [gy[k, :, :r.made[i]].cpu().numpy().T for k, i in enumerate(picks)], [r.made[i] for i in picks], lengths, True, True)
    for k, i in enumerate(picks):
        got = x.grad[k].cpu().numpy().T
        assert np.array_equal(bits(got[:lengths[k]]), bits(want[k])), i
        assert (bits(got[lengths[k]:]) == 0).all(), i             # zero at and past lengths[i]
    # a gradient that is not contiguous along T goes through .contiguous()
    x2 = x0.clone().requires_grad_()
    y2, _, _ = cs(x2, ratios, lengths)
    y2.backward(gy.transpose(1, 2).contiguous().transpose(1, 2))
    assert torch.equal(x2.grad, x.grad)
    with pytest.raises(RuntimeError):                             # (once differentiable)
        x3 = x0.clone().requires_grad_()
        (g3,) = torch.autograd.grad(cs(x3, ratios, lengths)[0].sum(), x3, create_graph=True)
        g3.sum().backward()
    y4 = cs(x0.clone().requires_grad_(), ratios, lengths)[0]
    cs.close(); plain.close()
    with pytest.raises(RuntimeError):
        y4.sum().backward()


def test_stretcher_then_resampler_is_differentiable_end_to_end():
    import torch
    import audio_resampler_amd as A
    r = run(32, 2)
    picks, T = [3, 9], 4500
    lengths, ratios = [CASES[i][2] for i in picks], [CASES[i][1] for i in picks]
    x = torch.from_numpy(np.ascontiguousarray(clip(T, 2, np.float32).T)).to("cuda").unsqueeze(0).repeat(2, 1, 1).requires_grad_()
    cs, rs = A.ClipStretcher(2, RATE), A.ClipResampler(2, RATE, RATE * 3 // 4, taps=64, filters=64)
    y, y_len = cs(x, ratios, lengths)
    z, z_len = rs(y, y_len)
    assert z.grad_fn is not None
    w = torch.from_numpy(np.random.default_rng(12).standard_normal(tuple(z.shape)).astype(np.float32)).to("cuda")
    (z * w).sum().backward()
    # by hand: the resampler's adjoint on w, then the stretcher's on that
    yd = y.detach().clone().requires_grad_()
    z2, _ = rs(yd, y_len)
    (z2 * w).sum().backward()
    torch.cuda.synchronize()
    made = [r.made[i] for i in picks]
    assert y_len.tolist() == made
    _, want, _ = adjoint(r, picks, [yd.grad[k, :, :m].cpu().numpy().T for k, m in enumerate(made)], made, lengths, True, False)
    for k in range(2):
        got = x.grad[k].cpu().numpy().T
        assert np.array_equal(bits(got[:lengths[k]]), bits(want[k])) and (got[lengths[k]:] == 0).all(), k
        assert np.abs(got).max() > 0
    cs.close(); rs.close()
