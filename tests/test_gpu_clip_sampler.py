"""GPU: resampleSampleClipsPlanarDevice, resampleSampleAdjointClipsPlanarDevice, resampleSamplePositionGradientClipsPlanarDevice and
ClipSampler.  The yardstick is tests/_sampler_ref.py (the strict CPU oracle's bank, restated in float64; tests/test_sampler_ref.py holds it
to the oracle), never the library's own forward.  The bounds are derived, not measured:

forward    4-byte build |y - ys| <= 2^-24 |ys| + (T + 4) 2^-52 scale (the result's rounding; T fused multiply-adds of a chain against the
           yardstick's own T products and sums, the lerp's three roundings), 8-byte build (T + 6) 2^-53 scale; scale = sum |b x|, lerped.
           An output without a window has scale 0: exactly 0 is asked.
adjoint    |gx - A^T gy| <= (K + 4) u |A|^T |gy| per frame, K the column's entries, u the sample type's unit roundoff: the bound
           tests/test_gpu_clip_adjoint.py applies to expected_gradient.
slope      |gp - ref| <= (C T + C + 2) 2^-52 sum_c |gy| (F sum_t |db x|) per output.
Every buffer a call writes lies between guard bands of a sentinel (and, planar, between rows at a pitch larger than the row), which must
survive; x holds NaN at and past the clip's frames and in the row padding, gy past the outputs.  No position is chosen to make a kernel
fault: every one has a defined result."""
from fractions import Fraction

import numpy as np
import pytest

import audio_resampler_amd as A
from audio_resampler_amd import rate_grad, sampler
import _rate_grad_ref as RG
import _sampler_ref as S
from test_sampler_ref import one_segment_per_phase

pytestmark = pytest.mark.gpu
BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
SAMPLE_TILE = 256          # outputs per task of the forward and the slope: ART_SAMPLE_TILE (art_internal.h), fir_sample.hip's SM_TILE
ADJOINT_TILE = 256         # input frames per task of the adjoint: ADJ_TILE (fir_adjoint_walk.hip.h)
ADJOINT_CHUNK = 256        # outputs per trip of the adjoint's walk through the LDS: ADJ_CHUNK (fir_adjoint_walk.hip.h)
SENTINEL = -777.25
LONG = 600                 # frames of the long clips: more than two input tiles
assert LONG > 2 * ADJOINT_TILE


def np_of(width):
    return np.float64 if width == 64 else np.float32


def unit(width):
    return 2.0 ** -53 if width == 64 else 2.0 ** -24


# ---- buffers between guard bands ----------------------------------------------------------------------------------------------------------
def pack(a, planar, pad, base, width, fill):
    """a [C, n] as a device buffer `base` samples into its allocation — planes n + pad apart (pitch 0 for one channel or interleaved: the
    padding then lies behind the frames), everything that is not a frame of `a` filled with `fill` -> (tensor, address, pitch)"""
    import torch
    Cn, n = a.shape
    if planar and Cn > 1:
        pitch = n + pad
        host = np.full((Cn, pitch), fill, np.float64)
        host[:, :n] = a
        host = host.reshape(-1)
    else:
        pitch = 0
        host = np.concatenate([np.ascontiguousarray(a.T).reshape(-1), np.full(pad * Cn, fill)])
    t = torch.from_numpy(np.concatenate([np.full(base, fill), host, np.full(5, fill)]).astype(np_of(width))).cuda()
    return t, t.data_ptr() + base * t.element_size(), pitch


def unpack(t, Cn, n, pitch, base):
    """the frames [C, n] of such a buffer as float64, and whether everything else still holds the sentinel"""
    h = t.cpu().numpy().astype(np.float64)
    body = h[base:base + (Cn * pitch if pitch else Cn * n)]
    grid = body.reshape(Cn, pitch) if pitch else body.reshape(n, Cn).T
    got = grid[:, :n].copy()
    grid[:, :n] = SENTINEL
    return got, bool(np.all(h == SENTINEL))


def run(width, ctxs, items, planar=True, pad=3, base=1, stream=None, which=("y", "gx", "gp")):
    """the three entries on one batch.  An item: dict(x [C, N_alloc] (NaN at and past n_in), n_in, p [M_alloc], n_out, gy [C, M_alloc] (NaN at and
    past n_out)), and adjoint=False for a curve the adjoint entry is not asked about.  Returns per item dict(y [C, n_out], gx [C, n_in], gp [n_out])."""
    import torch
    SB = sampler.binding(width)
    n = len(items)
    nan = float("nan")
    xs = [pack(it["x"], planar, pad, base, width, nan) for it in items]
    gys = [pack(it["gy"], planar, pad, base, width, nan) for it in items]
    ps = [torch.from_numpy(np.concatenate([it["p"], [nan]])).cuda() for it in items]
    n_in, n_out = [it["n_in"] for it in items], [it["n_out"] for it in items]
    chans = [it["x"].shape[0] for it in items]
    out = [dict() for _ in items]
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    if "y" in which:
        ys = [pack(np.full((c, m), SENTINEL), planar, pad, base, width, SENTINEL) for c, m in zip(chans, n_out)]
        launches = SB.sample_clips_planar_device(ctxs, [v[1] for v in xs], [v[2] for v in xs], n_in, ps, n_out, [v[1] for v in ys], [v[2] for v in ys])
        assert launches == (1 if any(n_out) else 0)
    if "gx" in which:
        asked = [i for i in range(n) if items[i].get("adjoint", True)]
        gxs = {i: pack(np.full((chans[i], n_in[i]), SENTINEL), planar, pad, base, width, SENTINEL) for i in asked}
        launches = SB.sample_adjoint_clips_planar_device([ctxs[i] for i in asked], [ps[i] for i in asked], [n_out[i] for i in asked],
                                                         [gys[i][1] for i in asked], [gys[i][2] for i in asked],
                                                         [gxs[i][1] for i in asked], [gxs[i][2] for i in asked], [n_in[i] for i in asked])
        assert launches == (1 if any(n_out[i] and n_in[i] for i in asked) else 0)
    if "gp" in which:
        gps = [torch.full((m + 4,), SENTINEL, dtype=torch.float64, device="cuda") for m in n_out]
        launches = SB.sample_position_gradient_clips_planar_device(ctxs, [v[1] for v in xs], [v[2] for v in xs], n_in, ps, n_out,
                                                                   [v[1] for v in gys], [v[2] for v in gys], [g.data_ptr() + 16 for g in gps])
        assert launches == (1 if any(n_out) else 0)
    (stream or torch.cuda.current_stream()).synchronize()
    torch.cuda.synchronize()
    for i in range(n):
        if "y" in which:
            out[i]["y"], clean = unpack(ys[i][0], chans[i], n_out[i], ys[i][2], base)
            assert clean, ("y: written outside the item's rows", i)
        if "gx" in which and i in gxs:
            got, clean = unpack(gxs[i][0], chans[i], n_in[i], gxs[i][2], base)
            assert clean, ("gx: written outside the item's rows", i)
            # (an item without outputs is no part of the launch: the adjoint zeroes nothing)
            assert n_out[i] or np.all(got == SENTINEL)
            out[i]["gx"] = got if n_out[i] else np.zeros_like(got)
        if "gp" in which:
            h = gps[i].cpu().numpy()
            assert np.all(h[:2] == SENTINEL) and np.all(h[2 + n_out[i]:] == SENTINEL), ("gp: written outside the item's doubles", i)
            out[i]["gp"] = h[2:2 + n_out[i]].copy()
    return out


# ---- the curves -----------------------------------------------------------------------------------------------------------------------------
def curves(T, F):
    """(name, frames, positions, the adjoint entry may be asked) — every curve non-decreasing unless said otherwise"""
    half = T // 2
    made = []
    for ratio in (0.37, 1.0, 48000 / 44100, 2.5):
        for d in (0.0, 0.25, -float(half), LONG - 3.0):
            count = int(np.ceil((LONG + half + 2 - d) * ratio)) + 3       # (runs a few outputs past the last window)
            made.append((f"affine-{ratio:.3g}{d:+g}", LONG, np.arange(count) / ratio + d, True))
    for frames in (0, 1, 5):                                          # (shorter than any T here)
        made.append((f"short-{frames}", frames, np.arange(frames + T + 6) * 0.75 - half - 2.0, True))
    made.append(("constant", LONG, np.full(3 * SAMPLE_TILE + 1, LONG / 3 + 0.3), True))        # every output on one position: M terms per frame of the window
    m = np.arange(700.0)
    made.append(("sine-warp", LONG, 0.85 * m + 20.0 * np.sin(2 * np.pi * m / 200.0), True))     # (slope 0.85 +- 0.63: monotone)
    made.append(("decreasing", LONG, LONG + half - 0.5 - 0.9 * m, False))
    k = np.arange(6 * F + 3.0)
    made.append(("boundaries", LONG, 100.0 + k / F, True))           # on (or a rounding beside) the filter boundaries, integers among them
    made.append(("integers", 5, np.arange(-half - 1.0, 5.0 + half + 1.0), True))
    p = 2.0 ** -40
    edges = [-np.inf, -1e300, -(half + 1) - p, -(half + 1.0), -half - 0.5, -1e-30, 0.0, 2.25, LONG - 1.0, LONG + half - 1.0, LONG + half - p,
             float(LONG + half), 1e300, np.inf, np.nan]
    made.append(("edges", LONG, np.array(edges), True))
    return made


def make_items(T, F, channels, width, seed):
    rng = np.random.default_rng(seed)
    items = []
    for name, frames, p, adjoint in curves(T, F):
        x = np.full((channels, frames + 4), np.nan)
        x[:, :frames] = (0.25 * rng.standard_normal((channels, frames))).astype(np_of(width))
        gy = rng.standard_normal((channels, len(p))).astype(np_of(width)).astype(np.float64)
        items.append(dict(name=name, x=x, n_in=frames, p=p, n_out=len(p), gy=gy, adjoint=adjoint))
    return items


def check(width, T, F, lowpass, flags, it, got, what=("y", "gx", "gp")):
    """one item's results against the yardstick; returns the worst error / bound of each"""
    Cn = it["x"].shape[0]
    n_in, n_out = it["n_in"], it["n_out"]
    ref = S.sample(T, F, lowpass, flags, it["x"][:, :n_in], it["p"][:n_out], it["gy"][:, :n_out], width, operator="gx" in what and "gx" in got)
    worst = {}
    if "y" in what:
        bound = (T + 6) * 2.0 ** -53 * ref.scale if width == 64 else 2.0 ** -24 * np.abs(ref.ys) + (T + 4) * 2.0 ** -52 * ref.scale
        err = np.abs(got["y"] - ref.ys)
        assert np.all(np.isfinite(got["y"])), it["name"]
        assert np.all(err <= bound), (it["name"], "y", float(err.max()), np.argwhere(err > bound)[:4].tolist())
        assert np.all(got["y"][:, ~ref.live] == 0)
        worst["y"] = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    if "gx" in what and "gx" in got:
        bound = (ref.entries + 4) * unit(width) * ref.gx_scale
        err = np.abs(got["gx"] - ref.gx)
        assert np.all(err <= bound), (it["name"], "gx", float(err.max()), np.argwhere(err > bound)[:4].tolist())
        worst["gx"] = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    if "gp" in what and "gp" in got:
        bound = (Cn * T + Cn + 2) * 2.0 ** -52 * ref.gp_scale
        err = np.abs(got["gp"] - ref.gp)
        assert np.all(err <= bound), (it["name"], "gp", float(err.max()), np.argwhere(err > bound)[:4].tolist())
        assert np.all(got["gp"][~ref.live] == 0)
        worst["gp"] = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    return ref, worst


CONFIGS = [
    ("8x4-lowpass", 8, 4, 0.45, BH | IN | LP, 2),
    ("16x16-mono", 16, 16, 0.45, BH | IN | LP, 1),
    ("16x16-five-channels", 16, 16, 0.0, BH | IN, 5),
    ("32x7", 32, 7, 0.45, BH | IN | LP, 2),
    ("16x16-nearest-filter", 16, 16, 0.45, BH | LP, 2),
    ("16x16-pass-through", 16, 16, 0.0, BH, 2),
]


# ---- 1. the three entries against the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,T,F,lowpass,flags,channels", CONFIGS, ids=[c[0] for c in CONFIGS])
@pytest.mark.parametrize("width", [32, 64])
def test_entries_match_the_yardstick(width, name, T, F, lowpass, flags, channels):
    pytest.importorskip("torch")
    B = A.binding(width)
    items = make_items(T, F, channels, width, 40 + T)
    assert len(items) >= 5 and max(it["n_out"] for it in items) > 2 * SAMPLE_TILE and max(it["n_out"] for it in items) > 2 * ADJOINT_CHUNK
    assert any(it["n_in"] < T and it["n_in"] for it in items) and any(it["n_in"] == 0 for it in items)
    ctx = B.Resampler(channels, T, F, lowpass, flags)
    which = ("y", "gx", "gp") if flags & IN else ("y", "gx")
    got = run(width, [ctx] * len(items), items, which=which)
    worst = {}
    for it, g in zip(items, got):
        ref, w = check(width, T, F, lowpass, flags, it, g, which)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if it["name"] == "constant":                              # (duplicate positions: every frame of the window receives all M terms)
            assert ref.entries.max() == it["n_out"] and 1 <= np.count_nonzero(ref.entries) <= T
        if it["name"] == "edges":
            assert ref.live.tolist() == [False] * 3 + [True] * 8 + [False] * 4
            inside = g["y"][:, [5, 6, 7, 8]]
            assert np.all(inside != 0)                            # (just inside the interval: the yardstick's value, above; well inside: not zero)
    print(name, "width", width, "worst error / bound", worst)
    if not flags & IN:                                            # the position gradient refuses a context that does not interpolate
        with pytest.raises(RuntimeError):
            run(width, [ctx], items[:1], which=("gp",))
    ctx.close()


@pytest.mark.parametrize("width", [32, 64])
def test_the_default_filter(width):
    pytest.importorskip("torch")
    B = A.binding(width)
    T = F = 380
    flags = BH | IN | LP
    rng = np.random.default_rng(3)
    items = []
    for ratio, d, count in ((48000 / 44100, 0.0, 700), (0.5, -190.0, 420)):
        x = np.full((2, LONG + 4), np.nan)
        x[:, :LONG] = (0.25 * rng.standard_normal((2, LONG))).astype(np_of(width))
        items.append(dict(name=f"default-{ratio:.3g}", x=x, n_in=LONG, p=np.arange(count) / ratio + d, n_out=count,
                          gy=rng.standard_normal((2, count)).astype(np_of(width)).astype(np.float64)))
    ctx = B.Resampler(2, T, F, 0.0, flags)
    got = run(width, [ctx] * 2, items)
    for it, g in zip(items, got):
        _, worst = check(width, T, F, 0.0, flags, it, g)
        print(it["name"], "width", width, "worst error / bound", worst)
    ctx.close()


# ---- 2. the slope's chain, bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_the_slope_is_the_chain_restated(width):
    pytest.importorskip("torch")
    import _oracle as O
    B = A.binding(width)
    T, F, flags = 16, 16, BH | IN | LP
    bank = O.binding(width).OracleResampler(1, T, F, 0.45, flags, kind="strict").bank()
    rng = np.random.default_rng(17)
    N = 40
    x = (0.25 * rng.standard_normal((2, N))).astype(np_of(width)).astype(np.float64)
    p = np.array([-3.5, 0.0, 7.3125, 20.0 + 5.0 / F, 33.99, N + 2.75])
    gy = rng.standard_normal((2, len(p))).astype(np_of(width)).astype(np.float64)
    ctx = B.Resampler(2, T, F, 0.45, flags)
    (got,) = run(width, [ctx], [dict(name="chain", x=x, n_in=N, p=p, n_out=len(p), gy=gy)], which=("gp",))
    ref = S.sample(T, F, 0.45, flags, x, p, gy, width)
    for m in range(len(p)):
        first, fi = int(ref.first[m]), int(ref.fi[m])
        want = 0.0
        for c in range(2):                                        # fma ((double) b_hi - (double) b_lo, x, acc), t ascending; F *; gy *; the channels in order
            acc = 0.0
            for t in range(T):
                if 0 <= first + t < N:
                    d = float(bank[fi + 1][t]) - float(bank[fi][t])
                    acc = float(Fraction(d) * Fraction(float(x[c, first + t])) + Fraction(acc))
            want = want + float(gy[c, m]) * (F * acc)
        assert want != 0.0 and got["gp"][m] == want, (m, got["gp"][m], want)
    ctx.close()


# ---- 3. bits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_bits_do_not_depend_on_batch_place_layout_pitch_or_stream(width):
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    T, F, flags = 16, 16, BH | IN | LP
    items = make_items(T, F, 2, width, 90)
    mine = next(it for it in items if it["name"] == "sine-warp")
    others = [it for it in items if it["name"] in ("short-0", "short-5", "constant", "affine-2.5+0", "affine-0.37-8", "integers")]
    assert len(others) == 6
    ctxs = [B.Resampler(2, T, F, 0.45, flags) for _ in range(3)]
    bits = lambda r: [r[k].view(np.uint64).tolist() for k in ("y", "gx", "gp")]
    (alone,) = run(width, ctxs[:1], [mine])
    assert all(np.count_nonzero(alone[k]) > alone[k].size // 2 for k in ("y", "gx", "gp"))
    first = run(width, [ctxs[0]] * 7, [mine] + others)[0]
    last = run(width, [ctxs[1]] * 3 + [ctxs[0]] * 4, others + [mine])[-1]
    (interleaved,) = run(width, ctxs[:1], [mine], planar=False)
    (tight,) = run(width, ctxs[:1], [mine], pad=0, base=0)
    (wide,) = run(width, ctxs[:1], [mine], pad=29, base=3)
    side = torch.cuda.Stream()
    ctxs[2].set_stream(side.cuda_stream)
    (streamed,) = run(width, [ctxs[2]], [mine], stream=side)
    for other in (first, last, interleaved, tight, wide, streamed):
        assert bits(other) == bits(alone)
    # outputs cut short: the curve ends there, and what lies behind it in p and gy (NaN here) is not read
    cut = mine["n_out"] - 37
    short = dict(mine, p=mine["p"][:cut], gy=mine["gy"][:, :cut], n_out=cut)
    poisoned = dict(mine, p=np.concatenate([mine["p"][:cut], np.full(37, np.nan)]), n_out=cut,
                    gy=np.concatenate([mine["gy"][:, :cut], np.full((2, 37), np.nan)], 1))
    (want,) = run(width, ctxs[:1], [short])
    (got,) = run(width, ctxs[:1], [poisoned])
    assert bits(got) == bits(want) and bits(want)[1] != bits(alone)[1]
    for r in ctxs:
        r.close()


# ---- 4. refusals on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_refusals_on_the_device_enqueue_and_count_nothing(width):
    torch = pytest.importorskip("torch")
    B, SB = A.binding(width), sampler.binding(width)
    errors = B.lib().artamdErrorCount()
    T, F, flags = 16, 16, BH | IN | LP
    dt = torch.float64 if width == 64 else torch.float32
    plain = B.Resampler(1, T, F, 0.45, flags)
    fixed = B.Resampler(1, T, F, 0.0, flags, (44100.0, 48000.0, 0))
    nearest = B.Resampler(1, T, F, 0.45, BH | LP)
    ends = B.Resampler(1, T, F, 0.45, flags | A.EXTRAPOLATE_ENDPOINTS)
    elsewhere = B.Resampler(1, T, F, 0.45, flags)
    side = torch.cuda.Stream()
    elsewhere.set_stream(side.cuda_stream)
    x, g = torch.ones(30, dtype=dt, device="cuda"), torch.ones(20, dtype=dt, device="cuda")
    p = torch.arange(20, dtype=torch.float64, device="cuda")
    y, gx = torch.full((20,), SENTINEL, dtype=dt, device="cuda"), torch.full((30,), SENTINEL, dtype=dt, device="cuda")
    gp = torch.full((20,), SENTINEL, dtype=torch.float64, device="cuda")

    def calls(ctxs, n_in=30, n_out=20, xs=x, ps=p, gs=g, ys=y, gxs=gx, gps=gp):
        k = len(ctxs)
        return ((SB.sample_clips_planar_device, (ctxs, [xs] * k, None, [n_in] * k, [ps] * k, [n_out] * k, [ys] * k, None)),
                (SB.sample_adjoint_clips_planar_device, (ctxs, [ps] * k, [n_out] * k, [gs] * k, None, [gxs] * k, None, [n_in] * k)),
                (SB.sample_position_gradient_clips_planar_device, (ctxs, [xs] * k, None, [n_in] * k, [ps] * k, [n_out] * k, [gs] * k, None, [gps] * k)))

    refused = [calls([ends]), calls([plain, elsewhere]), calls([plain], n_in=-1), calls([plain], n_out=-1), calls([plain], n_in=2 ** 31 - 1 - 2 * T + 1),
               calls([plain], ps=None)]
    for triple in refused:
        for fn, args in triple:
            with pytest.raises(RuntimeError):
                fn(*args)
    for index, more in ((0, dict(xs=None)), (0, dict(ys=None)), (1, dict(gs=None)), (1, dict(gxs=None)), (2, dict(xs=None)), (2, dict(gs=None)), (2, dict(gps=None))):
        fn, args = calls([plain], **more)[index]
        with pytest.raises(RuntimeError):
            fn(*args)
    fn, args = calls([nearest])[2]                                # (the position gradient of a nearest-filter context)
    with pytest.raises(RuntimeError):
        fn(*args)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (y, gx, gp)) and B.lib().artamdErrorCount() == errors
    # taken: a fixed-ratio context (only its bank is used), the nearest filter's forward and adjoint, one context listed twice
    for triple in (calls([fixed]), calls([plain, plain])):
        assert [fn(*args) for fn, args in triple] == [1, 1, 1]
    assert [fn(*args) for fn, args in calls([nearest])[:2]] == [1, 1]
    # nothing live: no launch, nothing written (the adjoint: an item without frames or without outputs)
    y.fill_(SENTINEL); gx.fill_(SENTINEL); gp.fill_(SENTINEL)
    assert [fn(*args) for fn, args in calls([plain], n_out=0)] == [0, 0, 0]
    assert calls([plain], n_in=0)[1][0](*calls([plain], n_in=0)[1][1]) == 0
    assert calls([plain], n_in=0, xs=None)[0][0](*calls([plain], n_in=0, xs=None)[0][1]) == 1      # (no frames: silence, and no buffer is needed)
    torch.cuda.synchronize()
    assert bool((gx == SENTINEL).all()) and bool((gp == SENTINEL).all()) and bool((y == 0).all()) and B.lib().artamdErrorCount() == errors
    for r in (plain, fixed, nearest, ends, elsewhere):
        r.close()


# ---- 5. ClipSampler ---------------------------------------------------------------------------------------------------------------------------
def sampler_case(width, seed=5):
    """x [3, 2, 600] with lengths, a monotone curve per clip and a gradient of y, as numpy in the build's sample type"""
    rng = np.random.default_rng(seed)
    lengths, M = [LONG, 41, 300], 2 * ADJOINT_CHUNK + 150
    xh = (0.25 * rng.standard_normal((3, 2, LONG))).astype(np_of(width))
    m = np.arange(float(M))
    ph = np.stack([0.9 * m - 8.0, 0.07 * m - 3.0 + np.sin(m / 40.0), 0.45 * m + 0.125])
    gh = rng.standard_normal((3, 2, M)).astype(np_of(width))
    return lengths, M, xh, ph, gh


def poisoned(xh, lengths):
    out = xh.copy()
    for i, n in enumerate(lengths):
        out[i, :, n:] = np.nan
    return out


@pytest.mark.parametrize("width", [32, 64])
def test_clip_sampler_forward_and_both_gradients(width, monkeypatch):
    torch = pytest.importorskip("torch")
    SB = sampler.binding(width)
    T, F, flags, lowpass = 16, 16, BH | IN | LP, 0.45
    lengths, M, xh, ph, gh = sampler_case(width)
    outs = [M, M - 100, 77]
    sorts = []
    real_sort = torch.sort
    monkeypatch.setattr(torch, "sort", lambda *a, **k: (sorts.append(1), real_sort(*a, **k))[1])      # (counts the calls; torch's own, not the library's)
    clip = SB.ClipSampler(2, T, F, flags, lowpass)
    x = torch.from_numpy(poisoned(xh, lengths)).cuda().requires_grad_()
    p = torch.from_numpy(ph).cuda().requires_grad_()
    g = torch.from_numpy(gh).cuda()
    g_poisoned = g.clone()
    for i, n in enumerate(outs):
        g_poisoned[i, :, n:] = float("nan")
    with torch.no_grad():
        quiet = clip(x, p, lengths, outs)
    assert quiet.grad_fn is None and not quiet.requires_grad
    y = clip(x, p, lengths, outs)
    assert y.shape == (3, 2, M) and y.dtype == x.dtype and y.grad_fn is not None and torch.equal(y.detach(), quiet)
    y.backward(g_poisoned)                                        # (grad_y at and past out_lengths is not read)
    assert sorts == [], "a monotone curve was sorted"
    assert x.grad.shape == x.shape and p.grad.shape == p.shape and p.grad.dtype == torch.float64
    for i, (n, k) in enumerate(zip(lengths, outs)):
        assert bool((y[i, :, k:] == 0).all()) and bool((x.grad[i, :, n:] == 0).all()) and bool((p.grad[i, k:] == 0).all())
        it = dict(name=f"clip-{i}", x=xh[i].astype(np.float64), n_in=n, p=ph[i], n_out=k, gy=gh[i].astype(np.float64))
        got = dict(y=y[i, :, :k].detach().cpu().numpy().astype(np.float64), gx=x.grad[i, :, :n].cpu().numpy().astype(np.float64),
                   gp=p.grad[i, :k].cpu().numpy())
        _, worst = check(width, T, F, lowpass, flags, it, got)
        print("ClipSampler width", width, "clip", i, "worst error / bound", worst)
    monotone = x.grad.clone()

    # the same outputs in reverse order (a strictly decreasing curve among them: reverse playback): backward sorts, and meets the same bound
    xr = torch.from_numpy(poisoned(xh, lengths)).cuda().requires_grad_()
    pr = torch.from_numpy(np.ascontiguousarray(ph[:, ::-1])).cuda().requires_grad_()
    yr = clip(xr, pr, lengths)
    yr.backward(torch.from_numpy(np.ascontiguousarray(gh[:, :, ::-1])).cuda())
    assert len(sorts) == 1, "a decreasing curve was not sorted (or sorted more than once)"
    for i, n in enumerate(lengths):
        it = dict(name=f"reversed-{i}", x=xh[i].astype(np.float64), n_in=n, p=ph[i, ::-1], n_out=M, gy=gh[i, :, ::-1].astype(np.float64))
        got = dict(y=yr[i].detach().cpu().numpy().astype(np.float64), gx=xr.grad[i, :, :n].cpu().numpy().astype(np.float64), gp=pr.grad[i].cpu().numpy())
        _, worst = check(width, T, F, lowpass, flags, it, got)
        print("ClipSampler width", width, "reversed clip", i, "worst error / bound", worst)
    assert bool((xr.grad[0] != 0).any()) and monotone.shape == xr.grad.shape

    # x alone, positions alone: only the call that is needed; a curve for every clip, in float32: gradients of their own shape and dtype
    del sorts[:]
    shared = torch.from_numpy(ph[2].astype(np.float32)).cuda().requires_grad_()
    x2 = torch.from_numpy(xh).cuda()
    y2 = clip(x2, shared, lengths)
    y2.backward(g)
    assert shared.grad.shape == (M,) and shared.grad.dtype == torch.float32 and x2.grad is None and sorts == []
    want, slack, size = np.zeros(M), np.zeros(M), np.zeros(M)
    for i, n in enumerate(lengths):
        ref = S.sample(T, F, lowpass, flags, xh[i, :, :n].astype(np.float64), shared.detach().cpu().numpy().astype(np.float64), gh[i].astype(np.float64), width)
        want, slack, size = want + ref.gp, slack + (2 * T + 4) * 2.0 ** -52 * ref.gp_scale, size + np.abs(ref.gp)
    err = np.abs(shared.grad.cpu().numpy().astype(np.float64) - want)
    # (autograd narrows every clip's row to float32 first — 2^-24 of each — and then adds the three in float32: two sums, 2^-24 of a partial sum each)
    assert np.all(err <= slack + 3 * 2.0 ** -24 * size), float(err.max())
    x3 = torch.from_numpy(xh).cuda().requires_grad_()
    y3 = clip(x3, torch.from_numpy(ph).cuda(), lengths)
    y3.backward(g)
    assert x3.grad.shape == (3, 2, LONG) and torch.equal(x3.grad, clip_grad_x(clip, xh, ph, g, lengths)) and sorts == []
    # [C, T] in, one clip out; no clip at all
    y1 = clip(torch.from_numpy(xh[0]).cuda(), torch.from_numpy(ph[0]).cuda())
    assert y1.shape == (1, 2, M)
    empty = SB.ClipSampler(2, T, F, flags, lowpass)
    x0 = torch.zeros(0, 2, 10, dtype=x.dtype, device="cuda", requires_grad=True)
    p0 = torch.zeros(7, dtype=torch.float64, device="cuda", requires_grad=True)
    y0 = empty(x0, p0)
    y0.sum().backward()
    assert y0.shape == (0, 2, 7) and x0.grad.shape == (0, 2, 10) and p0.grad.shape == (7,) and not bool(p0.grad.any()) and empty.pool == []
    with pytest.raises(RuntimeError):                             # (once differentiable)
        y4 = clip(x3, p, lengths)
        (gp4,) = torch.autograd.grad((y4 * g).sum(), p, create_graph=True)
        gp4.sum().backward()
    # backward after close () raises
    y5 = clip(x3, p, lengths)
    clip.close()
    with pytest.raises(RuntimeError):
        y5.sum().backward()


def clip_grad_x(clip, xh, ph, g, lengths):
    """the x gradient once more, from a fresh graph: the same call, the same bits"""
    import torch
    x = torch.from_numpy(xh).cuda().requires_grad_()
    clip(x, torch.from_numpy(ph).cuda(), lengths).backward(g)
    return x.grad


# ---- 6. gradcheck ---------------------------------------------------------------------------------------------------------------------------
def test_gradcheck_in_the_samples_and_the_positions_on_the_8_byte_build():
    torch = pytest.importorskip("torch")
    SB = sampler.binding(64)
    T, F, flags, eps = 16, 16, BH | IN, 2.0 ** -20
    lengths = [24, 17]
    xh = 0.25 * np.random.default_rng(81).standard_normal((2, 1, 24))
    # positions whose frac F stays 2^-10 + eps F away from every integer: no interpolation cell changes under the probe — asserted from
    # the yardstick's cell at p +- eps
    k = np.arange(12.0)
    ph = np.stack([-6.0 + 2.75 * k + (0.3 + 0.31 * (k % 2)) / F, 20.0 - 1.625 * k + 0.45 / F])        # (the second runs backwards: the sorted path)
    margin = 2.0 ** -10 + eps * F
    fr = (ph - np.floor(ph)) * F
    assert np.all(np.abs(fr - np.round(fr)) >= margin)
    slopes = []
    for i, n in enumerate(lengths):
        lo, mid, hi = (S.sample(T, F, 0.0, flags, xh[i][:, :n], ph[i] + d) for d in (-eps, 0.0, eps))
        assert np.array_equal(lo.cell, mid.cell) and np.array_equal(hi.cell, mid.cell) and np.array_equal(lo.live, hi.live)
        slopes.append(np.abs(mid.D).max())
    # as tests/test_gpu_clip_rate_grad.py takes it: 1e-7 of the largest slope for an entry of the Jacobian (an output's D, or a filter weight)
    tol = 1e-7 * max(slopes)
    clip = SB.ClipSampler(1, T, F, flags, 0.0)
    x = torch.from_numpy(xh).cuda().requires_grad_()
    p = torch.from_numpy(ph).cuda().requires_grad_()
    print("eps", eps, "atol", tol)
    assert torch.autograd.gradcheck(lambda t, q: clip(t, q, lengths), (x, p), eps=eps, atol=tol, rtol=1e-7)
    clip.close()


# ---- 7. ties to the clip classes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [48000 / 44100, 0.37], ids=str)
@pytest.mark.parametrize("width", [32, 64])
def test_at_the_clip_entries_positions_the_sampler_is_clip_warper(width, ratio):
    torch = pytest.importorskip("torch")
    B, SB = A.binding(width), sampler.binding(width)
    T, F, flags, lowpass, N = 16, 16, BH | IN | LP, 0.45, 160
    nseg, counts = one_segment_per_phase(T, F, flags, N, ratio)
    assert nseg == (1, 1)                                         # (one block, one ring segment per phase: off - T is exact)
    p = S.aligned_positions(counts, (ratio,), T)
    M = len(p)
    rng = np.random.default_rng(31)
    xh = (0.25 * rng.standard_normal((1, 2, N))).astype(np_of(width))
    gh = rng.standard_normal((1, 2, M)).astype(np_of(width))
    warper, clip = B.ClipWarper(2, T, F, flags, lowpass, block=N), SB.ClipSampler(2, T, F, flags, lowpass)
    xw, xs = torch.from_numpy(xh).cuda().requires_grad_(), torch.from_numpy(xh).cuda().requires_grad_()
    yw, made = warper(xw, ratio)
    assert made.tolist() == [M]
    ys = clip(xs, torch.from_numpy(p).cuda())
    ref = S.sample(T, F, lowpass, flags, xh[0].astype(np.float64), p, width=width)
    # the warper's kernels sum in the sample type: T products and sums of it, the lerp, the result
    for name, y, bound in (("ClipSampler", ys, (T + 6) * 2.0 ** -53 * ref.scale if width == 64 else 2.0 ** -24 * np.abs(ref.ys) + (T + 4) * 2.0 ** -52 * ref.scale),
                           ("ClipWarper", yw, (T + 6) * unit(width) * ref.scale)):
        err = np.abs(y[0].detach().cpu().numpy().astype(np.float64) - ref.ys)
        print(name, "width", width, "ratio", ratio, "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (name, float(err.max()))
    g = torch.from_numpy(gh).cuda()
    yw.backward(g); ys.backward(g)
    assert torch.equal(xw.grad, xs.grad)                          # (the same weights in the same order: adj_walk, both)
    warper.close(); clip.close()


@pytest.mark.parametrize("width", [32, 64])
def test_a_ratio_in_front_of_the_sampler_gets_clip_rate_warpers_gradient(width):
    torch = pytest.importorskip("torch")
    SB, RW = sampler.binding(width), rate_grad.binding(width)
    T, F, flags, lowpass, N, ratio = 16, 16, BH | IN | LP, 0.45, 160, 1.3071
    half = T // 2
    nseg, counts = one_segment_per_phase(T, F, flags, N, ratio)
    assert nseg == (1, 1)
    made, M = counts[0], sum(counts)
    rng = np.random.default_rng(37)
    xh = (0.25 * rng.standard_normal((1, 2, N))).astype(np_of(width))
    gh = rng.standard_normal((1, 2, M)).astype(np_of(width))
    gh[:, :, made:] = 0.0                                         # (the flush's outputs held apart: they move with the count the warper holds fixed)
    x, g = torch.from_numpy(xh).cuda(), torch.from_numpy(gh).cuda()
    warper, clip = RW.ClipRateWarper(2, T, F, flags, lowpass, block=N), SB.ClipSampler(2, T, F, flags, lowpass)
    rw = torch.tensor(ratio, dtype=torch.float64, device="cuda", requires_grad=True)
    yw, lengths = warper(x, rw)
    assert lengths.tolist() == [M]
    (yw * g).sum().backward()
    rs = torch.tensor(ratio, dtype=torch.float64, device="cuda", requires_grad=True)
    p = (half - T) + torch.arange(M, dtype=torch.float64, device="cuda") / rs
    ys = clip(x, p[None, :], out_lengths=[made])
    (ys * g).sum().backward()
    ref = RG.clip(T, F, lowpass, flags, (N,), (ratio,), xh[0].astype(np.float64), gh[0].astype(np.float64), width)
    tol = ref.terms[0] * (M + 4) * 2.0 ** -52 + 2.0 ** -53 * abs(ref.grad[0])
    print("width", width, "ClipRateWarper", float(rw.grad), "through ClipSampler", float(rs.grad), "yardstick", ref.grad[0], "tolerance", tol)
    assert float(rw.grad) != 0.0 and abs(float(rs.grad) - float(rw.grad)) <= tol and abs(float(rs.grad) - ref.grad[0]) <= tol
    warper.close(); clip.close()
