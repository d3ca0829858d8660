"""GPU: resampleSampleBandClipsPlanarDevice, resampleSampleBandAdjointClipsPlanarDevice, resampleSampleBandGradientsClipsPlanarDevice and
ClipBandSampler.  The yardstick is tests/_band_ref.py: tests/_sampler_ref.py's `sample` per rung, blended in float64 by art_hip.h's
definitions (tests/test_band_ref.py holds it to the sampler's yardstick) — never the library's own output.  The bounds are derived, not
measured; u is the sample type's unit roundoff, T the taps, C the channels, `scale` the yardstick's sum |b x| lerped, per rung:

forward    the sampler's bound for each rung's a_k (tests/test_gpu_clip_sampler.py), which the blend carries to the scale blended by lam, and
           the blend's own roundings: a_L (1 - lam), a_{L+1} lam and their sum, 2^-53 each of at most the blended scale, on the device and
           again in the yardstick — 3 * 2^-52 of it ((1.0 - lam) is the same double on both sides).  4-byte build
           |y - ys| <= 2^-24 |ys| + (T + 7) 2^-52 scale; 8-byte build (T + 6 + 6) 2^-53 scale.  Where lam == 0 nothing is blended and the
           sampler's own bound would do; the wider one is asked everywhere.  Without a window scale is 0: exactly 0 is asked.
adjoint    |gx - A^T gy| <= (entries + 6) u |A|^T |gy| per frame, A the yardstick's blended and rounded weights: the sampler's
           (entries + 4) and two more for what the blend's roundings in double can move a weight's rounding to the sample type by.
slope      the sampler's (C T + C + 2) 2^-52 on the blended slope scale, and the blend's three roundings per channel as above:
           |gp - ref| <= (C T + C + 5) 2^-52 sum_c |gy| slope_scale.
level      gl = sum_c gy (a_{j+1} - a_j): per channel two values, each with the forward's (T + 4) 2^-52 scale_k, their difference (one
           rounding of at most scale_j + scale_{j+1}), the product with gy and the sum over the channels:
           |gl - ref| <= (2 C (T + 4) + C + 2) 2^-52 sum_c |gy| (scale_j + scale_{j+1}); exactly 0 where the level does not move
           (outside [0, K - 1], a NaN, K = 1, no window).
Every buffer a call writes lies between guard bands of a sentinel, which must survive; x holds NaN at and past the clip's frames and in the
row padding, gy, positions and levels past the outputs.  No position or level is chosen to make a kernel fault: every one has a defined
result."""
import numpy as np
import pytest

import audio_resampler_amd as A
from audio_resampler_amd import band
import _band_ref as BR
from test_gpu_clip_sampler import ADJOINT_CHUNK, LONG, SAMPLE_TILE, SENTINEL, curves, np_of, pack, unit, unpack
from test_gpu_clip_sampler import run as sampler_run

pytestmark = pytest.mark.gpu
BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
FLAGS = BH | IN | LP
DEFAULT = (1.0, 2 ** -0.5, 0.5, 2 ** -1.5, 0.25)
LADDERS = {1: (0.9,), 2: (1.0, 0.5), 3: (1.0, 0.6, 0.3), 8: tuple(2.0 ** (-k / 2) for k in range(8))}
LEVEL_TOLERANCE = 2.0 ** -44       # tests/test_clip_band_abi.py: what two restatements of levels_of may differ by


def contexts(width, channels, T, F, cutoffs):
    """a ladder as ClipBandSampler makes it (resampleInit clears INCLUDE_LOWPASS at 1.0)"""
    return [A.binding(width).Resampler(channels, T, F, c, FLAGS) for c in cutoffs]


def edge_levels(K):
    return [-np.inf, -1.0, -0.0, 0.0, 2.0 ** -60, 1 - 2.0 ** -53, 1.0, K - 1 - 2.0 ** -40, K - 1.0, float(K), np.inf, np.nan]


def level_curve(kind, M, K, rng):
    m = np.arange(M)
    if kind == "random":
        return rng.uniform(0.0, K - 1.0, M)
    if kind == "ramp":                                            # through every whole level, and past both ends, in steps of 1/8
        return (m * 0.125) % (K + 1.0) - 1.0
    if kind == "edges":
        return np.array(edge_levels(K))[m % 12]
    return np.full(M, float(kind))


# ---- the three entries on one batch ---------------------------------------------------------------------------------------------------------
def run(width, ladders, items, planar=True, pad=3, base=1, stream=None, which=("y", "gx", "gp", "gl")):
    """An item: dict(x [C, N_alloc] (NaN at and past n_in), n_in, p [M_alloc], levels [M_alloc], n_out, gy [C, M_alloc]), and adjoint=False for
    a curve the adjoint entry is not asked about; ladders [i]: item i's K contexts.  Returns per item dict(y, gx, gp, gl)."""
    import torch
    SB = band.binding(width)
    n, K = len(items), len(ladders[0])
    nan = float("nan")
    flat = lambda idx: [c for i in idx for c in ladders[i]]
    xs = [pack(it["x"], planar, pad, base, width, nan) for it in items]
    gys = [pack(it["gy"], planar, pad, base, width, nan) for it in items]
    ps = [torch.from_numpy(np.concatenate([it["p"], [nan]])).cuda() for it in items]
    ls = [torch.from_numpy(np.concatenate([it["levels"], [nan]])).cuda() for it in items]
    n_in, n_out = [it["n_in"] for it in items], [it["n_out"] for it in items]
    chans = [it["x"].shape[0] for it in items]
    out = [dict() for _ in items]
    everyone = list(range(n))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    if "y" in which:
        ys = [pack(np.full((c, m), SENTINEL), planar, pad, base, width, SENTINEL) for c, m in zip(chans, n_out)]
        launches = SB.sample_band_clips_planar_device(flat(everyone), K, [v[1] for v in xs], [v[2] for v in xs], n_in, ps, ls, n_out,
                                                      [v[1] for v in ys], [v[2] for v in ys])
        assert launches == (1 if any(n_out) else 0)
    if "gx" in which:
        asked = [i for i in everyone if items[i].get("adjoint", True)]
        gxs = {i: pack(np.full((chans[i], n_in[i]), SENTINEL), planar, pad, base, width, SENTINEL) for i in asked}
        launches = SB.sample_band_adjoint_clips_planar_device(flat(asked), K, [ps[i] for i in asked], [ls[i] for i in asked], [n_out[i] for i in asked],
                                                              [gys[i][1] for i in asked], [gys[i][2] for i in asked],
                                                              [gxs[i][1] for i in asked], [gxs[i][2] for i in asked], [n_in[i] for i in asked])
        assert launches == (1 if any(n_out[i] and n_in[i] for i in asked) else 0)
    grads = [k for k in ("gp", "gl") if k in which]
    if grads:
        bufs = {k: [torch.full((m + 4,), SENTINEL, dtype=torch.float64, device="cuda") for m in n_out] for k in grads}
        ptrs = {k: [g.data_ptr() + 16 for g in v] for k, v in bufs.items()}
        launches = SB.sample_band_gradients_clips_planar_device(flat(everyone), K, [v[1] for v in xs], [v[2] for v in xs], n_in, ps, ls, n_out,
                                                                [v[1] for v in gys], [v[2] for v in gys], ptrs.get("gp"), ptrs.get("gl"))
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
            assert n_out[i] or np.all(got == SENTINEL)            # (an item without outputs is no part of the launch: nothing is zeroed)
            out[i]["gx"] = got if n_out[i] else np.zeros_like(got)
        for k in grads:
            h = bufs[k][i].cpu().numpy()
            assert np.all(h[:2] == SENTINEL) and np.all(h[2 + n_out[i]:] == SENTINEL), (k + ": written outside the item's doubles", i)
            out[i][k] = h[2:2 + n_out[i]].copy()
    return out


WANTED = {"affine-1.09+0": "random", "affine-2.5+0.25": "ramp", "affine-0.37+0.25": "edges", "sine-warp": "edges", "short-0": "ramp", "short-1": "ramp",
          "short-5": "random", "edges": "ramp", "constant": "ramp", "boundaries": "random", "decreasing": "random"}


def make_items(T, F, channels, K, width, seed, names=WANTED):
    rng = np.random.default_rng(seed)
    items = []
    for name, frames, p, adjoint in curves(T, F):
        if name not in names:
            continue
        x = np.full((channels, frames + 4), np.nan)
        x[:, :frames] = (0.25 * rng.standard_normal((channels, frames))).astype(np_of(width))
        gy = rng.standard_normal((channels, len(p))).astype(np_of(width)).astype(np.float64)
        items.append(dict(name=name, x=x, n_in=frames, p=p, levels=level_curve(names[name], len(p), K, rng), n_out=len(p), gy=gy, adjoint=adjoint))
    assert len(items) == len(names), [it["name"] for it in items]
    return items


def check(width, T, F, rungs, it, got, what=("y", "gx", "gp", "gl")):
    """one item's results against the yardstick; returns it and the worst error / bound of each"""
    Cn = it["x"].shape[0]
    n_in, n_out = it["n_in"], it["n_out"]
    ref = BR.sample(T, F, rungs, it["x"][:, :n_in], it["p"][:n_out], it["levels"][:n_out], it["gy"][:, :n_out], width, operator="gx" in what and "gx" in got)
    worst = {}

    def judge(key, value, bound):
        err = np.abs(got[key] - value)
        assert np.all(np.isfinite(got[key])), (it["name"], key)
        assert np.all(err <= bound), (it["name"], key, float(err.max()), np.argwhere(err > bound)[:4].tolist())
        worst[key] = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0

    if "y" in what:
        judge("y", ref.ys, (T + 12) * 2.0 ** -53 * ref.scale if width == 64 else 2.0 ** -24 * np.abs(ref.ys) + (T + 7) * 2.0 ** -52 * ref.scale)
        assert np.all(got["y"][:, ~ref.live] == 0)
    if "gx" in what and "gx" in got:
        judge("gx", ref.gx, (ref.entries + 6) * unit(width) * ref.gx_scale)
    if "gp" in what:
        judge("gp", ref.gp, (Cn * T + Cn + 5) * 2.0 ** -52 * ref.gp_scale)
        assert np.all(got["gp"][~ref.live] == 0)
    if "gl" in what:
        judge("gl", ref.gl, (2 * Cn * (T + 4) + Cn + 2) * 2.0 ** -52 * ref.gl_scale)
        assert np.all(got["gl"][~ref.moves] == 0)
    return ref, worst


CONFIGS = [
    # (taps, filters, channels, rungs, planar): every C in 1, 2, 3, 5 (the forward's groups of 4; the adjoint's of 4, 2 and 1), K in 1, 2, 3, 8
    (16, 16, 1, 1, True), (16, 16, 2, 2, False), (16, 16, 3, 3, True), (16, 16, 5, 8, False), (64, 64, 2, 3, True), (64, 64, 5, 2, True),
    (64, 64, 1, 8, False),
]


# ---- 1. the three entries against the yardstick ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,F,channels,K,planar", CONFIGS, ids=[f"{c[0]}x{c[1]}-C{c[2]}-K{c[3]}-{'planar' if c[4] else 'interleaved'}" for c in CONFIGS])
@pytest.mark.parametrize("width", [32, 64])
def test_entries_match_the_yardstick(width, T, F, channels, K, planar):
    pytest.importorskip("torch")
    cutoffs = LADDERS[K]
    rungs = BR.ladder(cutoffs, FLAGS)
    items = make_items(T, F, channels, K, width, 100 + T + K)
    assert max(it["n_out"] for it in items) > 2 * SAMPLE_TILE and max(it["n_out"] for it in items) > 2 * ADJOINT_CHUNK and LONG > 2 * 256
    assert {it["n_in"] for it in items} >= {0, 1, 5, LONG}
    ladder = contexts(width, channels, T, F, cutoffs)
    got = run(width, [ladder] * len(items), items, planar=planar)
    worst = {}
    for it, g in zip(items, got):
        ref, w = check(width, T, F, rungs, it, g)
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if it["name"] == "sine-warp":                             # the edge list of levels, on outputs that all have a window
            assert ref.live.all()
            L, lam, moves = BR.decode(edge_levels(K), K)
            assert ref.L[:12].tolist() == L.tolist() and ref.moves[:12].tolist() == moves.tolist()
            if K > 1:
                assert moves.tolist() == [False, False] + [True] * 7 + [False] * 3 and np.all(g["gl"][:12][moves] != 0)
            assert np.all(g["gl"][:12][~moves] == 0) and np.all(g["y"][:, :12] != 0)
        if K > 1 and it["name"] == "affine-1.09+0":              # (random levels: blends nearly everywhere)
            assert np.count_nonzero(ref.lam) > it["n_out"] // 2 and np.count_nonzero(g["gl"]) > it["n_out"] // 2
        if K > 1 and it["name"] == "affine-2.5+0.25":            # (the ramp: whole levels, blends and both ends' outsides)
            assert np.count_nonzero(ref.lam == 0) > it["n_out"] // 8 and np.count_nonzero(ref.lam) > it["n_out"] // 8
    print(f"{T}x{F} C {channels} K {K} width {width} worst error / bound", worst)
    for r in ladder:
        r.close()


@pytest.mark.parametrize("width", [32, 64])
def test_the_default_filter_and_ladder(width):
    pytest.importorskip("torch")
    T = F = 380
    rng = np.random.default_rng(3)
    items = []
    for ratio, d, count, kind in ((48000 / 44100, 0.0, 700, "random"), (0.5, -190.0, 420, "ramp")):
        x = np.full((2, LONG + 4), np.nan)
        x[:, :LONG] = (0.25 * rng.standard_normal((2, LONG))).astype(np_of(width))
        items.append(dict(name=f"default-{ratio:.3g}", x=x, n_in=LONG, p=np.arange(count) / ratio + d, levels=level_curve(kind, count, 5, rng), n_out=count,
                          gy=rng.standard_normal((2, count)).astype(np_of(width)).astype(np.float64)))
    ladder = contexts(width, 2, T, F, DEFAULT)
    got = run(width, [ladder] * 2, items)
    for it, g in zip(items, got):
        _, worst = check(width, T, F, BR.ladder(DEFAULT, FLAGS), it, g)
        print(it["name"], "width", width, "worst error / bound", worst)
    for r in ladder:
        r.close()


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------------
def bits(r, keys):
    return [r[k].view(np.uint64).tolist() for k in keys]


@pytest.mark.parametrize("channels", [2, 5])
@pytest.mark.parametrize("width", [32, 64])
def test_on_a_whole_level_the_bits_are_the_unbanded_entries_on_that_rung(width, channels):
    pytest.importorskip("torch")
    T, F, K = 16, 16, 3
    ladder = contexts(width, channels, T, F, LADDERS[K])
    names = {"sine-warp": "random", "short-5": "random", "affine-2.5+0.25": "random", "edges": "random"}
    items = make_items(T, F, channels, K, width, 7, names)
    per_rung = [sampler_run(width, [r] * len(items), items) for r in ladder]
    assert bits(per_rung[0][0], ("y", "gx", "gp")) != bits(per_rung[1][0], ("y", "gx", "gp"))
    keys = ("y", "gx", "gp")
    for L, same in ((0, (0.0, -0.0, -5.0, np.nan, -np.inf)), (1, (1.0,)), (2, (2.0, 2.5, 7.0, np.inf))):
        for level in same:
            got = run(width, [ladder] * len(items), [dict(it, levels=np.full(it["n_out"], level)) for it in items])
            for g, want in zip(got, per_rung[L]):
                assert bits(g, keys) == bits(want, keys), (L, level)
    # mixed whole levels: output m is rung L [m]'s in y and gp
    rng = np.random.default_rng(8)
    mixed = [dict(it, levels=rng.integers(-1, K + 1, it["n_out"]).astype(np.float64)) for it in items]
    got = run(width, [ladder] * len(items), mixed, which=("y", "gp"))
    for i, (it, g) in enumerate(zip(mixed, got)):
        L = np.clip(it["levels"], 0, K - 1).astype(int)
        assert len(set(L.tolist())) == K or it["n_out"] < 20
        for k in range(K):
            assert np.array_equal(g["y"][:, L == k], per_rung[k][i]["y"][:, L == k]) and np.array_equal(g["gp"][L == k], per_rung[k][i]["gp"][L == k])
    # a single rung is the unbanded entry at any level
    anything = [dict(it, levels=level_curve("edges", it["n_out"], 4, rng) + rng.uniform(-1, 1, it["n_out"])) for it in items]
    for k in (0, 2):
        got = run(width, [[ladder[k]]] * len(items), anything)
        for g, want in zip(got, per_rung[k]):
            assert bits(g, keys) == bits(want, keys) and not g["gl"].any()
    for r in ladder:
        r.close()


@pytest.mark.parametrize("width", [32, 64])
def test_bits_do_not_depend_on_batch_place_layout_pitch_stream_or_what_else_is_asked(width):
    torch = pytest.importorskip("torch")
    T, F, K = 16, 16, 3
    items = make_items(T, F, 2, K, width, 90)
    mine = next(it for it in items if it["name"] == "sine-warp")
    mine = dict(mine, levels=level_curve("random", mine["n_out"], K, np.random.default_rng(4)))
    others = [it for it in items if it["name"] in ("short-0", "short-5", "constant", "affine-2.5+0.25", "affine-0.37+0.25")]
    assert len(others) == 5
    ladders = [contexts(width, 2, T, F, LADDERS[K]) for _ in range(3)]
    keys = ("y", "gx", "gp", "gl")
    (alone,) = run(width, ladders[:1], [mine])
    assert all(np.count_nonzero(alone[k]) > alone[k].size // 2 for k in keys)
    first = run(width, [ladders[0]] * 6, [mine] + others)[0]
    last = run(width, [ladders[1]] * 3 + [ladders[0]] * 3, others + [mine])[-1]
    (interleaved,) = run(width, ladders[:1], [mine], planar=False)
    (tight,) = run(width, ladders[:1], [mine], pad=0, base=0)
    (wide,) = run(width, ladders[:1], [mine], pad=29, base=3)
    side = torch.cuda.Stream()
    for r in ladders[2]:
        r.set_stream(side.cuda_stream)
    (streamed,) = run(width, [ladders[2]], [mine], stream=side)
    for other in (first, last, interleaved, tight, wide, streamed):
        assert bits(other, keys) == bits(alone, keys)
    # either gradient alone is the same doubles as both together
    (only_p,) = run(width, ladders[:1], [mine], which=("gp",))
    (only_l,) = run(width, ladders[:1], [mine], which=("gl",))
    assert bits(only_p, ("gp",)) == bits(alone, ("gp",)) and bits(only_l, ("gl",)) == bits(alone, ("gl",))
    # outputs cut short: the curves end there, and what lies behind in p, the levels and gy (NaN here) is not read
    cut = mine["n_out"] - 37
    short = dict(mine, p=mine["p"][:cut], levels=mine["levels"][:cut], gy=mine["gy"][:, :cut], n_out=cut)
    poisoned = dict(mine, p=np.concatenate([mine["p"][:cut], np.full(37, np.nan)]), levels=np.concatenate([mine["levels"][:cut], np.full(37, np.nan)]),
                    n_out=cut, gy=np.concatenate([mine["gy"][:, :cut], np.full((2, 37), np.nan)], 1))
    (want,) = run(width, ladders[:1], [short])
    (got,) = run(width, ladders[:1], [poisoned])
    assert bits(got, keys) == bits(want, keys) and bits(want, keys)[1] != bits(alone, keys)[1]
    for lad in ladders:
        for r in lad:
            r.close()


# ---- 3. refusals on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_refusals_on_the_device_enqueue_and_count_nothing(width):
    torch = pytest.importorskip("torch")
    B, SB = A.binding(width), band.binding(width)
    errors = B.lib().artamdErrorCount()
    T, F = 16, 16
    dt = torch.float64 if width == 64 else torch.float32
    make = lambda channels=1, taps=T, filters=F, cutoff=0.5, flags=FLAGS: B.Resampler(channels, taps, filters, cutoff, flags)
    top, low = make(cutoff=1.0), make()
    stereo, longer, denser, nearest, ends, elsewhere = make(channels=2), make(taps=32), make(filters=32), make(flags=BH | LP), \
        make(flags=FLAGS | A.EXTRAPOLATE_ENDPOINTS), make()
    fixed = B.Resampler(1, T, F, 0.0, FLAGS, (44100.0, 48000.0, 0))
    side = torch.cuda.Stream()
    elsewhere.set_stream(side.cuda_stream)
    x, g = torch.ones(30, dtype=dt, device="cuda"), torch.ones(20, dtype=dt, device="cuda")
    p = torch.arange(20, dtype=torch.float64, device="cuda")
    lv = torch.full((20,), 0.5, dtype=torch.float64, device="cuda")
    y, gx = torch.full((20,), SENTINEL, dtype=dt, device="cuda"), torch.full((30,), SENTINEL, dtype=dt, device="cuda")
    gp, gl = (torch.full((20,), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2))

    def calls(ctxs, K, n_in=30, n_out=20, xs=x, ps=p, ls=lv, gs=g, ys=y, gxs=gx, gps=gp, gls=gl):
        k = len(ctxs) // K if K > 0 else 1
        one = lambda v: None if v is None else [v] * k
        return ((SB.sample_band_clips_planar_device, (ctxs, K, [xs] * k, None, [n_in] * k, [ps] * k, [ls] * k, [n_out] * k, [ys] * k, None)),
                (SB.sample_band_adjoint_clips_planar_device, (ctxs, K, [ps] * k, [ls] * k, [n_out] * k, [gs] * k, None, [gxs] * k, None, [n_in] * k)),
                (SB.sample_band_gradients_clips_planar_device, (ctxs, K, [xs] * k, None, [n_in] * k, [ps] * k, [ls] * k, [n_out] * k, [gs] * k, None,
                                                                one(gps), one(gls))))

    nine = [top] + [low] * 8
    refused = [calls([top, stereo], 2), calls([top, longer], 2), calls([top, denser], 2), calls([top, nearest], 2), calls([nearest, low], 2),
               calls([top, ends], 2), calls([top, elsewhere], 2), calls([top, low, top, elsewhere], 2), calls(nine, 9),
               calls([top, low], 2, n_in=-1), calls([top, low], 2, n_out=-1), calls([top, low], 2, n_in=2 ** 31 - 1 - 2 * T + 1),
               calls([top, low], 2, ps=None), calls([top, low], 2, ls=None)]
    for triple in refused:
        for fn, args in triple:
            with pytest.raises(RuntimeError):
                fn(*args)
    for index, more in ((0, dict(xs=None)), (0, dict(ys=None)), (1, dict(gs=None)), (1, dict(gxs=None)), (2, dict(xs=None)), (2, dict(gs=None)),
                        (2, dict(gps=None, gls=None))):
        fn, args = calls([top, low], 2, **more)[index]
        with pytest.raises(RuntimeError):
            fn(*args)
    # a list that is there, with a NULL entry for a clip that is part of the launch
    fn, args = calls([top, low], 2)[2]
    for at in (10, 11):
        with pytest.raises(RuntimeError):
            fn(*args[:at], [None], *args[at + 1:])
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (y, gx, gp, gl)) and B.lib().artamdErrorCount() == errors
    # taken: rungs that differ in INCLUDE_LOWPASS (1.0 and 0.5), a fixed-ratio context (only its bank is used), one context on every rung,
    # eight rungs, either gradient alone
    for triple in (calls([top, low], 2), calls([fixed, low], 2), calls([low] * 8, 8), calls([top, low, low, low], 2), calls([low], 1)):
        assert [fn(*args) for fn, args in triple] == [1, 1, 1]
    assert calls([top, low], 2, gps=None)[2][0](*calls([top, low], 2, gps=None)[2][1]) == 1
    assert calls([top, low], 2, gls=None)[2][0](*calls([top, low], 2, gls=None)[2][1]) == 1
    # nothing live: no launch, nothing written
    torch.cuda.synchronize()
    for t in (y, gx, gp, gl):
        t.fill_(SENTINEL)
    assert [fn(*args) for fn, args in calls([top, low], 2, n_out=0)] == [0, 0, 0]
    assert calls([top, low], 2, n_in=0)[1][0](*calls([top, low], 2, n_in=0)[1][1]) == 0
    assert calls([top, low], 2, n_in=0, xs=None)[0][0](*calls([top, low], 2, n_in=0, xs=None)[0][1]) == 1      # (no frames: silence, and no buffer is needed)
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (gx, gp, gl)) and bool((y == 0).all()) and B.lib().artamdErrorCount() == errors
    for r in (top, low, stereo, longer, denser, nearest, ends, elsewhere, fixed):
        r.close()


# ---- 4. ClipBandSampler ---------------------------------------------------------------------------------------------------------------------
def band_case(width, seed=5):
    """x [3, 2, 600] with lengths, a curve per clip (sine-warp, affine 2.5, a slow one) and a gradient of y, as numpy in the build's sample type"""
    rng = np.random.default_rng(seed)
    lengths, M = [LONG, 41, 300], 2 * ADJOINT_CHUNK + 150
    xh = (0.25 * rng.standard_normal((3, 2, LONG))).astype(np_of(width))
    m = np.arange(float(M))
    ph = np.stack([0.85 * m + 20.0 * np.sin(2 * np.pi * m / 200.0), 2.5 * m - 8.0, 0.45 * m + 0.125])
    gh = rng.standard_normal((3, 2, M)).astype(np_of(width))
    return lengths, M, xh, ph, gh


def poisoned(xh, lengths):
    out = xh.copy()
    for i, n in enumerate(lengths):
        out[i, :, n:] = np.nan
    return out


def as_got(y=None, gx=None, gp=None, gl=None):
    f = lambda t: t.detach().cpu().numpy().astype(np.float64)
    return {k: f(v) for k, v in (("y", y), ("gx", gx), ("gp", gp), ("gl", gl)) if v is not None}


@pytest.mark.parametrize("width", [32, 64])
def test_clip_band_sampler_at_automatic_levels(width):
    torch = pytest.importorskip("torch")
    SB = band.binding(width)
    T, F, cutoffs = 16, 16, LADDERS[3]
    rungs = BR.ladder(cutoffs, FLAGS)
    lengths, M, xh, ph, gh = band_case(width)
    outs = [M, M - 100, 77]
    clip = SB.ClipBandSampler(2, cutoffs, T, F, guard=0.75)
    x, p = torch.from_numpy(poisoned(xh, lengths)).cuda(), torch.from_numpy(ph).cuda()
    levels = clip.levels_of(p, outs)
    assert levels.is_cuda and levels.shape == (3, M) and levels.dtype == torch.float64 and clip.pool == []
    lh = levels.cpu().numpy()
    for i, n in enumerate(outs):
        want = BR.auto_levels(ph[i], n, cutoffs, 0.75)
        assert np.all(np.abs(lh[i] - want) <= LEVEL_TOLERANCE) and torch.equal(levels[i], clip.levels_of(p[i], outs)[i])
    # (the sine warp crosses a rung; the steep curve sits on the last one; the slow one stays inside the first cell, where the guard puts it)
    assert len(np.unique(np.floor(lh[0]))) >= 2 and np.all(np.abs(lh[1, :outs[1]] - 2.0) <= LEVEL_TOLERANCE) and np.all(lh[1, outs[1]:] == 0.0)
    assert 0.0 < lh[2, :outs[2]].min() and lh[2].max() < 1.0
    y = clip(x, p, lengths=lengths, out_lengths=outs)
    assert y.shape == (3, 2, M) and y.dtype == x.dtype and not y.requires_grad and len(clip.pool) == 3
    assert torch.equal(y, clip(x, p, levels, lengths, outs))
    for i, (n, k) in enumerate(zip(lengths, outs)):
        assert bool((y[i, :, k:] == 0).all())
        # (the levels the call used, held to the restatement above, are the yardstick's: what is judged here is y)
        it = dict(name=f"clip-{i}", x=xh[i].astype(np.float64), n_in=n, p=ph[i], levels=lh[i], n_out=k, gy=gh[i].astype(np.float64))
        _, worst = check(width, T, F, rungs, it, as_got(y=y[i, :, :k]), what=("y",))
        print("ClipBandSampler automatic levels, width", width, "clip", i, "worst error / bound", worst)
    clip.close()


@pytest.mark.parametrize("width", [32, 64])
def test_clip_band_sampler_backward_in_all_three_operands(width, monkeypatch):
    torch = pytest.importorskip("torch")
    SB = band.binding(width)
    T, F, cutoffs, K = 16, 16, LADDERS[3], 3
    rungs = BR.ladder(cutoffs, FLAGS)
    lengths, M, xh, ph, gh = band_case(width)
    outs = [M, M - 100, 77]
    rng = np.random.default_rng(21)
    lh = rng.uniform(-0.25, K - 0.75, (3, M))
    lh[:, ::9] = np.round(lh[:, ::9])                             # (whole levels among them, the ends too)
    sorts = []
    real_sort = torch.sort
    monkeypatch.setattr(torch, "sort", lambda *a, **k: (sorts.append(1), real_sort(*a, **k))[1])      # (counts the calls; torch's own, not the library's)
    clip = SB.ClipBandSampler(2, cutoffs, T, F)
    x = torch.from_numpy(poisoned(xh, lengths)).cuda().requires_grad_()
    p = torch.from_numpy(ph).cuda().requires_grad_()
    lv = torch.from_numpy(lh).cuda().requires_grad_()
    g = torch.from_numpy(gh).cuda()
    g_poisoned = g.clone()
    for i, n in enumerate(outs):
        g_poisoned[i, :, n:] = float("nan")
    with torch.no_grad():
        quiet = clip(x, p, lv, lengths, outs)
    assert quiet.grad_fn is None and not quiet.requires_grad
    y = clip(x, p, lv, lengths, outs)
    assert y.grad_fn is not None and torch.equal(y.detach(), quiet)
    y.backward(g_poisoned)                                        # (grad_y at and past out_lengths is not read)
    assert sorts == [], "a monotone curve was sorted"
    assert x.grad.shape == x.shape and p.grad.shape == p.shape and lv.grad.shape == lv.shape and p.grad.dtype == lv.grad.dtype == torch.float64
    for i, (n, k) in enumerate(zip(lengths, outs)):
        assert bool((x.grad[i, :, n:] == 0).all()) and bool((p.grad[i, k:] == 0).all()) and bool((lv.grad[i, k:] == 0).all())
        it = dict(name=f"clip-{i}", x=xh[i].astype(np.float64), n_in=n, p=ph[i], levels=lh[i], n_out=k, gy=gh[i].astype(np.float64))
        _, worst = check(width, T, F, rungs, it, as_got(y[i, :, :k], x.grad[i, :, :n], p.grad[i, :k], lv.grad[i, :k]))
        print("ClipBandSampler width", width, "clip", i, "worst error / bound", worst)

    # the same outputs in reverse order: backward sorts the curve, and gathers gy and the levels into the same order
    xr = torch.from_numpy(poisoned(xh, lengths)).cuda().requires_grad_()
    pr = torch.from_numpy(np.ascontiguousarray(ph[:, ::-1])).cuda().requires_grad_()
    lr = torch.from_numpy(np.ascontiguousarray(lh[:, ::-1])).cuda().requires_grad_()
    yr = clip(xr, pr, lr, lengths)
    yr.backward(torch.from_numpy(np.ascontiguousarray(gh[:, :, ::-1])).cuda())
    assert len(sorts) == 1, "a decreasing curve was not sorted (or sorted more than once)"
    for i, n in enumerate(lengths):
        it = dict(name=f"reversed-{i}", x=xh[i].astype(np.float64), n_in=n, p=ph[i, ::-1], levels=lh[i, ::-1], n_out=M, gy=gh[i, :, ::-1].astype(np.float64))
        _, worst = check(width, T, F, rungs, it, as_got(yr[i], xr.grad[i, :, :n], pr.grad[i], lr.grad[i]))
        print("ClipBandSampler width", width, "reversed clip", i, "worst error / bound", worst)

    # one curve and one level curve for every clip, the levels in float32: gradients of their own shape and dtype, summed over the clips;
    # x asks for nothing: the gradients call alone
    del sorts[:]
    shared_p = torch.from_numpy(ph[2]).cuda().requires_grad_()
    l32 = lh[0].astype(np.float32)
    shared_l = torch.from_numpy(l32).cuda().requires_grad_()
    x2 = torch.from_numpy(xh).cuda()
    y2 = clip(x2, shared_p, shared_l, lengths)
    y2.backward(g)
    assert shared_p.grad.shape == (M,) and shared_l.grad.shape == (M,) and shared_l.grad.dtype == torch.float32 and x2.grad is None and sorts == []
    want = {k: np.zeros(M) for k in ("gp", "gl", "gp_slack", "gl_slack", "gl_size")}
    for i, n in enumerate(lengths):
        ref = BR.sample(T, F, rungs, xh[i, :, :n].astype(np.float64), ph[2], l32.astype(np.float64), gh[i].astype(np.float64), width)
        err = np.abs(y2[i].detach().cpu().numpy().astype(np.float64) - ref.ys)
        assert np.all(err <= ((T + 12) * 2.0 ** -53 * ref.scale if width == 64 else 2.0 ** -24 * np.abs(ref.ys) + (T + 7) * 2.0 ** -52 * ref.scale))
        want["gp"] += ref.gp; want["gl"] += ref.gl; want["gl_size"] += np.abs(ref.gl)
        want["gp_slack"] += (2 * T + 2 + 5) * 2.0 ** -52 * ref.gp_scale
        want["gl_slack"] += (4 * (T + 4) + 2 + 2) * 2.0 ** -52 * ref.gl_scale
    # (autograd adds the three clips' rows in float64 — two sums, 2^-53 of a partial sum each — and narrows the levels' to float32)
    size_p = np.abs(shared_p.grad.cpu().numpy())
    assert np.all(np.abs(shared_p.grad.cpu().numpy() - want["gp"]) <= want["gp_slack"] + 3 * 2.0 ** -53 * (size_p + np.abs(want["gp"])))
    assert np.all(np.abs(shared_l.grad.cpu().numpy().astype(np.float64) - want["gl"]) <= want["gl_slack"] + 2.0 ** -23 * want["gl_size"])
    # levels alone; positions alone
    l3 = torch.from_numpy(lh).cuda().requires_grad_()
    clip(x2, torch.from_numpy(ph).cuda(), l3, lengths).backward(g)
    p3 = torch.from_numpy(ph).cuda().requires_grad_()
    clip(x2, p3, torch.from_numpy(lh).cuda(), lengths).backward(g)
    x4, p4, l4 = torch.from_numpy(xh).cuda().requires_grad_(), torch.from_numpy(ph).cuda().requires_grad_(), torch.from_numpy(lh).cuda().requires_grad_()
    clip(x4, p4, l4, lengths).backward(g)
    assert torch.equal(l3.grad, l4.grad) and torch.equal(p3.grad, p4.grad) and bool((l4.grad != 0).any()) and sorts == []
    # automatic levels carry no gradient; [C, T] in; no clip at all
    p5 = torch.from_numpy(ph[0]).cuda().requires_grad_()
    y5 = clip(torch.from_numpy(xh[0]).cuda(), p5)
    assert y5.shape == (1, 2, M)
    y5.backward(g[:1])
    assert p5.grad.shape == (M,) and bool((p5.grad != 0).any())
    empty = SB.ClipBandSampler(2, cutoffs, T, F)
    x0 = torch.zeros(0, 2, 10, dtype=x.dtype, device="cuda", requires_grad=True)
    p0, l0 = (torch.zeros(7, dtype=torch.float64, device="cuda", requires_grad=True) for _ in range(2))
    y0 = empty(x0, p0, l0)
    y0.sum().backward()
    assert y0.shape == (0, 2, 7) and x0.grad.shape == (0, 2, 10) and p0.grad.shape == (7,) and l0.grad.shape == (7,) and not bool(l0.grad.any()) and empty.pool == []
    with pytest.raises(RuntimeError):                             # (once differentiable)
        y6 = clip(x4, p4, l4, lengths)
        (g6,) = torch.autograd.grad((y6 * g).sum(), l4, create_graph=True)
        g6.sum().backward()
    # backward after close () raises
    y7 = clip(x4, p4, l4, lengths)
    clip.close()
    with pytest.raises(RuntimeError):
        y7.sum().backward()


def test_the_level_gradient_is_the_difference_quotient_on_the_8_byte_build():
    torch = pytest.importorskip("torch")
    SB = band.binding(64)
    T, F, cutoffs, K, h = 16, 16, LADDERS[3], 3, 2.0 ** -10
    rungs = BR.ladder(cutoffs, FLAGS)
    rng = np.random.default_rng(33)
    N, M = 80, 60
    xh = 0.25 * rng.standard_normal((1, 2, N))
    ph = np.sort(rng.uniform(-4.0, N + 4.0, (1, M)), axis=1)
    lh = rng.integers(0, K - 1, (1, M)) + rng.uniform(0.1, 0.9, (1, M))     # inside the cells: y is linear in the level from l - h to l + h
    gh = rng.standard_normal((1, 2, M))
    clip = SB.ClipBandSampler(2, cutoffs, T, F)
    x, p, g = torch.from_numpy(xh).cuda(), torch.from_numpy(ph).cuda(), torch.from_numpy(gh).cuda()
    lv = torch.from_numpy(lh).cuda().requires_grad_()
    clip(x, p, lv).backward(g)
    up, down = clip(x, p, torch.from_numpy(lh + h).cuda()), clip(x, p, torch.from_numpy(lh - h).cuda())
    quotient = ((g * (up - down)).sum(1) / (2 * h))[0].cpu().numpy()
    ref = BR.sample(T, F, rungs, xh[0], ph[0], lh[0], gh[0], 64)
    assert np.array_equal(np.floor(lh + h), np.floor(lh - h)) and ref.moves.sum() > M // 2
    # each of the two results comes from the same two rung values (their chains do not see the level) by 1.0 - lam, the two products, their
    # sum and the result's rounding: at most six roundings of 2^-53 of at most scale_j + scale_{j+1}, over 2h; l + h and l - h are rounded
    # themselves, 2^-52 of a level below 2 each: 2^-42 of the slope relative to 2h = 2^-9; all times |gy|, summed over the channels; and
    # the level gradient's own bound
    tol = (2 * 6 * 2.0 ** -53 / (2 * h) + 2.0 ** -42 + (2 * 2 * (T + 4) + 2 + 2) * 2.0 ** -52) * ref.gl_scale
    err = np.abs(quotient - lv.grad[0].cpu().numpy())
    print("level gradient against the difference quotient: worst error / tolerance", float((err / np.maximum(tol, 1e-300)).max()))
    assert np.all(err <= tol) and np.all(np.abs(lv.grad[0].cpu().numpy() - ref.gl) <= (2 * 2 * (T + 4) + 2 + 2) * 2.0 ** -52 * ref.gl_scale)
    assert np.count_nonzero(lv.grad[0].cpu().numpy()) == ref.moves.sum()
    clip.close()


@pytest.mark.parametrize("width", [32, 64])
def test_the_automatic_level_removes_what_would_alias_on_the_device(width):
    torch = pytest.importorskip("torch")
    SB = band.binding(width)
    T = F = 64
    N, M = 600, 300
    dt = torch.float64 if width == 64 else torch.float32
    clip = SB.ClipBandSampler(1, taps=T, filters=F)
    assert clip.cutoffs == DEFAULT
    p = 2.0 * torch.arange(M, dtype=torch.float64, device="cuda")
    assert bool((clip.levels_of(p) == 2.0).all())
    n = np.arange(N)
    rms = lambda t: float(np.sqrt(np.mean(t[0, 0, T:M - T].cpu().numpy().astype(np.float64) ** 2)))
    for tone, kept in ((0.75, False), (0.3, True)):
        x = torch.from_numpy(0.5 * np.cos(np.pi * tone * n)[None, None, :]).to(dt).cuda()
        full, banded = rms(clip(x, p, torch.zeros(M, dtype=torch.float64, device="cuda"))), rms(clip(x, p))
        print("width", width, "tone", tone, "full band rms", full, "automatic levels rms", banded, "ratio", banded / full)
        assert abs(full - 0.5 / np.sqrt(2)) < 1e-3
        assert abs(banded / full - 1.0) <= 1e-3 if kept else banded <= 1e-3 * full
    clip.close()
