"""The cases of tests/golden/clip_curve_parent_bits.npz — the six curve-sampling entries' results (sampler: forward, adjoint, position
gradient; band: forward, adjoint, gradients) at the commit the file names, kept so that the merge of the two kernel families into one
body per pass, and whatever tunes that body later, has bits to reproduce — shared by the generator
(tests/golden/make_golden_clip_curve.py) and the test that holds both sample widths to those bits (tests/test_gpu_clip_curve_bits.py).
Everything is synthetic and regenerated from a seed; of the library only the six public wrappers are called.  TEST INFRASTRUCTURE ONLY."""
import zlib

import numpy as np

import audio_resampler_amd as A

BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
TAPS = FILTERS = 16
HALF = TAPS // 2
SEED = 41
SENTINEL = -777.25
WIDTHS = (32, 64)

# name: (rungs (0: the unbanded entries), context flags, channels, planar (with a padded pitch) or interleaved, gradients asked for,
#        clips: (frames, outputs, curve, levels)).
# Frames 0, 5 and 300 / 601 (one and two tile boundaries of 256 input frames); more than 256 outputs on every long clip ("dense": more than
# 256 of them inside the first input tile's range, so the adjoint takes a second trip through its chunk); channels 1, 2 and 5 (adjoint
# groups of 1, 2 and 4, and a tail past the four channels in flight); "whole": positions on and within 1 / 64 of whole frames, which a
# nearest-filter context without the low-pass flag passes through.  Every curve is non-decreasing (the adjoint's precondition) and
# carries the special positions of `curve` below.  Ladders of 1, 3 and 8 rungs; gp alone, gl alone and both.
CASES = {
    "interp-2ch-planar-batch": (0, BH | IN | LP, 2, True, "p", ((601, 300, "ramp", None), (0, 40, "ramp", None), (5, 40, "ramp", None), (5, 0, "ramp", None), (5, 33, "ramp", None))),
    "interp-5ch-interleaved-dense": (0, BH | IN | LP, 5, False, "p", ((601, 420, "dense", None), (5, 40, "ramp", None))),
    "interp-1ch": (0, BH | IN | LP, 1, True, "p", ((300, 280, "ramp", None), (5, 20, "ramp", None))),
    "nearest-2ch-interleaved": (0, BH | LP, 2, False, "", ((300, 280, "ramp", None), (5, 20, "ramp", None), (0, 20, "ramp", None))),
    "nearest-5ch-planar-dense": (0, BH | LP, 5, True, "", ((300, 300, "dense", None), (5, 20, "ramp", None))),
    "nearest-1ch": (0, BH | LP, 1, False, "", ((300, 280, "ramp", None),)),
    "pass-through-2ch-planar": (0, BH, 2, True, "", ((300, 280, "whole", None), (5, 30, "whole", None))),
    "band3-2ch-planar-batch": (3, BH | IN | LP, 2, True, "pl", ((601, 300, "ramp", "mixed"), (0, 40, "ramp", "mixed"), (5, 40, "ramp", "mixed"), (5, 0, "ramp", "mixed"), (5, 33, "ramp", "whole"))),
    "band8-5ch-interleaved-dense": (8, BH | IN | LP, 5, False, "l", ((601, 420, "dense", "mixed"), (5, 40, "ramp", "fractional"))),
    "band1-1ch": (1, BH | IN | LP, 1, True, "pl", ((300, 280, "ramp", "mixed"), (5, 20, "ramp", "mixed"))),
    "band3-2ch-interleaved-p-alone": (3, BH | IN | LP, 2, False, "p", ((300, 280, "ramp", "mixed"), (5, 30, "ramp", "whole"), (5, 30, "ramp", "fractional"))),
    "band8-1ch-whole-levels": (8, BH | IN | LP, 1, False, "pl", ((300, 280, "dense", "whole"),)),
}


def curve(rng, frames, outputs, kind):
    """`outputs` non-decreasing positions over a clip of `frames` frames: both ends of the window range and beyond them, infinities, a tiny
    negative p for which p - floor(p) rounds to 1, whole frames, filter boundaries, repeated positions; NaNs last (they sort as +infinity)"""
    lo, hi = -(HALF + 1.0), frames + float(HALF)
    special = [-np.inf, -1e30, lo - 0.5, lo, lo + 0.25, -1e-17, 0.0, 2.0, 2.0 + 5 / 16, 2.0 + 5 / 16, hi - 0.25, hi, hi + 7.5, 1e30, np.inf]
    nans = [np.nan, np.nan]
    n = outputs - len(special) - len(nans)
    if n < 0:
        return np.array((special + nans)[len(special) + len(nans) - outputs:] if outputs else [], np.float64)
    if kind == "dense":
        body = np.concatenate([rng.uniform(60.0, 110.0, n - n // 5), rng.uniform(lo, hi, n // 5)])
    elif kind == "whole":
        body = np.floor(rng.uniform(lo, hi, n)) + rng.choice([0.0, 0.0, 1 / 64, -1 / 64, 0.375], n)
    else:
        body = rng.uniform(lo, hi, n)
    return np.concatenate([np.sort(np.concatenate([body, special])), nans])


def levels(rng, rungs, outputs, kind):
    """a level per output on a ladder of `rungs` rungs, in runs of 1 to 9 outputs of one sort (the adjoint takes its outputs four at a time,
    and a group on whole levels loads what the unbanded walk loads): whole; fractional; -0.0; negative; NaN; at and past the last rung"""
    top = float(rungs - 1)
    sorts = {"whole": lambda: float(rng.integers(0, rungs)), "fractional": lambda: rng.uniform(0.0, max(top, 0.75)),
             "zero": lambda: -0.0, "negative": lambda: -rng.uniform(0.0, 3.0), "nan": lambda: np.nan, "top": lambda: top,
             "past": lambda: top + rng.choice([0.5, 1e9, np.inf]), "below": lambda: -np.inf, "tiny": lambda: 1e-300,
             "under-top": lambda: np.nextafter(top, -1.0) if top else 0.0}
    names = sorted(sorts) + ["fractional"] * 4 + ["whole"] * 3 if kind == "mixed" else [kind]     # (half of a mixed curve lies inside the ladder)
    out = []
    while len(out) < outputs:
        draw = sorts[names[rng.integers(0, len(names))]]
        run = int(rng.integers(1, 10))
        out += [draw() for _ in range(run)] if rng.integers(0, 2) else [draw()] * run
    return np.array(out[:outputs], np.float64)


def inputs(name, width):
    """per clip (x [C, N], gy [C, M], positions [M], levels [M] or None), host arrays in the build's sample type; the same values in both widths"""
    rungs, _, channels, _, _, clips = CASES[name]
    rng = np.random.default_rng([SEED, zlib.crc32(name.encode())])
    smp = np.float64 if width == 64 else np.float32
    made = []
    for frames, outputs, kind, level_kind in clips:
        x = (0.25 * rng.standard_normal((channels, frames))).astype(np.float32).astype(smp)
        gy = (0.25 * rng.standard_normal((channels, outputs))).astype(np.float32).astype(smp)
        made.append((x, gy, curve(rng, frames, outputs, kind), levels(rng, rungs, outputs, level_kind) if rungs else None))
    return made


def keys(name):
    """the arrays stored for a case (without the width): per clip y, gx, and gp / gl where the case asks for them"""
    rungs, _, _, _, want, clips = CASES[name]
    return [f"{i}/{k}" for i in range(len(clips)) for k in ["y", "gx"] + (["gp"] if "p" in want else []) + (["gl"] if "l" in want and rungs else [])]


def run(name, width):
    """the case's clips through the family's three entries, one call each -> {key: array}.  Every result buffer starts at SENTINEL and is
    returned whole, its padding included: what an entry leaves alone is part of the record."""
    import torch
    from audio_resampler_amd import band, sampler
    rungs, flags, channels, planar, want, clips = CASES[name]
    B, S, L = A.binding(width), sampler.binding(width), band.binding(width)
    ladder = [B.Resampler(channels, TAPS, FILTERS, 0.9 * 0.8 ** k, flags) for k in range(max(rungs, 1))]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def lay(a, pad):
        """[C, n] on the host -> the device tensor of the case's layout (planar: pad more frames per row; interleaved: one more frame), its pitch"""
        c, n = a.shape
        full = np.full((c, n + pad) if planar else (n + 1, c), SENTINEL, a.dtype)
        if planar:
            full[:, :n] = a
        else:
            full[:n] = a.T
        return dev(full), (n + pad if planar else 0)

    made = inputs(name, width)
    k = len(clips)
    ctxs = ladder * k
    xs, gys, ys, gxs = ([lay(a, pad) for a in arrays] for arrays, pad in (
        ([m[0] for m in made], 3), ([m[1] for m in made], 5),
        ([np.full_like(m[1], SENTINEL) for m in made], 7), ([np.full_like(m[0], SENTINEL) for m in made], 2)))
    ps = [dev(m[2]) if len(m[2]) else torch.zeros(1, dtype=torch.float64, device="cuda") for m in made]
    lvs = [dev(m[3]) if rungs and len(m[3]) else torch.zeros(1, dtype=torch.float64, device="cuda") for m in made]
    gps, gls = ([torch.full((max(len(m[2]), 1),), SENTINEL, dtype=torch.float64, device="cuda") for m in made] for _ in range(2))
    n_in, n_out = [c[0] for c in clips], [c[1] for c in clips]
    t, pitch = (lambda pairs: [p[0] for p in pairs]), (lambda pairs: [p[1] for p in pairs])

    launches = []
    if rungs:
        launches.append(L.sample_band_clips_planar_device(ctxs, rungs, t(xs), pitch(xs), n_in, ps, lvs, n_out, t(ys), pitch(ys)))
        launches.append(L.sample_band_adjoint_clips_planar_device(ctxs, rungs, ps, lvs, n_out, t(gys), pitch(gys), t(gxs), pitch(gxs), n_in))
        launches.append(L.sample_band_gradients_clips_planar_device(ctxs, rungs, t(xs), pitch(xs), n_in, ps, lvs, n_out, t(gys), pitch(gys),
                                                                    gps if "p" in want else None, gls if "l" in want else None))
    else:
        launches.append(S.sample_clips_planar_device(ctxs, t(xs), pitch(xs), n_in, ps, n_out, t(ys), pitch(ys)))
        launches.append(S.sample_adjoint_clips_planar_device(ctxs, ps, n_out, t(gys), pitch(gys), t(gxs), pitch(gxs), n_in))
        if "p" in want:
            launches.append(S.sample_position_gradient_clips_planar_device(ctxs, t(xs), pitch(xs), n_in, ps, n_out, t(gys), pitch(gys), gps))
    torch.cuda.synchronize()
    assert launches == [1] * len(launches), (name, launches)
    got = {}
    for i in range(k):
        got[f"{i}/y"], got[f"{i}/gx"] = ys[i][0].cpu().numpy(), gxs[i][0].cpu().numpy()
        if "p" in want:
            got[f"{i}/gp"] = gps[i].cpu().numpy()
        if "l" in want and rungs:
            got[f"{i}/gl"] = gls[i].cpu().numpy()
    for r in ladder:
        r.close()
    assert sorted(got) == sorted(keys(name))
    return got
