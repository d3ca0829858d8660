"""The band-limited clip sampler next to the plain one on the same clips, everything in turn in one run:

  (a) sample, sample_adjoint, sample_slope     the unbanded entries on the ladder's rung 0 (tools/bench_clip_sampler.py's calls)
  (b) band0, band0_adjoint, band0_gradients    the banded entries at level 0 everywhere: the same rows of the same bank
  (c) band15, band15_adjoint, band15_gradients at a constant level of 1.5: two rungs per output
  (d) warp, warp_adjoint, warp_gradients       at ClipBandSampler's automatic levels on a sine-warp curve (steps 0.92 +- 0.6: levels from 0
                                               to about 1.2, neighbouring lanes on neighbouring blends), and beside it
      plain_warp, plain_warp_adjoint, plain_warp_slope   the unbanded entries on that curve
  The gradients calls ask for positions and levels together; band0_slope asks for the positions alone.

The shapes: tools/bench_clip_sampler.py's clips — B = 64 clips of 160,000 frames at 48000/44100, one and two channels, 380 taps and
filters — on the default ladder, K = 5.

    python tools/bench_clip_band.py [--calls 15] [--out FILE]

The lines it prints (and writes to FILE) are kept in profiles/clip_band.txt beside what was read from them.  Per case: median wall-clock
milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th percentile (the spread); and `device_ms`, the
call's time on the device alone (events around a call enqueued behind other work).
"""
import argparse
import json
import math

from bench_clip_warp import device_ms, timed
import torch
import audio_resampler_amd as A
from audio_resampler_amd import band, sampler

B, FRAMES, TAPS = 64, 160000, 380
RATIO = 48000 / 44100
CUTOFFS = (1.0, 2 ** -0.5, 0.5, 2 ** -1.5, 0.25)


def case(channels, calls):
    flags = A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.INCLUDE_LOWPASS
    ladder = [A.Resampler(channels, TAPS, TAPS, c, flags) for c in CUTOFFS]
    K = len(ladder)
    M = int(FRAMES * RATIO)
    x = torch.randn(B, channels, FRAMES, device="cuda") * 0.25
    gy = torch.randn(B, channels, M, device="cuda") * 0.25
    y = torch.zeros(B, channels, M, device="cuda")
    gx = torch.zeros(B, channels, FRAMES, device="cuda")
    gp, gl = (torch.zeros(B, M, dtype=torch.float64, device="cuda") for _ in range(2))
    rows = lambda t: [t[i].data_ptr() for i in range(B)]
    pitch = lambda t: [t.stride(1) if channels > 1 else 0] * B
    m = torch.arange(M, dtype=torch.float64, device="cuda")
    straight = m / RATIO - TAPS // 2
    period = 48000.0
    warped = straight + 0.6 * period / (2 * math.pi) * torch.sin(2 * math.pi * m / period)
    auto = band.ClipBandSampler(channels, CUTOFFS, TAPS, TAPS).levels_of(warped)[0].contiguous()
    levels = {"band0": torch.zeros(M, dtype=torch.float64, device="cuda"), "band15": torch.full((M,), 1.5, dtype=torch.float64, device="cuda"), "warp": auto}
    lead, rungs = [ladder[0]] * B, ladder * B
    lengths, outs = [FRAMES] * B, [M] * B
    state, fns = {}, {}

    def plain(name, p):
        curve = [p.data_ptr()] * B

        def forward():
            state[name] = sampler.sample_clips_planar_device(lead, rows(x), pitch(x), lengths, curve, outs, rows(y), pitch(y))

        def adjoint():
            state[name + "_adjoint"] = sampler.sample_adjoint_clips_planar_device(lead, curve, outs, rows(gy), pitch(gy), rows(gx), pitch(gx), lengths)

        def slope():
            state[name + "_slope"] = sampler.sample_position_gradient_clips_planar_device(lead, rows(x), pitch(x), lengths, curve, outs, rows(gy), pitch(gy),
                                                                                          rows(gp))

        fns.update({name: forward, name + "_adjoint": adjoint, name + "_slope": slope})

    def banded(name, p, lv):
        curve, lvs = [p.data_ptr()] * B, [lv.data_ptr()] * B

        def forward():
            state[name] = band.sample_band_clips_planar_device(rungs, K, rows(x), pitch(x), lengths, curve, lvs, outs, rows(y), pitch(y))

        def adjoint():
            state[name + "_adjoint"] = band.sample_band_adjoint_clips_planar_device(rungs, K, curve, lvs, outs, rows(gy), pitch(gy), rows(gx), pitch(gx),
                                                                                    lengths)

        def gradients():
            state[name + "_gradients"] = band.sample_band_gradients_clips_planar_device(rungs, K, rows(x), pitch(x), lengths, curve, lvs, outs, rows(gy),
                                                                                        pitch(gy), rows(gp), rows(gl))

        fns.update({name: forward, name + "_adjoint": adjoint, name + "_gradients": gradients})

    plain("sample", straight)
    banded("band0", straight, levels["band0"])

    def band0_slope():
        state["band0_slope"] = band.sample_band_gradients_clips_planar_device(rungs, K, rows(x), pitch(x), lengths, [straight.data_ptr()] * B,
                                                                              [levels["band0"].data_ptr()] * B, outs, rows(gy), pitch(gy), rows(gp), None)

    fns["band0_slope"] = band0_slope
    banded("band15", straight, levels["band15"])
    banded("warp", warped, levels["warp"])
    plain("plain_warp", warped)

    # at level 0 the banded forward is the unbanded one bit for bit
    fns["sample"]()
    want = y.clone()
    fns["band0"]()
    torch.cuda.synchronize()
    assert torch.equal(y, want), "the banded forward at level 0 is not the sampler's"
    res = dict(B=B, channels=channels, ratio=round(RATIO, 6), frames=FRAMES, outputs=M, rungs=K,
               auto_levels=[round(float(auto.min()), 3), round(float(auto.mean()), 3), round(float(auto.max()), 3)])
    for name, fn in fns.items():
        res[name] = timed(fn, calls, 3)
    res["launches"] = {k: state[k] for k in fns}
    res["device_ms"] = {k: device_ms(fn) for k, fn in fns.items()}
    for ours, theirs in (("band0", "sample"), ("band0_adjoint", "sample_adjoint"), ("band0_slope", "sample_slope"), ("band0_gradients", "sample_slope"),
                         ("band15", "sample"), ("band15_adjoint", "sample_adjoint"), ("band15_gradients", "sample_slope"),
                         ("warp", "plain_warp"), ("warp_adjoint", "plain_warp_adjoint"), ("warp_gradients", "plain_warp_slope")):
        res[ours + "_over_" + theirs + "_device"] = round(res["device_ms"][ours] / res["device_ms"][theirs], 2)
    for r in ladder:
        r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# [median, 25th, 75th percentile] ms per call, host side included; 64 clips of 160,000 frames at 48000/44100, 380 taps, a ladder of 5 rungs",
             "# device: " + torch.cuda.get_device_name(0)]
    for channels in (1, 2):
        lines.append(json.dumps(case(channels, a.calls)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
