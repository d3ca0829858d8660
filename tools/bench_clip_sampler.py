"""The clip sampler next to the planned clip entries on the same clips, everything in turn in one run:

  sample          resampleSampleClipsPlanarDevice at p[m] = m / ratio - taps / 2 (the clip entries' own outputs)
  sample_adjoint  resampleSampleAdjointClipsPlanarDevice (the gradient of the samples)
  sample_slope    resampleSamplePositionGradientClipsPlanarDevice (the gradient of the positions)
  warp            resampleProcessScheduleClipsPlanarDevice from a fresh start, blocks of 1,024 frames at the one ratio (ClipWarper's forward)
  warp_adjoint    resampleAdjointScheduleClipsPlanarDevice (ClipWarper's backward)
  rate_grad       resampleRateGradientScheduleClipsPlanarDevice (ClipRateWarper's ratio gradient: two launches)

The shapes: B = 64 clips of 160,000 frames, one and two channels, ratios 48000/44100 and 0.5, 380 taps and filters.

    python tools/bench_clip_sampler.py [--calls 15] [--out FILE]

The lines it prints (and writes to FILE) are kept in profiles/clip_sampler.txt beside what was read from them.

Per case: median wall-clock milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th percentile (the
spread); and `device_ms`, the call's time on the device alone (events around a call enqueued behind other work).
"""
import argparse
import json

from bench_clip_warp import device_ms, timed
import torch
import audio_resampler_amd as A
from audio_resampler_amd import rate_grad, sampler

B, FRAMES, TAPS, BLOCK = 64, 160000, 380, 1024
RATIOS = (48000 / 44100, 0.5)


def case(channels, ratio, calls):
    flags = A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.INCLUDE_LOWPASS
    pool = [A.Resampler(channels, TAPS, TAPS, 0.0, flags) for _ in range(B)]
    frames = [min(BLOCK, FRAMES - k) for k in range(0, FRAMES, BLOCK)]
    rates = [ratio] * len(frames)
    caps = [int((n + 2) * ratio) + 4 for n in frames]
    caps[-1] = int((frames[-1] + TAPS // 2 + 2) * ratio) + 4
    room = sum(caps)
    x = torch.randn(B, channels, FRAMES, device="cuda") * 0.25
    y = torch.zeros(B, channels, room, device="cuda")
    gy = torch.randn(B, channels, room, device="cuda") * 0.25
    gx = torch.zeros(B, channels, FRAMES, device="cuda")
    gr = torch.zeros(B, len(frames), dtype=torch.float64, device="cuda")
    rows = lambda t: [t[i].data_ptr() for i in range(B)]
    pitch = lambda t: [t.stride(1) if channels > 1 else 0] * B
    state = {}

    def warp():
        state["warp"] = A.process_schedule_clips_planar_device(pool, rows(x), pitch(x), [frames] * B, rows(y), pitch(y), [caps] * B, [rates] * B,
                                                               flush_last=[True] * B, from_start=True)

    warp()
    torch.cuda.synchronize()
    launches, got = state["warp"]
    made = [sum(g for _, g in res) for _, res in got]
    M = made[0]
    assert all(m == M for m in made)
    lead = [pool[0]] * B

    def warp_adjoint():
        state["warp_adjoint"] = A.adjoint_schedule_clips_planar_device(lead, rows(gy), pitch(gy), made, rows(gx), pitch(gx), [frames] * B, [rates] * B)

    def grad():
        state["rate_grad"] = rate_grad.rate_gradient_schedule_clips_planar_device(lead, rows(x), pitch(x), rows(gy), pitch(gy), made, [frames] * B, [rates] * B,
                                                                                  rows(gr))

    # the sampler on the same outputs: one curve on the device, listed for every clip
    p = torch.arange(M, dtype=torch.float64, device="cuda") / ratio - TAPS // 2
    ys = torch.zeros(B, channels, M, device="cuda")
    gp = torch.zeros(B, M, dtype=torch.float64, device="cuda")
    curve, lengths, outs = [p.data_ptr()] * B, [FRAMES] * B, [M] * B

    def sample():
        state["sample"] = sampler.sample_clips_planar_device(lead, rows(x), pitch(x), lengths, curve, outs, rows(ys), pitch(ys))

    def sample_adjoint():
        state["sample_adjoint"] = sampler.sample_adjoint_clips_planar_device(lead, curve, outs, rows(gy), pitch(gy), rows(gx), pitch(gx), lengths)

    def sample_slope():
        state["sample_slope"] = sampler.sample_position_gradient_clips_planar_device(lead, rows(x), pitch(x), lengths, curve, outs, rows(gy), pitch(gy), rows(gp))

    sample()
    torch.cuda.synchronize()
    # (the same outputs up to the sum's order: the planned positions are these up to a rounding of the ring's offsets)
    assert float((ys - y[:, :, :M]).abs().max()) < 1e-3, "the sampler's clips are not the warper's"
    fns = dict(sample=sample, sample_adjoint=sample_adjoint, sample_slope=sample_slope, warp=warp, warp_adjoint=warp_adjoint, rate_grad=grad)
    res = dict(B=B, channels=channels, ratio=round(ratio, 6), frames=FRAMES, outputs=M)
    for name, fn in fns.items():
        res[name] = timed(fn, calls, 3)
    state["warp"] = state["warp"][0]
    res["launches"] = {k: state[k] for k in fns}
    res["device_ms"] = {k: device_ms(fn) for k, fn in fns.items()}
    for ours, theirs in (("sample", "warp"), ("sample_adjoint", "warp_adjoint"), ("sample_slope", "rate_grad")):
        res[ours + "_over_" + theirs] = round(res[ours][0] / res[theirs][0], 2)
        res[ours + "_over_" + theirs + "_device"] = round(res["device_ms"][ours] / res["device_ms"][theirs], 2)
    for r in pool:
        r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# [median, 25th, 75th percentile] ms per call, host side included; 64 clips of 160,000 frames, 380 taps, the warper's blocks 1,024 frames",
             "# device: " + torch.cuda.get_device_name(0)]
    for channels in (1, 2):
        for ratio in RATIOS:
            lines.append(json.dumps(case(channels, ratio, a.calls)))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
