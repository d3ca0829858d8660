"""The ratio gradient of variable-rate clips next to the forward and the sample gradient of the same batch, everything in turn in one run:

  forward      resampleProcessScheduleClipsPlanarDevice from a fresh start
  adjoint      resampleAdjointScheduleClipsPlanarDevice (the gradient of the samples)
  rate_grad    resampleRateGradientScheduleClipsPlanarDevice (the gradient of the blocks' ratios: two launches)
  and the same clips cut into tiny blocks (--tiny frames each: 1,000 blocks of 16), batches up to 64
  forward_tiny, adjoint_tiny, rate_grad_tiny

The shapes are tools/bench_clip_warp.py's: B stereo clips of 16,000 frames, 380 taps, blocks of 1,024 frames, ratios a slow walk inside
0.9 .. 1.1.

    python tools/bench_clip_rate_grad.py [--calls 15] [--batches 1,64,1024] [--tiny 16] [--out FILE]

The lines it prints (and writes to FILE) are kept in profiles/clip_rate_grad.txt beside what was read from them.

Per case: median wall-clock milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th percentile; and
`device_ms`, the call's time on the device alone (events around a call enqueued behind other work).
"""
import argparse
import json

from bench_clip_warp import BATCHES, BLOCK, CH, FRAMES, TAPS, cut, device_ms, timed, walk
import numpy as np
import torch
import audio_resampler_amd as A
from audio_resampler_amd import rate_grad


def schedule(pool, x, y, frames, ratios):
    """(the forward's argument tuple, its caps) for every clip cut into `frames` at `ratios`"""
    B = len(pool)
    caps = [[int((n + 2) * r) + 4 for n, r in zip(frames, row)] for row in ratios]
    for c, row in zip(caps, ratios):
        c[-1] = int((frames[-1] + TAPS // 2 + 2) * row[-1]) + 4
    assert max(sum(c) for c in caps) <= y.shape[2]
    return (pool, [x[i].data_ptr() for i in range(B)], [x.stride(1)] * B, [frames] * B, [y[i].data_ptr() for i in range(B)], [y.stride(1)] * B, caps, ratios)


def trio(pool, x, y, gy, gx, gr, frames, ratios, calls, warm, suffix=""):
    """the three calls on one cut of the clips -> their timings, launches and device times under names ending in `suffix`"""
    B, K = len(pool), len(frames)
    args = schedule(pool, x, y, frames, ratios)
    state = {}

    def forward():
        state["fwd"] = A.process_schedule_clips_planar_device(*args, flush_last=[True] * B, from_start=True)

    forward()
    torch.cuda.synchronize()
    launches, got = state["fwd"]
    assert all(made == K and all(used == n for (used, _), n in zip(res, frames)) for made, res in got)
    made = [sum(g for _, g in res) for _, res in got]
    ins, gouts, gins = [x[i].data_ptr() for i in range(B)], [gy[i].data_ptr() for i in range(B)], [gx[i].data_ptr() for i in range(B)]
    grads = [gr[i].data_ptr() for i in range(B)]

    def adjoint():
        state["adj"] = A.adjoint_schedule_clips_planar_device([pool[0]] * B, gouts, [gy.stride(1)] * B, made, gins, [gx.stride(1)] * B, [frames] * B, ratios)

    def grad():
        state["rate"] = rate_grad.rate_gradient_schedule_clips_planar_device([pool[0]] * B, ins, [x.stride(1)] * B, gouts, [gy.stride(1)] * B, made,
                                                                             [frames] * B, ratios, grads)

    gr.fill_(float("nan"))
    grad()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(gr[:, :K]).all()) and bool((gr[:, :K] != 0).any()), "the ratio gradient was not set"
    out = {"blocks" + suffix: K, "outputs" + suffix: int(sum(made))}
    for name, fn in (("forward", forward), ("adjoint", adjoint), ("rate_grad", grad)):
        out[name + suffix] = timed(fn, calls, warm)
    out["launches" + suffix] = dict(forward=launches, adjoint=state["adj"], rate_grad=state["rate"])
    out["device_ms" + suffix] = dict(forward=device_ms(forward), adjoint=device_ms(adjoint), rate_grad=device_ms(grad))
    for name in ("rate_grad", "adjoint"):
        out[name + "_over_forward" + suffix] = round(out[name + suffix][0] / out["forward" + suffix][0], 2)
        out[name + "_over_forward_device" + suffix] = round(out["device_ms" + suffix][name] / out["device_ms" + suffix]["forward"], 2)
    return out


def case(B, calls, tiny):
    flags = A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.INCLUDE_LOWPASS
    pool = [A.Resampler(CH, TAPS, TAPS, 0.0, flags) for _ in range(B)]
    rng = np.random.default_rng(7)
    frames, small = cut(BLOCK), cut(tiny)
    K = len(frames)
    ratios = [walk(rng, K) for _ in range(B)]
    room = int((FRAMES + TAPS) * 1.1) + 8 * len(small)
    x = torch.randn(B, CH, FRAMES, device="cuda") * 0.25
    y = torch.zeros(B, CH, room, device="cuda")
    gy = torch.randn(B, CH, room, device="cuda") * 0.25
    gx = torch.zeros(B, CH, FRAMES, device="cuda")
    gr = torch.zeros(B, len(small), dtype=torch.float64, device="cuda")
    res = dict(B=B)
    res.update(trio(pool, x, y, gy, gx, gr, frames, ratios, calls, 3))
    if B <= 64:                                                  # (a thousand phases per clip: the host plans every one of them)
        tiny_ratios = [[row[min(k * tiny // BLOCK, K - 1)] for k in range(len(small))] for row in ratios]
        res.update(trio(pool, x, y, gy, gx, gr, small, tiny_ratios, max(3, calls // 3), 1, "_tiny"))
    for r in pool:
        r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tiny", type=int, default=16)
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    a = ap.parse_args()
    lines = ["# [median, 25th, 75th percentile] ms per call, host side included; stereo clips of 16,000 frames, 380 taps, blocks of 1,024 frames",
             "# device: " + torch.cuda.get_device_name(0)]
    for B in [int(v) for v in a.batches.split(",")]:
        lines.append(json.dumps(case(B, a.calls, a.tiny)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
