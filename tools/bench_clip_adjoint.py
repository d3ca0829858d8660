"""The clip adjoint next to the forward it transposes: resampleAdjointClipsPlanarDevice and, in the same run on the same batch,
resampleProcessAndFlushClipsPlanarDevice from a fresh start — the two do the same number of multiply-adds.  B stereo clips of 16,000
frames, 380 taps, 44.1 -> 16 kHz (160 phases, nearest filter, low-pass) and 16 -> 44.1 kHz (interpolating).  The forward runs on a pool
of B contexts, the adjoint on the first of them for every item.

    python tools/bench_clip_adjoint.py [--calls 15] [--batches 1,64,1024] [--channels 2] [--width 32] [--out profiles/clip_adjoint.txt]

--channels picks the adjoint kernel's channel-group width (1, 2, 3-4, 5 and more), --width the build (32: 4-byte samples, 64: 8-byte).

Per case: median wall-clock milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th percentile, and
the ratio of the medians (adjoint / forward).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from audio_resampler_amd import binding  # noqa: E402

FRAMES, TAPS = 16000, 380
BATCHES = (1, 64, 1024)
RATES = ((44100.0, 16000.0), (16000.0, 44100.0))


def timed(fn, calls, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    q = np.percentile(out, [50, 25, 75])
    return [round(float(v), 3) for v in q]


def case(B, src, dst, calls, CH=2, width=32):
    A = binding(width)
    dt = torch.float64 if width == 64 else torch.float32
    flags = A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.INCLUDE_LOWPASS
    pool = [A.Resampler(CH, TAPS, TAPS, 0.0, flags, (src, dst, 0)) for _ in range(B)]
    ratio = dst / src
    cap = int((FRAMES + TAPS) * ratio) + 64
    x = torch.randn(B, CH, FRAMES, dtype=dt, device="cuda") * 0.25
    y = torch.zeros(B, CH, cap, dtype=dt, device="cuda")
    ins = [x[i].data_ptr() for i in range(B)]
    outs = [y[i].data_ptr() for i in range(B)]

    def forward():
        return A.process_and_flush_clips_planar_device(pool, ins, [x.stride(1)] * B, [FRAMES] * B, outs, [y.stride(1)] * B, [cap] * B,
                                                       [ratio] * B, from_start=True)

    made = [g for _, g in forward()]
    gy = torch.randn(B, CH, cap, dtype=dt, device="cuda") * 0.25
    gx = torch.zeros(B, CH, FRAMES, dtype=dt, device="cuda")
    gouts = [gy[i].data_ptr() for i in range(B)]
    gins = [gx[i].data_ptr() for i in range(B)]

    def adjoint():
        return A.adjoint_clips_planar_device([pool[0]] * B, gouts, [gy.stride(1)] * B, made, gins, [gx.stride(1)] * B, [FRAMES] * B, [ratio] * B)

    # <A x, gy> = <x, A^T gy>: the two calls are each other's transpose
    adjoint()
    torch.cuda.synchronize()
    mask = torch.arange(cap, device="cuda")[None, None, :] < torch.tensor(made, device="cuda")[:, None, None]
    lhs = float((y.double() * gy.double() * mask).sum())
    rhs = float((x.double() * gx.double()).sum())
    res = dict(forward=timed(forward, calls), adjoint=timed(adjoint, calls), transpose_mismatch=float("%.2e" % (abs(lhs - rhs) / max(abs(lhs), 1.0))))
    for r in pool:
        r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--width", type=int, default=32, choices=(32, 64))
    a = ap.parse_args()
    what = "stereo clips" if a.channels == 2 else f"{a.channels}-channel clips"
    if a.width == 64:
        what = "8-byte samples, " + what
    lines = ["# [median, 25th, 75th percentile] ms per call; forward: the clips entry from a fresh start; adjoint: resampleAdjointClipsPlanarDevice",
             f"# {what} of 16,000 frames, 380 taps; device: " + torch.cuda.get_device_name(0)]
    for src, dst in RATES:
        for B in [int(v) for v in a.batches.split(",")]:
            r = case(B, src, dst, a.calls, a.channels, a.width)
            r.update(case=f"{src:g} -> {dst:g}", B=B, adjoint_over_forward=round(r["adjoint"][0] / r["forward"][0], 2))
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
