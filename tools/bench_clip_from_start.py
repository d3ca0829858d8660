"""Whole clips from a fresh start: the clips entries (decimateProcessClipsPlanarLEDevice, resampleProcessAndFlushClipsPlanarDevice with
fromStart) next to the route they replace, rebuilt here and timed in the same run — a reset per context, the batch entry, and for the
decimator a clipped() read-back per context.  B stereo clips of one second at 44.1 kHz; the decimator to 16 bits, once with ATH
shaping and high-pass dither and once with neither; the resampler 44.1 -> 16 kHz with 380 taps.

    python tools/bench_clip_from_start.py [--calls 15] [--out profiles/clips_from_start.txt]

Per case: median wall-clock milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th percentile.
A gain counts when the new route's median is under the old route's 25th percentile.
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
import audio_resampler_amd as A  # noqa: E402

RATE, FRAMES, CH = 44100, 44100, 2
ATH = A.DITHER_HIGHPASS | A.SHAPING_ATH_CURVE
BATCHES = (1, 64, 256, 1024)


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


def decimator_case(B, flags, calls):
    pool = [A.Decimator(CH, 16, 2, 1.0, RATE, flags) for _ in range(B)]
    x = (torch.rand(B, CH, FRAMES, device="cuda") * 2 - 1) * 1.05
    pcm = torch.zeros(B, CH, FRAMES * 2, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(B, dtype=torch.int64, device="cuda")
    ins = [x[i].data_ptr() for i in range(B)]
    outs = [pcm[i].data_ptr() for i in range(B)]
    ip, op, n = [x.stride(1)] * B, [pcm.stride(1)] * B, [FRAMES] * B
    seen = [0] * B

    def old():
        for d in pool:
            d.reset()
        A.decimate_batch_planar_device(pool, ins, ip, n, outs, op)
        after = [d.clipped() for d in pool]
        got = [a - b for a, b in zip(after, seen)]
        seen[:] = after
        return got

    def new():
        A.decimate_clips_planar_device(pool, ins, ip, n, outs, op, from_start=True, d_clip_counts=counts)
        return counts.tolist()

    a = old()
    ref = pcm.clone()
    b = new()
    assert a == b and torch.equal(ref, pcm), "the two routes disagree"
    seen[:] = [d.clipped() for d in pool]
    res = dict(old=timed(old, calls), new=timed(new, calls))
    for d in pool:
        d.close()
    return res


def resampler_case(B, calls):
    flags = A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.INCLUDE_LOWPASS
    pool = [A.Resampler(CH, 380, 380, 0.0, flags, (44100.0, 16000.0, 0)) for _ in range(B)]
    ratio = 16000.0 / 44100.0
    cap = int(FRAMES * ratio) + 380 + 64
    x = torch.randn(B, CH, FRAMES, device="cuda") * 0.25
    y = torch.zeros(B, CH, cap, device="cuda")
    ins = [x[i].data_ptr() for i in range(B)]
    outs = [y[i].data_ptr() for i in range(B)]
    args = (pool, ins, [x.stride(1)] * B, [FRAMES] * B, outs, [y.stride(1)] * B, [cap] * B, [ratio] * B)

    def old():
        for r in pool:
            r.reset()
        return A.process_and_flush_batch_planar_device(*args)

    def new():
        return A.process_and_flush_clips_planar_device(*args, from_start=True)

    a = old()
    ref = y.clone()
    b = new()
    assert a == b and torch.equal(ref, y), "the two routes disagree"
    res = dict(old=timed(old, calls), new=timed(new, calls))
    for r in pool:
        r.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    a = ap.parse_args()
    lines = ["# [median, 25th, 75th percentile] ms per call; old: reset per context + batch entry (+ clipped() per context); new: the clips entry",
             "# device: " + torch.cuda.get_device_name(0)]
    for B in [int(v) for v in a.batches.split(",")]:
        for name, run in (("decimate 16-bit ATH + high-pass dither", lambda: decimator_case(B, ATH, a.calls)),
                          ("decimate 16-bit, no shaping, no dither", lambda: decimator_case(B, 0, a.calls)),
                          ("resample 44.1 -> 16 kHz, 380 taps", lambda: resampler_case(B, a.calls))):
            r = run()
            r.update(case=name, B=B, gain=round(r["old"][0] / r["new"][0], 2), beyond_spread=r["new"][0] < r["old"][1])
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
