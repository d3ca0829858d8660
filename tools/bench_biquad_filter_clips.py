"""The out-of-place clip filter next to the routes it replaces, in one run on the same batch: biquadBankFilterClipsPlanarDevice
forwards against clone + ClipFilter, and with time reversed (the gradient) against flip + clone + ClipFilter + flip.  B stereo clips
of one second at 44.1 kHz through ART's pre-filter and post-filter (two low-pass sections each).  The new calls list one bank B times;
ClipFilter works on its pool of B banks.

    python tools/bench_biquad_filter_clips.py [--calls 15] [--batches 1,64,1024] [--out FILE]

Per case: median wall-clock milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th percentile, and
the ratio of the medians (new / replaced).  torch.flip already returns a copy, so the reversed route is timed twice: as the issue
spells it (flip, clone, filter, flip) and lean (flip, filter, flip).
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

FRAMES, CH = 44100, 2
BATCHES = (1, 64, 1024)
FILTERS = (("pre", 44100 * 0.45 / 96000), ("post", 44100 * 0.45 / 48000))      # ART's -p cut-offs, 96 -> 44.1 kHz and 44.1 -> 48 kHz


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


def case(B, freq, calls):
    cf = A.ClipFilter(CH, [("lowpass", freq), ("lowpass", freq)], max_batch=B)
    x = torch.randn(B, CH, FRAMES, device="cuda") * 0.25
    y = torch.empty_like(x)
    cf(x.clone())                                             # (the pool's banks; the new calls read the first)
    bank = cf.pool[0]
    ins, outs, pitch = [x[i].data_ptr() for i in range(B)], [y[i].data_ptr() for i in range(B)], [x.stride(1)] * B

    def new(reverse):
        return lambda: A.biquad_filter_clips_planar_device([bank] * B, ins, pitch, outs, pitch, [FRAMES] * B, reversed=reverse)

    def clone_filter():
        return cf(x.clone())

    def flip_clone_filter_flip():
        return cf(x.flip(2).clone()).flip(2)

    def flip_filter_flip():
        return cf(x.flip(2)).flip(2)

    # the same bits either way
    new(False)()
    same_forward = bool(torch.equal(y, clone_filter()))
    new(True)()
    same_reversed = bool(torch.equal(y, flip_filter_flip()))
    res = dict(forward=timed(new(False), calls), clone_filter=timed(clone_filter, calls), reversed=timed(new(True), calls),
               flip_clone_filter_flip=timed(flip_clone_filter_flip, calls), flip_filter_flip=timed(flip_filter_flip, calls),
               launches=new(True)(), route_launches=cf.launches, same_bits=same_forward and same_reversed)
    torch.cuda.synchronize()
    cf.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    a = ap.parse_args()
    lines = ["# [median, 25th, 75th percentile] ms per call; forward / reversed: biquadBankFilterClipsPlanarDevice on one bank listed B times;",
             "# clone_filter, flip_clone_filter_flip, flip_filter_flip: the torch routes around the in-place ClipFilter (a pool of B banks)",
             f"# stereo clips of {FRAMES:,} frames, 4-byte samples, two low-pass sections; device: " + torch.cuda.get_device_name(0)]
    for name, freq in FILTERS:
        for B in [int(v) for v in a.batches.split(",")]:
            r = case(B, freq, a.calls)
            r.update(filter=name, B=B, forward_over_route=round(r["forward"][0] / r["clone_filter"][0], 2),
                     reversed_over_route=round(r["reversed"][0] / r["flip_clone_filter_flip"][0], 2),
                     reversed_over_lean_route=round(r["reversed"][0] / r["flip_filter_flip"][0], 2))
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
