"""Whole channels-first clips through the biquad banks: biquadBankApplyClipsPlanarDevice against the route it replaces, in one session,
the routes taking turns.

    clips    this tree's entry with fromStart = 1: the clips' time-parallel calls in shared launches, no copy per bank
    batch    the route before it, which stays in the library: biquadBankReset for every bank, then biquadBankApplyBatchPlanarDevice,
             which makes every clip of more than 512 frames its own single time-parallel call

B stereo clips of 1 s at 44.1 kHz through ART's -p cascades (two low-passes: the pre-filter's cut-off of 96 -> 44.1 kHz, the
post-filter's of 44.1 -> 48 kHz), as planes of a [B, C, T] tensor and as interleaved [B, T, C] frames; B = 1, 16, 64, 256, 1024.  Both
routes filter the same buffers in place, from fresh-bank state in every timed call (the reset is part of both: inside the entry, or the
loop in front of the batch entry); the first call of each case checks that the two routes give the same bits and states.

One JSON line per case: [median, 25th, 75th percentile] ms of wall clock around call + synchronise over the timed calls,
batch_over_clips (the ratio of the medians) and `spread`, the larger interquartile range of the two routes as a fraction of its median
(a difference at B = 1 below it is noise).  --out PATH also writes the lines as a table.

    python tools/bench_biquad_clips.py [--quick] [--out PATH]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import audio_resampler_amd as A  # noqa: E402

RATE = 44100
FILTERS = [("pre", 44100 * 0.45 / 96000), ("post", 44100 * 0.45 / 48000)]


def quartiles(times):
    return [round(float(v), 3) for v in np.percentile(np.array(times) * 1e3, [50, 25, 75])]


def banks(n, ch, freq):
    co = A.BiquadCoefficients()
    A.lib().biquad_lowpass(C.byref(co), freq)
    secs = (A.Biquad * (ch * 2))()
    for k in range(ch * 2):
        A.lib().biquad_init(C.byref(secs[k]), C.byref(co), 1.0)
    return [A.BiquadBank(secs, ch, 2) for _ in range(n)]


def case(name, freq, planar, n, calls, warm):
    ch, T = 2, RATE
    g = torch.Generator(device="cuda").manual_seed(5)
    shape = (n, ch, T) if planar else (n, T, ch)
    x0 = torch.rand(*shape, generator=g, device="cuda") * 2 - 1
    bufs = {"clips": x0.clone(), "batch": x0.clone()}
    sets = {"clips": banks(n, ch, freq), "batch": banks(n, ch, freq)}
    size = x0.element_size()
    ptrs = {r: [b.data_ptr() + i * b.stride(0) * size for i in range(n)] for r, b in bufs.items()}
    pitches, frames = [T if planar else 0] * n, [T] * n
    launches = {}

    def clips():
        launches["clips"] = A.biquad_clips_planar_device(sets["clips"], ptrs["clips"], pitches, frames, from_start=True)

    def batch():
        for b in sets["batch"]:
            b.reset()
        launches["batch"] = A.biquad_batch_planar_device(sets["batch"], ptrs["batch"], pitches, frames)

    clips(); batch()
    torch.cuda.synchronize()
    assert torch.equal(bufs["clips"].view(torch.int32), bufs["batch"].view(torch.int32))
    for a, b in zip(sets["clips"][:4] + sets["clips"][-1:], sets["batch"][:4] + sets["batch"][-1:]):
        assert bytes(memoryview(a.read())) == bytes(memoryview(b.read()))
    t = {"clips": [], "batch": []}
    for k in range(warm + calls):
        for route, fn in (("clips", clips), ("batch", batch)):
            bufs[route].copy_(x0)                            # (outside the clock: the same input every call)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= warm:
                t[route].append(time.perf_counter() - t0)
    row = {"filter": name, "layout": "planar" if planar else "interleaved", "clips": n, "channels": ch, "frames": T,
           "clips_ms": quartiles(t["clips"]), "batch_ms": quartiles(t["batch"]), "clips_launches": launches["clips"],
           "batch_launches": launches["batch"], "repairs": sum(b.repairs() for b in sets["clips"])}
    row["batch_over_clips"] = round(row["batch_ms"][0] / row["clips_ms"][0], 2)
    row["spread"] = round(max((q[2] - q[1]) / q[0] for q in (row["clips_ms"], row["batch_ms"])), 3)
    print(json.dumps(row), flush=True)
    for b in sets["clips"] + sets["batch"]:
        b.close()
    return row


def main():
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    head = {"device": torch.cuda.get_device_name(0), "calls": 8 if quick else 20}
    print(json.dumps(head), flush=True)
    rows = [case(name, freq, planar, n, head["calls"], 2 if quick else 3)
            for name, freq in FILTERS for planar in (True, False) for n in ((1, 16) if quick else (1, 16, 64, 256, 1024))]
    if out:
        with open(out, "w") as f:
            f.write(f"# tools/bench_biquad_clips.py on {head['device']}: B stereo clips of 1 s at 44.1 kHz, ART's -p cascades, ms per call "
                    f"[median, 25th, 75th] over {head['calls']} calls\n# clips = biquadBankApplyClipsPlanarDevice (fromStart); batch = "
                    "biquadBankReset per bank + biquadBankApplyBatchPlanarDevice (every clip its own single time-parallel call)\n")
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
