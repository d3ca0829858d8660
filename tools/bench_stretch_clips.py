"""Whole channels-first clips through the time stretcher: stretchProcessAndFlushBatchPlanarDevice on [B, C, T] rows against the route
it replaces, in one session, the routes taking turns.

    clips    this tree's whole-clip entry on the tensor's own rows, fromStart = 1: one launch, one synchronisation -> [B, C, Tout]
    rounds   the route before it: transpose to interleaved [B, T, C] (torch), stretchProcessBatchDevice, stretchFlushBatchDevice
             rounds behind one another until a round gives nothing for every clip, transpose back to [B, C, Tout]

B clips of 1 s at 44.1 kHz (ART's periods, rate // 350 and rate // 50): mono and stereo at ratios 0.8 and 1.25, and a stereo cascaded
pair at 3.1; B = 1, 16, 64, 256.  Both routes start every timed call from fresh-context state: `clips` by fromStart inside the timed
call; `rounds` by stretchReset OUTSIDE the clock (it keeps the accumulated length error, so a later call's counts can differ
from the first call's by a period; the work is the same).  Buffers are allocated once; `rounds` builds
its pointer table again for every flush round, as it must (each round writes behind the last).  The first call of each case checks
that the two routes give the same counts and the same samples.

One JSON line per case: [median, 25th, 75th percentile] ms of wall clock around call + synchronise over the timed calls, and
rounds_over_clips, the ratio of the medians.  --out PATH also writes the lines as a table.

    python tools/bench_stretch_clips.py [--quick] [--out PATH]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import audio_resampler_amd as A  # noqa: E402
import _stretch as S  # noqa: E402

L = A.lib()
RATE = 44100
SHORT, LONG = RATE // 350, RATE // 50
CASES = [("mono_0.8", 1, 0, 0.8), ("mono_1.25", 1, 0, 1.25), ("stereo_0.8", 2, 0, 0.8), ("stereo_1.25", 2, 0, 1.25),
         ("stereo_dual_3.1", 2, A.STRETCH_DUAL_FLAG, 3.1)]


def quartiles(times):
    return [round(float(v), 3) for v in np.percentile(np.array(times) * 1e3, [50, 25, 75])]


def case(name, ch, flags, ratio, n, calls, warm):
    T = RATE
    base = S.signal(T + 64 * 16, ch, RATE, seed=3)
    x = torch.from_numpy(np.ascontiguousarray(np.stack([base[16 * (i % 64): 16 * (i % 64) + T].T for i in range(n)]))).to("cuda")     # [n, ch, T]
    assert x.stride(2) == 1 and x.stride(1) == T
    cap = L.artamdStretchClipCapacity(LONG, flags, T, ratio)
    y = torch.zeros(n, ch, cap, device="cuda")
    new = [A.Stretcher(SHORT, LONG, ch, flags) for _ in range(n)]
    old = [A.Stretcher(SHORT, LONG, ch, flags) for _ in range(n)]
    size = x.element_size()
    pitches = (x.stride(1), y.stride(1)) if ch > 1 else (0, 0)
    args = ([x.data_ptr() + i * x.stride(0) * size for i in range(n)], [pitches[0]] * n, [T] * n,
            [y.data_ptr() + i * y.stride(0) * size for i in range(n)], [pitches[1]] * n, [cap] * n, [ratio] * n)

    def clips():
        return A.stretch_clips_batch_planar_device(new, *args, from_start=True)

    # the route before: interleaved staging on both sides, one table per round
    xi = torch.empty(n, T, ch, device="cuda")
    oi = torch.zeros(n, cap, ch, device="cuda")
    y_old = torch.zeros(n, ch, cap, device="cuda")
    ctx = (C.c_void_p * n)(*[s.p for s in old])
    ins = (C.c_void_p * n)(*[xi[i].data_ptr() for i in range(n)])
    nin, rat, made = (C.c_int * n)(*([T] * n)), (C.c_double * n)(*([ratio] * n)), (C.c_int * n)()
    row_bytes = ch * size

    def rounds():
        xi.copy_(x.transpose(1, 2))
        total = [0] * n
        outs = (C.c_void_p * n)(*[oi[i].data_ptr() for i in range(n)])
        assert L.stretchProcessBatchDevice(ctx, n, ins, nin, outs, rat, made) == 0
        while True:
            total = [t + g for t, g in zip(total, made)]
            outs = (C.c_void_p * n)(*[oi[i].data_ptr() + t * row_bytes for i, t in enumerate(total)])
            assert L.stretchFlushBatchDevice(ctx, n, outs, made) == 0
            if not any(made):
                break
        m = max(total)
        y_old[:, :, :m].copy_(oi[:, :m].transpose(1, 2))
        return total

    def fresh_old():                                     # (outside the clock)
        for s in old:
            L.stretchReset(s.p)
        torch.cuda.synchronize()

    got_new = clips()
    fresh_old()
    got_old = rounds()
    torch.cuda.synchronize()
    assert got_new == got_old, (got_new[:4], got_old[:4])
    for i in range(n):
        assert torch.equal(y[i, :, :got_new[i]], y_old[i, :, :got_old[i]]), i
    t = {"clips": [], "rounds": []}
    for k in range(warm + calls):
        for route, fn in (("clips", clips), ("rounds", rounds)):
            if route == "rounds":
                fresh_old()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if k >= warm:
                t[route].append(time.perf_counter() - t0)
    row = {"case": name, "clips": n, "channels": ch, "frames": T, "ratio": ratio, "out_frames": got_new[0],
           "clips_ms": quartiles(t["clips"]), "rounds_ms": quartiles(t["rounds"])}
    row["rounds_over_clips"] = round(row["rounds_ms"][0] / row["clips_ms"][0], 2)
    print(json.dumps(row), flush=True)
    for s in new + old:
        s.close()
    return row


def main():
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    head = {"device": torch.cuda.get_device_name(0), "calls": 8 if quick else 20}
    print(json.dumps(head), flush=True)
    rows = [case(name, ch, flags, ratio, n, head["calls"], 2 if quick else 3)
            for name, ch, flags, ratio in CASES for n in ((1, 16) if quick else (1, 16, 64, 256))]
    if out:
        with open(out, "w") as f:
            f.write(f"# tools/bench_stretch_clips.py on {head['device']}: B clips of 1 s at 44.1 kHz, ms per call [median, 25th, 75th] over "
                    f"{head['calls']} calls\n# clips = stretchProcessAndFlushBatchPlanarDevice on [B, C, T] rows; rounds = transpose, "
                    "stretchProcessBatchDevice, stretchFlushBatchDevice rounds, transpose back\n")
            f.write(f"{'case':<18}{'B':>5}  {'clips_ms':<26}{'rounds_ms':<26}{'rounds/clips':>12}\n")
            for r in rows:
                f.write(f"{r['case']:<18}{r['clips']:>5}  {str(r['clips_ms']):<26}{str(r['rounds_ms']):<26}{r['rounds_over_clips']:>12}\n")


if __name__ == "__main__":
    main()
