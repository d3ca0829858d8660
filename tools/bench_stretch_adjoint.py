"""The stretcher's adjoint and its logged forward next to the plain forward: stretchProcessAndFlushBatchPlanarDevice from a fresh start,
stretchProcessAndFlushLoggedBatchPlanarDevice and stretchAdjointClipsPlanarDevice on the same batch in the same run, taken in turn so
that a drift of the box falls on all three.  B one-second clips at 44.1 kHz (periods 126 .. 882 frames, ART's), mono and stereo, at
the ratios 0.8, 1.25 and — a STRETCH_DUAL_FLAG pair — 3.1.  The forwards run on a pool of B contexts, the adjoint on the first of them
for every item.

    python tools/bench_stretch_adjoint.py [--calls 15] [--batches 1,64,1024] [--out profiles/stretch_adjoint.txt]

Per case: median wall-clock milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th percentile; the
ratios of the medians; and two checks on the batch that was timed: the logged output equals the plain one, and <A x, g> = <x, A^T g>.
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

RATE = 44100
FRAMES = RATE
PERIODS = (RATE // 350, RATE // 50)
BATCHES = (1, 64, 1024)
CASES = ((0.8, 0), (1.25, 0), (3.1, A.STRETCH_DUAL_FLAG))


def clips(B, ch):
    """pitched clips, each at its own pitch and glide, with a little noise: what the period search is made for"""
    g = torch.Generator(device="cuda").manual_seed(B * 2 + ch)
    t = torch.arange(FRAMES, device="cuda", dtype=torch.float64) / RATE
    f0 = 90.0 + 120.0 * torch.rand(B, 1, 1, generator=g, device="cuda", dtype=torch.float64)
    ph = 2 * np.pi * f0 * (t + 0.05 * torch.sin(2 * np.pi * 0.7 * t)) + 0.3 * torch.arange(ch, device="cuda").view(1, ch, 1)
    x = 0.5 * torch.sin(ph) + 0.2 * torch.sin(2 * ph + 0.3) + 0.02 * torch.randn(B, ch, FRAMES, generator=g, device="cuda", dtype=torch.float64)
    return x.float().contiguous()


def timed_in_turn(fns, calls, warm=2):
    for fn in fns:
        for _ in range(warm):
            fn()
    out = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return [[round(float(v), 3) for v in np.percentile(o, [50, 25, 75])] for o in out]


def case(B, ch, ratio, flags, calls):
    L = A.lib()
    pool = [A.Stretcher(*PERIODS, ch, flags) for _ in range(B)]
    cap = L.artamdStretchClipCapacity(PERIODS[1], flags, FRAMES, ratio)
    stages = 2 if flags & A.STRETCH_DUAL_FLAG else 1
    log_caps = [L.artamdStretchLogCapacity(*PERIODS, flags, FRAMES, ratio, s) for s in (0, 1)]
    x = clips(B, ch)
    y, y2 = torch.zeros(B, ch, cap, device="cuda"), torch.zeros(B, ch, cap, device="cuda")
    logs = torch.zeros(B, sum(log_caps), 4, dtype=torch.int32, device="cuda")
    pitch = lambda t: t.stride(1) if ch > 1 else 0
    rows = lambda t: [t[i].data_ptr() for i in range(B)]
    d_logs = [(logs[i].data_ptr(), logs[i, log_caps[0]:].data_ptr() if stages == 2 else None) for i in range(B)]
    common = (rows(x), [pitch(x)] * B, [FRAMES] * B)
    state = {}

    def plain():
        state["made"] = A.stretch_clips_batch_planar_device(pool, *common, rows(y), [pitch(y)] * B, [cap] * B, [ratio] * B, from_start=True)

    def logged():
        state["made2"], state["counts"] = A.stretch_clips_logged_batch_planar_device(
            pool, *common, rows(y2), [pitch(y2)] * B, [cap] * B, [ratio] * B, d_logs, [log_caps] * B)

    plain(); logged()
    torch.cuda.synchronize()
    made, counts = state["made"], state["counts"]
    same = state["made2"] == made and torch.equal(y, y2)
    gy = torch.randn(B, ch, cap, device="cuda") * 0.25
    gx = torch.zeros(B, ch, FRAMES, device="cuda")

    def adjoint():
        state["launches"] = A.stretch_adjoint_clips_planar_device([pool[0]] * B, d_logs, counts, rows(gy), [pitch(gy)] * B, made,
                                                                  rows(gx), [pitch(gx)] * B, [FRAMES] * B)

    adjoint()
    torch.cuda.synchronize()
    mask = torch.arange(cap, device="cuda")[None, None, :] < torch.tensor(made, device="cuda")[:, None, None]
    lhs = float((y.double() * gy.double() * mask).sum())
    rhs = float((x.double() * gx.double()).sum())
    t_plain, t_logged, t_adjoint = timed_in_turn([plain, logged, adjoint], calls)
    res = dict(forward=t_plain, logged=t_logged, adjoint=t_adjoint, launches=state["launches"],
               logged_over_forward=round(t_logged[0] / t_plain[0], 3), adjoint_over_forward=round(t_adjoint[0] / t_plain[0], 4),
               segments_per_clip=round(float(np.mean([sum(c) for c in counts])), 1), logged_equals_plain=bool(same),
               transpose_mismatch=float("%.2e" % (abs(lhs - rhs) / max(abs(lhs), 1.0))))
    for s in pool:
        s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    a = ap.parse_args()
    lines = ["# [median, 25th, 75th percentile] ms per call, the three taken in turn; forward: stretchProcessAndFlushBatchPlanarDevice from a fresh start;",
             "# logged: stretchProcessAndFlushLoggedBatchPlanarDevice; adjoint: stretchAdjointClipsPlanarDevice.  One-second clips at 44.1 kHz, float;",
             "# device: " + torch.cuda.get_device_name(0)]
    for ch in (1, 2):
        for ratio, flags in CASES:
            for B in [int(v) for v in a.batches.split(",")]:
                r = dict(channels=ch, ratio=ratio, dual=bool(flags), B=B)
                r.update(case(B, ch, ratio, flags, a.calls))
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
