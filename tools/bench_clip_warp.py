"""The variable-rate clip entries next to what they replace and what they transpose, everything in turn in one run on the same batch:

  forward          resampleProcessScheduleClipsPlanarDevice from a fresh start (one zeroing launch, then the schedule's launches)
  forward_before   the route before it: resampleReset per context, then resampleProcessScheduleBatchPlanarDevice
  adjoint          resampleAdjointScheduleClipsPlanarDevice (K blocks and the flush: K + 1 phases)
  and, at a constant ratio of 1.0884 with the same blocks,
  adjoint_const    the same entry, every block at that ratio
  adjoint_2phase   resampleAdjointClipsPlanarDevice (one process call and the flush) on the same clips
  and, to show where the blocks kernel is slow, the same clips cut into tiny blocks (--tiny frames each)
  adjoint_tiny     resampleAdjointScheduleClipsPlanarDevice (batches up to 64)

B stereo clips of 16,000 frames, 380 taps, blocks of 1,024 frames, ratios a slow walk inside 0.9 .. 1.1.

    python tools/bench_clip_warp.py [--calls 15] [--batches 1,64,1024] [--tiny 16] [--out FILE]

The lines it prints (and writes to FILE) are kept in profiles/clip_warp.txt, section 2, beside what was read from them.

Per case: median wall-clock milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th percentile; and
for the adjoints `device_ms`, the call's time on the device alone (events around a call enqueued behind other work).
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

FRAMES, CH, TAPS, BLOCK = 16000, 2, 380, 1024
BATCHES = (1, 64, 1024)
CONST = 1.0884


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


def device_ms(fn, calls=5):
    """the call's time on the device alone (upload and kernels): enqueued behind a few large matrix products, so that the host part of the
    call — planning, the wrapper's lists — is over before the stream reaches it; median of `calls`"""
    big = torch.randn(8192, 8192, device="cuda")
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        for _ in range(4):
            big @ big
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_time(end))
    return round(float(np.median(out)), 3)


def walk(rng, blocks):
    """a slow random walk of the ratio inside 0.9 .. 1.1, one value per block"""
    r, out = 1.0, []
    for _ in range(blocks):
        r = min(1.1, max(0.9, r + 0.01 * float(rng.standard_normal())))
        out.append(r)
    return out


def cut(block):
    return [min(block, FRAMES - k) for k in range(0, FRAMES, block)]


def case(B, calls, tiny):
    flags = A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.INCLUDE_LOWPASS
    pool = [A.Resampler(CH, TAPS, TAPS, 0.0, flags) for _ in range(B)]
    rng = np.random.default_rng(7)
    frames = cut(BLOCK)
    K = len(frames)
    ratios = [walk(rng, K) for _ in range(B)]
    caps = [[int((n + 2) * r) + 4 for n, r in zip(frames, row)] for row in ratios]
    for c, row in zip(caps, ratios):
        c[-1] = int((frames[-1] + TAPS // 2 + 2) * row[-1]) + 4
    room = max(sum(c) for c in caps)
    x = torch.randn(B, CH, FRAMES, device="cuda") * 0.25
    y = torch.zeros(B, CH, room, device="cuda")
    ins, outs = [x[i].data_ptr() for i in range(B)], [y[i].data_ptr() for i in range(B)]
    args = (pool, ins, [x.stride(1)] * B, [frames] * B, outs, [y.stride(1)] * B, caps, ratios)
    state = {}

    def forward():
        state["fwd"] = A.process_schedule_clips_planar_device(*args, flush_last=[True] * B, from_start=True)

    def forward_before():
        for r in pool:
            r.reset()
        state["old"] = A.process_schedule_batch_planar_device(*args, flush_last=[True] * B)

    forward()
    torch.cuda.synchronize()
    launches, got = state["fwd"]
    assert all(made == K and all(used == n for (used, _), n in zip(res, frames)) for made, res in got)
    made = [sum(g for _, g in res) for _, res in got]
    kept = y.clone()
    forward_before()
    torch.cuda.synchronize()
    assert torch.equal(kept, y) and state["old"][1] == got, "the two forward routes disagree"

    count = int(FRAMES * CONST)                                  # (the constant-ratio cases' gradient frames: under their clips' outputs)
    gy = torch.randn(B, CH, max(room, count), device="cuda") * 0.25
    gx = torch.zeros(B, CH, FRAMES, device="cuda")
    gouts, gins = [gy[i].data_ptr() for i in range(B)], [gx[i].data_ptr() for i in range(B)]

    def adjoint():
        state["adj"] = A.adjoint_schedule_clips_planar_device([pool[0]] * B, gouts, [gy.stride(1)] * B, made, gins, [gx.stride(1)] * B, [frames] * B, ratios)

    # <A x, gy> = <x, A^T gy>: the two calls are each other's transpose
    adjoint()
    torch.cuda.synchronize()
    mask = torch.arange(room, device="cuda")[None, None, :] < torch.tensor(made, device="cuda")[:, None, None]
    lhs = float((y.double() * gy[:, :, :room].double() * mask).sum())
    rhs = float((x.double() * gx.double()).sum())
    res = dict(B=B, blocks=K, forward=timed(forward, calls), forward_before=timed(forward_before, calls), adjoint=timed(adjoint, calls),
               forward_launches=launches, forward_before_launches=state["old"][0], adjoint_launches=state["adj"],
               transpose_mismatch=float("%.2e" % (abs(lhs - rhs) / max(abs(lhs), 1.0))))

    # a constant ratio: the blocks entry against the two-phase entry on the same clips (zero gradient past the shorter of the two counts:
    # cutting a clip into calls may move its output count by a frame)
    flat = [[CONST] * K] * B
    gx2 = torch.zeros(B, CH, FRAMES, device="cuda")
    gins2 = [gx2[i].data_ptr() for i in range(B)]

    def adjoint_const():
        return A.adjoint_schedule_clips_planar_device([pool[0]] * B, gouts, [gy.stride(1)] * B, [count] * B, gins, [gx.stride(1)] * B, [frames] * B, flat)

    def adjoint_2phase():
        return A.adjoint_clips_planar_device([pool[0]] * B, gouts, [gy.stride(1)] * B, [count] * B, gins2, [gx2.stride(1)] * B, [FRAMES] * B, [CONST] * B)

    res.update(adjoint_const=timed(adjoint_const, calls), adjoint_2phase=timed(adjoint_2phase, calls))
    res["const_max_difference"] = float("%.2e" % float((gx - gx2).abs().max()))
    res["device_ms"] = dict(adjoint=device_ms(adjoint), adjoint_const=device_ms(adjoint_const), adjoint_2phase=device_ms(adjoint_2phase))

    small = cut(tiny)
    tiny_ratios = [[row[min(k * tiny // BLOCK, K - 1)] for k in range(len(small))] for row in ratios]

    def adjoint_tiny():
        return A.adjoint_schedule_clips_planar_device([pool[0]] * B, gouts, [gy.stride(1)] * B, [count // 2] * B, gins, [gx.stride(1)] * B,
                                                      [small] * B, tiny_ratios)

    if B <= 64:                                                  # (a thousand phases per clip: the host plans every one of them)
        res.update(tiny_blocks=len(small), adjoint_tiny=timed(adjoint_tiny, max(3, calls // 3), warm=1))
    res.update(adjoint_over_forward=round(res["adjoint"][0] / res["forward"][0], 2),
               forward_over_before=round(res["forward"][0] / res["forward_before"][0], 2),
               const_over_2phase=round(res["adjoint_const"][0] / res["adjoint_2phase"][0], 2))
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
