"""Blocks of one stream in one launch (resampleProcessScheduleInterleavedDevice) against the per-call loop, on config E's stream.

BASELINE configs[4] (config E): stereo, 380 taps x 380 filters, nearest filter, a new ratio every block from the sequence
DST/SRC x (1 + 100e-6 sin(2 pi i / 64)) — every 32nd entry is exactly 160/147, which the matrix-core path takes, so a schedule is cut there.
For blocks of 4,096, 16,384 and 65,536 frames and K = 1, 4, 16, 64 blocks per schedule, twin contexts play the same 64 blocks: one as
schedules of K blocks, the other as single calls.  Reported per point: wall-clock Msamples/s (input samples; medians of alternating runs,
each ending in a synchronisation), FIR-kernel time per block and launches from resampleHipReadTiming (a separate timed run), and the
schedule's speed-up.  One process; one JSON line per point, a summary table at the end.

    timeout -k 10 600 python tools/bench_schedule.py [--reps 7] [--blocks 4096,16384,65536] [--ks 1,4,16,64]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import audio_resampler_amd as A  # noqa: E402

SRC, DST, CH, TAPS = 44100, 48000, 2, 380
TOTAL_BLOCKS = 64


def ratio(i):
    return DST / SRC * (1 + 100e-6 * math.sin(2 * math.pi * i / 64))


def make():
    r = A.Resampler(CH, TAPS, TAPS, 0.0, A.BLACKMAN_HARRIS)
    r.advance(TAPS / 2)
    return r


def play(r, x, d_out, B, K, first, schedule):
    """TOTAL_BLOCKS blocks of B frames from block index `first`, as schedules of K or as single calls"""
    ratios = [ratio(first + i) for i in range(TOTAL_BLOCKS)]
    caps = [int(B * q) + 64 for q in ratios]
    if schedule:
        out = 0
        for j in range(0, TOTAL_BLOCKS, K):
            made, res = r.process_schedule_device(x[j * B:], [B] * K, d_out[out:], caps[j:j + K], ratios[j:j + K])
            assert made == K and all(u == B for u, _ in res), (made, res)
            out += sum(g for _, g in res)
    else:
        out = 0
        for j in range(TOTAL_BLOCKS):
            u, g = r.process_device(x[j * B:], B, d_out[out:], caps[j], ratios[j])
            assert u == B
            out += g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--blocks", default="4096,16384,65536")
    ap.add_argument("--ks", default="1,4,16,64")
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    rows = []
    for B in [int(v) for v in args.blocks.split(",")]:
        x = torch.from_numpy((rng.standard_normal((TOTAL_BLOCKS * B + 4096, CH)) * 0.25).astype(np.float32)).cuda()
        d_out = torch.zeros((int(TOTAL_BLOCKS * B * DST / SRC * 1.01) + 64 * TOTAL_BLOCKS, CH), device="cuda")
        for K in [int(v) for v in args.ks.split(",")]:
            sched, single = make(), make()
            first = 1
            play(sched, x, d_out, B, K, first, True); play(single, x, d_out, B, K, first, False)        # warm-up
            first += TOTAL_BLOCKS
            torch.cuda.synchronize()
            wall = {True: [], False: []}
            for rep in range(args.reps):
                for side in ((True, False) if rep % 2 == 0 else (False, True)):
                    r = sched if side else single
                    t0 = time.perf_counter()
                    play(r, x, d_out, B, K, first, side)
                    r.synchronize()
                    wall[side].append(time.perf_counter() - t0)
                first += TOTAL_BLOCKS
            timed = {}
            for side, r in ((True, sched), (False, single)):
                r.set_timing(True)
                play(r, x, d_out, B, K, first, side)
                ms, launches = r.read_timing()
                r.set_timing(False)
                timed[side] = (ms, launches)
            first += TOTAL_BLOCKS
            samples = TOTAL_BLOCKS * B * CH
            row = {"block": B, "K": K,
                   "schedule_msps": samples / statistics.median(wall[True]) / 1e6,
                   "loop_msps": samples / statistics.median(wall[False]) / 1e6,
                   "schedule_kernel_us_per_block": timed[True][0] * 1e3 / TOTAL_BLOCKS,
                   "loop_kernel_us_per_block": timed[False][0] * 1e3 / TOTAL_BLOCKS,
                   "schedule_launches": timed[True][1], "loop_launches": timed[False][1]}
            row["wall_speedup"] = row["schedule_msps"] / row["loop_msps"]
            print(json.dumps(row), flush=True)
            rows.append(row)
            sched.close(); single.close()
    print(f"\n{'block':>6} {'K':>3} | {'sched Msps':>10} {'loop Msps':>10} {'x':>5} | {'sched us/blk':>12} {'loop us/blk':>11} | launches")
    for r in rows:
        print(f"{r['block']:>6} {r['K']:>3} | {r['schedule_msps']:>10.1f} {r['loop_msps']:>10.1f} {r['wall_speedup']:>5.2f} | "
              f"{r['schedule_kernel_us_per_block']:>12.2f} {r['loop_kernel_us_per_block']:>11.2f} | {r['schedule_launches']} / {r['loop_launches']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
