"""N streams x K buffered blocks in one call (resampleProcessScheduleBatchInterleavedDevice) against the two routes without it:
N single schedules (resampleProcessScheduleInterleavedDevice per stream) and K batches (resampleProcessBatchInterleavedDevice per block index).

Stereo streams, 380 taps x 380 filters, nearest filter (config E's stream), blocks of 480 frames, block k of every stream at entry k + 1 of
config E's ratio sequence DST/SRC x (1 + 100e-6 sin(2 pi i / 64)).  For N in 16, 256, 1024 and K in 1, 4, 16 three sets of N contexts play
the same tick (every stream's K blocks) over and over, each by its route.  The C entries are called with argument arrays built once, so
the time is the library's, not the binding's.  Reported per point: wall-clock microseconds per tick, device-resident — the median over
--reps windows of --ticks ticks, each window ending in a device synchronisation, the routes alternating — with the windows' spread, the
launches the new entry reports, and its speed-up over the better of the two other routes.  The first tick of fresh contexts is compared
bit for bit across the three routes.  One process; one JSON line per point, a summary table at the end.

    timeout -k 10 900 python tools/bench_schedule_batch.py [--reps 9] [--ticks 20] [--streams 16,256,1024] [--blocks 1,4,16]
"""
import argparse
import ctypes as C
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

SRC, DST, CH, TAPS, BLOCK = 44100, 48000, 2, 380, 480


def ratio(i):
    return DST / SRC * (1 + 100e-6 * math.sin(2 * math.pi * i / 64))


def make(n):
    rs = [A.Resampler(CH, TAPS, TAPS, 0.0, A.BLACKMAN_HARRIS) for _ in range(n)]
    for r in rs:
        r.advance(TAPS / 2)
    return rs


class Tick:
    """the three routes' argument arrays for N streams x K blocks (x [N, K * BLOCK, CH] in, one [N, K * cap, CH] output per route)"""

    def __init__(self, N, K, x, outs):
        self.L, self.N, self.K = A.lib(), N, K
        self.ratios = [ratio(k + 1) for k in range(K)]
        self.cap = int(BLOCK * max(self.ratios)) + 64
        vp = lambda values: (C.c_void_p * len(values))(*values)
        ints = lambda values: (C.c_int * len(values))(*values)
        self.sets = [make(N) for _ in range(3)]
        ctx = [vp([C.cast(r.p, C.c_void_p).value for r in rs]) for rs in self.sets]
        self.keep = []
        # the new entry: one call
        frames, caps, rates = ints([BLOCK] * K), ints([self.cap] * K), (C.c_double * K)(*self.ratios)
        self.res_a = [(A.ResampleResult * K)() for _ in range(N)]
        self.made = (C.c_int * N)()
        self.args_a = (ctx[0], N, ints([K] * N), vp([x[s].data_ptr() for s in range(N)]), vp([C.addressof(frames)] * N),
                       vp([outs[0][s].data_ptr() for s in range(N)]), vp([C.addressof(caps)] * N), vp([C.addressof(rates)] * N), None,
                       vp([C.addressof(r) for r in self.res_a]), self.made)
        # N single schedules
        self.res_b = [(A.ResampleResult * K)() for _ in range(N)]
        self.args_b = [(self.sets[1][s].p, K, x[s].data_ptr(), frames, outs[1][s].data_ptr(), caps, rates, 0, self.res_b[s]) for s in range(N)]
        # K batches (block k's outputs at frame k * cap of the stream's output)
        self.res_c = [(A.ResampleResult * N)() for _ in range(K)]
        self.args_c = [(ctx[2], N, vp([x[s][k * BLOCK:].data_ptr() for s in range(N)]), ints([BLOCK] * N),
                        vp([outs[2][s][k * self.cap:].data_ptr() for s in range(N)]), ints([self.cap] * N), (C.c_double * N)(*([self.ratios[k]] * N)),
                        self.res_c[k]) for k in range(K)]
        self.keep += [frames, caps, rates]

    def batch(self):
        rc = self.L.resampleProcessScheduleBatchInterleavedDevice(*self.args_a)
        assert rc > 0, rc
        return rc

    def schedules(self):
        for a in self.args_b:
            assert self.L.resampleProcessScheduleInterleavedDevice(*a) == self.K
        return self.N

    def batches(self):
        for a in self.args_c:
            assert self.L.resampleProcessBatchInterleavedDevice(*a) == 0
        return self.K

    def close(self):
        for rs in self.sets:
            for r in rs:
                r.close()


def first_tick_agrees(t, outs):
    """fresh contexts: the three routes make the same counts and the same samples"""
    t.batch(); t.schedules(); t.batches()
    torch.cuda.synchronize()
    for s in range(t.N):
        at = 0
        for k in range(t.K):
            a, b, c = t.res_a[s][k], t.res_b[s][k], t.res_c[k][s]
            assert (a.input_used, a.output_generated) == (b.input_used, b.output_generated) == (c.input_used, c.output_generated) == (BLOCK, a.output_generated)
            g = a.output_generated
            assert torch.equal(outs[0][s][at:at + g], outs[1][s][at:at + g]) and torch.equal(outs[0][s][at:at + g], outs[2][s][k * t.cap:k * t.cap + g]), (s, k)
            at += g
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--streams", default="16,256,1024")
    ap.add_argument("--blocks", default="1,4,16")
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    rows = []
    for N in [int(v) for v in args.streams.split(",")]:
        for K in [int(v) for v in args.blocks.split(",")]:
            x = torch.from_numpy((rng.standard_normal((N, K * BLOCK, CH)) * 0.25).astype(np.float32)).cuda()
            cap = int(BLOCK * max(ratio(k + 1) for k in range(K))) + 64
            outs = [torch.zeros((N, K * cap, CH), device="cuda") for _ in range(3)]
            torch.cuda.synchronize()
            t = Tick(N, K, x, outs)
            agree = first_tick_agrees(t, outs)
            routes = {"batch": t.batch, "schedules": t.schedules, "batches": t.batches}
            launches = 0
            for name, fn in routes.items():                     # warm-up
                for _ in range(3):
                    got = fn()
                    launches = got if name == "batch" else launches
            torch.cuda.synchronize()
            wall = {name: [] for name in routes}
            names = list(routes)
            for rep in range(args.reps):
                for name in names[rep % 3:] + names[:rep % 3]:
                    fn = routes[name]
                    t0 = time.perf_counter()
                    for _ in range(args.ticks):
                        fn()
                    torch.cuda.synchronize()
                    wall[name].append((time.perf_counter() - t0) / args.ticks * 1e6)
            row = {"streams": N, "blocks": K, "first_tick_agrees": agree, "batch_launches": launches}
            for name in names:
                row[name + "_us"] = statistics.median(wall[name])
                row[name + "_us_min_max"] = [min(wall[name]), max(wall[name])]
            row["speedup_over_better"] = min(row["schedules_us"], row["batches_us"]) / row["batch_us"]
            print(json.dumps(row), flush=True)
            rows.append(row)
            t.close()
    print(f"\n{'N':>5} {'K':>3} | {'new us':>9} {'N scheds':>9} {'K batches':>9} | {'x better':>8} | launches")
    for r in rows:
        print(f"{r['streams']:>5} {r['blocks']:>3} | {r['batch_us']:>9.1f} {r['schedules_us']:>9.1f} {r['batches_us']:>9.1f} | "
              f"{r['speedup_over_better']:>8.2f} | {r['batch_launches']} / {r['streams']} / {r['blocks']}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
