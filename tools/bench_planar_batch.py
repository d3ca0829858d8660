#!/usr/bin/env python3
"""Batches of channels-first clips on one GPU: N stereo clips [N, 2, frames], one ordinary call per clip, three ways.

    python tools/bench_planar_batch.py [--before LIB] [--sizes 1,4,16,64,256,1024] [--reps 5] [--out profiles/planar_batch.txt]

Cases:
  general  stereo x 380 taps, 44.1 -> 16 kHz, 4,000 frames a clip: every call stays planar on the general kernel;
  staged   stereo x 988 taps, 44.1 -> 48 kHz, kernel preference 6, 102,400 frames a clip (frames x channels x taps = 2.02e8 >= 2e8): every
           call goes through the context's interleaved staging; sizes above --staged-max clips are not run (device memory: about 5 MB a clip with its staging and the transposed copies).
Columns, each measured in a child process of its own so that one library is loaded per process:
  before/loop     the loop of resampleProcessPlanarDevice calls with the library of --before (the parent commit's build);
  this/loop       the same loop with this tree's library;
  this/transpose  x.transpose (1, 2).contiguous (), resampleProcessBatchInterleavedDevice, and the transpose back;
  this/planar     ONE resampleProcessBatchPlanarDevice call on the tensor's own rows.
Two warm-up calls (the second is the steady state: a staged stream's first matrix launch builds its rows and is a single call), then --reps
timed repetitions of one call per context on a continuing stream; the timed window is the wall clock round the calls and a final
synchronise.  Medians with the 25th and 75th percentile.  One JSON line per measurement, also appended to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"general": dict(ch=2, T=380, frames=4000, rates=(44100.0, 16000.0), pref=0),
         "staged": dict(ch=2, T=988, frames=102400, rates=(44100.0, 48000.0), pref=6)}


def emit(args, row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


def child(args):
    import ctypes as C
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import audio_resampler_amd as A
    B = A.binding(32)
    modes = args.modes.split(",")
    if modes == ["loop"]:                    # (a library from before the planar batch entries existed: the loop needs the single call only)
        for name in ("resampleProcessAndFlushPlanarDevice", "resampleProcessBatchPlanarDevice", "resampleProcessAndFlushBatchPlanarDevice"):
            B.EXPORTED_SYMBOLS.pop(name, None)
    L = B.lib()
    for case in args.cases.split(","):
        k = CASES[case]
        ch, T, frames, ratio = k["ch"], k["T"], k["frames"], k["rates"][1] / k["rates"][0]
        flags = A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE
        cap = int(frames * ratio) + 64
        for n in [int(v) for v in args.sizes.split(",")]:
            if case == "staged" and n > args.staged_max:
                continue
            rs = [B.Resampler(ch, T, T, 0.0, flags, (k["rates"][0], k["rates"][1], 0)) for _ in range(n)]
            for r in rs:
                if k["pref"]:
                    r.set_kernel(k["pref"])
                r.advance(T / 2)
            x = 0.25 * torch.randn(n, ch, frames, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
            y = torch.zeros(n, ch, cap, device="cuda")
            yi = torch.zeros(n, cap, ch, device="cuda")
            ctx = (C.c_void_p * n)(*[C.cast(r.p, C.c_void_p) for r in rs])
            ptrs = lambda t: (C.c_void_p * n)(*[t[i].data_ptr() for i in range(n)])
            a_in, a_out, a_outi = ptrs(x), ptrs(y), ptrs(yi)
            a_ip, a_op = (C.c_long * n)(*([frames] * n)), (C.c_long * n)(*([cap] * n))
            a_n, a_cap, a_ratio = (C.c_int * n)(*([frames] * n)), (C.c_int * n)(*([cap] * n)), (C.c_double * n)(*([ratio] * n))
            res = (B.ResampleResult * n)()

            def loop():
                for i, r in enumerate(rs):
                    res[i] = L.resampleProcessPlanarDevice(r.p, a_in[i], frames, frames, a_out[i], cap, cap, ratio)

            def transpose():
                xi = x.transpose(1, 2).contiguous()
                assert L.resampleProcessBatchInterleavedDevice(ctx, n, ptrs(xi), a_n, a_outi, a_cap, a_ratio, res) == 0
                y.copy_(yi.transpose(1, 2))

            def planar():
                assert L.resampleProcessBatchPlanarDevice(ctx, n, a_in, a_ip, a_n, a_out, a_op, a_cap, a_ratio, res) == 0

            for mode in modes:
                fn = {"loop": loop, "transpose": transpose, "planar": planar}[mode]
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                times = []
                for _ in range(args.reps):
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
                t = np.array(times) * 1e3
                emit(args, {"lib": args.label, "mode": mode, "case": case, "clips": n, "frames": frames, "reps": args.reps,
                            "ms_median": round(float(np.median(t)), 4), "ms_p25": round(float(np.percentile(t, 25)), 4),
                            "ms_p75": round(float(np.percentile(t, 75)), 4), "us_per_clip": round(float(np.median(t)) * 1e3 / n, 2),
                            "outputs": sum(res[i].output_generated for i in range(n)), "last_kernel": rs[0].last_kernel()})
            for r in rs:
                r.close()
            del x, y, yi


def run_child(args, label, lib, modes):
    env = dict(os.environ)
    if lib:
        env["ARTAMD_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--label", label, "--modes", modes, "--sizes", args.sizes, "--cases", args.cases,
           "--reps", str(args.reps), "--staged-max", str(args.staged_max)] + (["--out", args.out] if args.out else [])
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", help="libartamd.so of another build (the parent commit): its loop is the baseline column")
    ap.add_argument("--sizes", default="1,4,16,64,256,1024")
    ap.add_argument("--cases", default="general,staged")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--staged-max", type=int, default=1024)
    ap.add_argument("--out", help="append every JSON line to this file (profiles/planar_batch.txt)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--modes", default="loop,transpose,planar")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    props = torch.cuda.get_device_properties(0)
    # (the run's settings, not its command line: where the other build's library and the output file lie says nothing about the measurement)
    emit(args, {"device": props.name, "gcn_arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count, "sizes": args.sizes,
                "cases": args.cases, "reps": args.reps, "staged_max": args.staged_max, "before": bool(args.before)})
    rc = 0
    if args.before:
        rc |= run_child(args, "before", args.before, "loop")
    rc |= run_child(args, "this", None, "loop,transpose,planar")
    return rc


if __name__ == "__main__":
    sys.exit(main())
