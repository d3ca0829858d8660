#!/usr/bin/env python3
"""Many streams' matrix-core calls in one batch call: N contexts of one shape, device-resident input and output, row sets warm (every
context has made one single call), then resampleProcessBatchInterleavedDevice call after call.

    python tools/bench_matrix_batch.py --before LIB [--sizes 1,2,4,8,16,64,256] [--cases ...] [--reps 7] [--calls 20]

Three columns, each measured in a child process of its own so that one library is loaded per process:
  before   the same batch call with the library of --before (another build's libartamd.so: the parent commit's, which makes these calls
           one by one) — the baseline;
  singles  this tree's library with ARTAMD_BATCH_MATRIX=0 (the cross-check of the baseline: the same one-by-one calls);
  grouped  this tree's library as it ships (one grouped launch per shape).
A repetition is --calls batch calls back to back and one synchronise of the stream, the wall clock around them; reported per stream
call (time / calls / N): median, 25th and 75th percentile over --reps repetitions after one warm-up repetition.  `gathered` is how many
of the N contexts report resampleHipLastGathered after the last call.  Cases:
  stereo380_24576 / stereo380_4096   2 ch x 380 taps, 44.1 -> 48 k fixed ratio (nearest filter: the pass-through pass), preference 6
  c8_988_16384 / c8_988_65536        8 ch x 988 taps interpolating, preference 6
  policy_c8_988_441                  8 ch x 988 taps under the cut-invariant policy, 441-frame ticks
Prints one JSON line per measurement.  FIR-kernel time and the fraction of the f32 matrix peak are not this tool's: they come from a
kernel trace of one column (`rocprofv3 --kernel-trace --stats -- python tools/bench_matrix_batch.py --child --label grouped --sizes 64 ...`,
and the same with ARTAMD_BATCH_MATRIX=0), whose per-kernel totals divide by the calls made."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {
    # name: (channels, taps, kernel preference, policy, frames per call)
    "stereo380_24576": (2, 380, 6, False, 24576),
    "stereo380_4096": (2, 380, 6, False, 4096),
    "c8_988_16384": (8, 988, 6, False, 16384),
    "c8_988_65536": (8, 988, 6, False, 65536),
    "policy_c8_988_441": (8, 988, 0, True, 441),
}


def child(args):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import audio_resampler_amd as A
    B = A.binding(32)
    for case in args.cases.split(","):
        ch, T, pref, policy, frames = CASES[case]
        for n in [int(v) for v in args.sizes.split(",")]:
            if n * frames * ch * 4 * 2.2 > args.max_bytes:
                continue
            rs = []
            for _ in range(n):
                r = B.Resampler(ch, T, T, 0.0, A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE, (44100.0, 48000.0, 0))
                if pref:
                    r.set_kernel(pref)
                if policy:
                    r.set_cut_invariant(True)
                r.advance(T / 2)
                rs.append(r)
            cap = int(frames * 48000 / 44100) + 64
            x = torch.rand(n, frames, ch, device="cuda") - 0.5
            y = torch.zeros(n, cap, ch, device="cuda")
            warm_in = torch.rand(max(frames, 8192), ch, device="cuda") - 0.5
            warm_out = torch.zeros(int(warm_in.shape[0] * 1.1) + 64, ch, device="cuda")
            for r in rs:                                    # the first matrix launch of a stream builds its rows: outside the timed window
                r.process_device(warm_in, warm_in.shape[0], warm_out, warm_out.shape[0], 0.0)
            d_in, d_out = [x[i] for i in range(n)], [y[i] for i in range(n)]
            ns, caps, ratios = [frames] * n, [cap] * n, [0.0] * n

            def rep():
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    B.process_batch_device(rs, d_in, ns, d_out, caps, ratios)
                torch.cuda.synchronize()
                return time.perf_counter() - t0

            rep()
            t = np.array([rep() for _ in range(args.reps)]) * 1e6 / args.calls / n
            gathered = sum(r.last_gathered() for r in rs)
            kernels = sorted({r.last_kernel() for r in rs})
            digest = int(y.view(torch.int32).to(torch.int64).sum().item())
            print(json.dumps({"lib": args.label, "case": case, "streams": n, "frames": frames, "reps": args.reps, "calls": args.calls,
                              "us_per_call_median": round(float(np.median(t)), 3), "us_p25": round(float(np.percentile(t, 25)), 3),
                              "us_p75": round(float(np.percentile(t, 75)), 3), "gathered": gathered, "kernels": kernels, "digest": digest}), flush=True)
            for r in rs:
                r.close()
            del x, y


def run_child(args, label, lib, env_extra):
    env = dict(os.environ, **env_extra)
    if lib:
        env["ARTAMD_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--label", label, "--sizes", args.sizes, "--cases", args.cases,
           "--reps", str(args.reps), "--calls", str(args.calls), "--max-bytes", str(args.max_bytes)]
    return subprocess.run(cmd, env=env, timeout=args.child_seconds).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", help="libartamd.so of another build (the parent commit): the baseline column")
    ap.add_argument("--sizes", default="1,2,4,8,16,64,256")
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--max-bytes", type=float, default=8e9, help="skip a size whose buffers would exceed this")
    ap.add_argument("--child-seconds", type=float, default=500.0)
    ap.add_argument("--columns", default="before,singles,grouped")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--label", default="grouped")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    props = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": props.name, "gcn_arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
                      "argv": sys.argv[1:]}), flush=True)
    rc = 0
    for col in args.columns.split(","):
        if col == "before" and args.before:
            rc |= run_child(args, "before", args.before, {})
        elif col == "singles":
            rc |= run_child(args, "singles", None, {"ARTAMD_BATCH_MATRIX": "0"})
        elif col == "grouped":
            rc |= run_child(args, "grouped", None, {})
    return rc


if __name__ == "__main__":
    sys.exit(main())
