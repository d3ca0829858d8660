#!/usr/bin/env python3
"""Many whole clips converted on one GPU: N clips of a few thousand frames, 44.1 -> 16 kHz, each reset -> process -> flush.  The loop of
resampleProcessAndFlushInterleavedDevice calls next to ONE resampleProcessAndFlushBatchInterleavedDevice call.

    python tools/bench_flush_batch.py [--before LIB] [--sizes 64,1024,8192] [--frames 4000] [--reps 5] [--loop-seconds 60]

Shapes: stereo x 380 taps and 8 channels x 988 taps, with and without EXTRAPOLATE_ENDPOINTS.  Tonal input (a sum of a few sines and a
little noise per clip: the LPC fits end early on noise and would flatter the result).  Every repetition re-arms the contexts
(resampleReset, advance by T/2) outside the timed window, which is the wall clock around the calls and a final synchronise of the
stream.  Medians with the 25th and 75th percentile over --reps repetitions after one warm-up.
Three columns, each measured in a child process of its own so that one library is loaded per process: the loop with the library of
--before (another build's libartamd.so: the parent commit's), the loop with this tree's library, the batched call with this tree's.
A loop of extrapolating clips is serial on its stream and costs two rounds of LPC fits per clip, some tenths of a second: a case whose
first (warm-up) repetition shows that --reps repetitions would exceed --loop-seconds is timed with fewer repetitions (3, or one), and a
case that the next smaller size's time per clip predicts to exceed --loop-seconds in ONE repetition is not run at all
("skipped": the predicted seconds; the loop's time per clip does not depend on N).
Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"stereo_380": (2, 380), "eight_988": (8, 988)}
RATIO = 16000 / 44100


def tonal(frames, ch, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    n = np.arange(frames)[:, None]
    f = rng.uniform(0.001, 0.05, (1, ch))
    x = 0.5 * np.sin(2 * np.pi * f * n + rng.uniform(0, 6.3, (1, ch))) + 0.2 * np.sin(2 * np.pi * 3.1 * f * n)
    return np.ascontiguousarray((x + 1e-4 * rng.standard_normal((frames, ch))).astype(np.float32))


def child(args):
    """one library (ARTAMD_LIB, set by the parent), every case of the list, the modes asked for"""
    import ctypes as C
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import audio_resampler_amd as A
    B = A.binding(32)
    if "batched" not in args.modes:          # (a library from before the batched entry existed: the loop needs the single call only)
        B.EXPORTED_SYMBOLS.pop("resampleProcessAndFlushBatchInterleavedDevice", None)
    L = B.lib()
    per_clip = {}                            # (shape, extrapolate, mode) -> seconds per clip at the last size measured
    for shape in args.shapes.split(","):
        ch, T = SHAPES[shape]
        for extrap in (0, 1):
            flags = A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | (A.EXTRAPOLATE_ENDPOINTS if extrap else 0)
            for n in [int(v) for v in args.sizes.split(",")]:
                rs = [B.Resampler(ch, T, T, 0.0, flags) for _ in range(n)]
                # clip i = frames [i, i + frames) of one signal: every clip ends on other samples (other fits), one upload
                base = torch.from_numpy(tonal(args.frames + n, ch, seed=n + ch)).cuda()
                cap = int(args.frames * RATIO) + T
                out = torch.zeros(n, cap, ch, device="cuda")
                ins = [base.data_ptr() + 4 * ch * i for i in range(n)]
                outs = [out[i].data_ptr() for i in range(n)]
                ctx = (C.c_void_p * n)(*[C.cast(r.p, C.c_void_p) for r in rs])
                a_in, a_out = (C.c_void_p * n)(*ins), (C.c_void_p * n)(*outs)
                a_n, a_cap, a_ratio = (C.c_int * n)(*([args.frames] * n)), (C.c_int * n)(*([cap] * n)), (C.c_double * n)(*([RATIO] * n))
                res = (B.ResampleResult * n)()

                def arm():
                    for r in rs:
                        r.reset(); r.advance(T / 2)
                    torch.cuda.synchronize()

                def loop():
                    for i, r in enumerate(rs):
                        res[i] = L.resampleProcessAndFlushInterleavedDevice(r.p, ins[i], args.frames, outs[i], cap, RATIO)

                def batched():
                    assert L.resampleProcessAndFlushBatchInterleavedDevice(ctx, n, a_in, a_n, a_out, a_cap, a_ratio, res) == 0

                for mode in args.modes.split(","):
                    fn = loop if mode == "loop" else batched
                    predicted = per_clip.get((shape, extrap, mode), 0.0) * n
                    if predicted > args.loop_seconds:
                        print(json.dumps({"lib": args.label, "mode": mode, "shape": shape, "extrapolate": extrap, "clips": n, "frames": args.frames,
                                          "skipped": round(predicted, 1)}), flush=True)
                        continue
                    arm()
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); warm = time.perf_counter() - t0
                    reps = args.reps if warm * args.reps <= args.loop_seconds else 3 if warm * 3 <= args.loop_seconds else 1 if warm <= args.loop_seconds else 0
                    times = []
                    for _ in range(reps):
                        arm()
                        t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times.append(time.perf_counter() - t0)
                    t = np.array(times if times else [warm]) * 1e3
                    per_clip [(shape, extrap, mode)] = float(np.median(t)) * 1e-3 / n
                    made = sum(res[i].output_generated for i in range(n))
                    digest = int(out.view(torch.int32).to(torch.int64).sum().item())
                    print(json.dumps({"lib": args.label, "mode": mode, "shape": shape, "extrapolate": extrap, "clips": n, "frames": args.frames,
                                      "reps": reps, "ms_median": round(float(np.median(t)), 3), "ms_p25": round(float(np.percentile(t, 25)), 3),
                                      "ms_p75": round(float(np.percentile(t, 75)), 3), "ms_per_clip": round(float(np.median(t)) / n, 4),
                                      "outputs": made, "digest": digest}), flush=True)
                for r in rs:
                    r.close()
                del base, out


def run_child(args, label, lib, modes):
    env = dict(os.environ)
    if lib:
        env["ARTAMD_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--label", label, "--modes", modes, "--sizes", args.sizes, "--shapes", args.shapes,
           "--frames", str(args.frames), "--reps", str(args.reps), "--loop-seconds", str(args.loop_seconds)]
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", help="libartamd.so of another build (the parent commit): its loop is the baseline column")
    ap.add_argument("--sizes", default="64,1024,8192")
    ap.add_argument("--shapes", default="stereo_380,eight_988")
    ap.add_argument("--frames", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-seconds", type=float, default=60.0)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--label", default="this")
    ap.add_argument("--modes", default="loop,batched")
    args = ap.parse_args()
    if args.child:
        return child(args)
    import torch
    props = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": props.name, "gcn_arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count,
                      "argv": sys.argv[1:]}), flush=True)
    rc = 0
    if args.before:
        rc |= run_child(args, "before", args.before, "loop")
    rc |= run_child(args, "this", None, "loop,batched")
    return rc


if __name__ == "__main__":
    sys.exit(main())
