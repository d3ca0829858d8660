#!/usr/bin/env python3
"""End-point LPC extrapolation: device time of artamdExtrapolateBatchDevice against the host cost of the same fits, and the first call +
flush of an extrapolating ART-form stream (8 channels, 988 taps, tonal input).

    python tools/bench_extrapolate.py [--before ROOT] [--reps 5]

- device: counts 494 and 987, white noise / two sines / low sine + faint noise, n = 1, 8, 64, 512 runs per launch (backward runs, T - count
  extras each, as the resampler's prefill makes them); the median of --reps launches, after one warm-up, timed with HIP events;
- host: the same fit, one run, on one core, as the reference's extrapolate_forward (oracle/_ref/libartref_strict.so, where it was built);
- stream: wall time of the first call (its prefill fits) and of the flush (its forward fits) of an 8-channel 988-tap fixed-ratio
  EXTRAPOLATE_ENDPOINTS stream, synchronised, for this tree and, with --before ROOT, for the library of another checkout (ROOT), each in a
  child process of its own.
Prints one JSON line per measurement."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STREAM_CHILD = r'''
import sys, time, json
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import audio_resampler_amd as A
ch, T = 8, 988
rng = np.random.default_rng(1)
n = np.arange(40000)[:, None]
f = rng.uniform(0.001, 0.05, (1, ch))
x = (0.5 * np.sin(2 * np.pi * f * n) + 0.2 * np.sin(2 * np.pi * 3.1 * f * n) + 1e-4 * rng.standard_normal((40000, ch))).astype(np.float32)
d_in = torch.from_numpy(x).cuda(); d_out = torch.zeros(60000, ch, device="cuda")
res = {}
for rep in range(4):
    r = A.Resampler(ch, T, T, 0.0, A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.INCLUDE_LOWPASS | A.EXTRAPOLATE_ENDPOINTS, fixed=(44100.0, 48000.0, 0))
    r.advance(T / 2)
    torch.cuda.synchronize()
    t0 = time.perf_counter(); u, g = r.process_device(d_in, 4096, d_out, 8000, 48000 / 44100); torch.cuda.synchronize(); t1 = time.perf_counter()
    u2, g2 = r.process_device(d_in[4096:], 16384, d_out, 30000, 48000 / 44100); torch.cuda.synchronize(); t2 = time.perf_counter()
    u3, g3 = r.process_device(None, -1, d_out, 30000, 48000 / 44100); torch.cuda.synchronize(); t3 = time.perf_counter()
    if rep:                                # (the first context pays for the library's one-time setup)
        res.setdefault("first_call_ms", []).append((t1 - t0) * 1e3); res.setdefault("ordinary_call_ms", []).append((t2 - t1) * 1e3)
        res.setdefault("flush_ms", []).append((t3 - t2) * 1e3)
    r.close()
print(json.dumps({k: float(np.median(v)) for k, v in res.items()}))
'''


def device_runs(torch, X, count, kind, n, reps):
    import audio_resampler_amd as A
    known = [X.signal(kind, count, 32, seed=i) for i in range(min(n, 16))]
    extras = 1024 - count
    d_in = torch.from_numpy(np.concatenate([known[i % len(known)] for i in range(n)])).cuda()
    d_out = torch.zeros(n * extras, device="cuda")
    ins = [d_in.data_ptr() + 4 * count * i for i in range(n)]
    outs = [d_out.data_ptr() + 4 * extras * i for i in range(n)]
    call = lambda: A.extrapolate_batch_device(ins, [count] * n, [1] * n, [1] * n, outs, [extras] * n)
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); call(); b.record(); b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def host_fit(X, count, kind):
    if not X.ref_available(32):
        return None
    R = X.RefExtrapolator(32)
    known = X.signal(kind, count, 32)
    t0 = time.perf_counter()
    R.run(known, 1024 - count, True)
    return (time.perf_counter() - t0) * 1e3


def stream(root):
    p = subprocess.run([sys.executable, "-c", STREAM_CHILD, root], capture_output=True, text=True, timeout=600)
    if p.returncode:
        return {"error": p.stderr[-400:]}
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", help="another checkout (its built library) for the stream's before / after")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import _extrapolate as X
    props = torch.cuda.get_device_properties(0)
    print(json.dumps({"device": props.name, "gcn_arch": getattr(props, "gcnArchName", ""), "cus": props.multi_processor_count}), flush=True)
    for count in (494, 987):
        for kind in ("white", "two_sines", "low_sine"):
            host = host_fit(X, count, kind)
            for n in (1, 8, 64, 512):
                ms = device_runs(torch, X, count, kind, n, args.reps)
                print(json.dumps({"count": count, "signal": kind, "runs": n, "launch_ms": round(ms, 4), "per_fit_ms": round(ms / n, 5),
                                  "host_fit_ms": None if host is None else round(host, 4)}), flush=True)
    print(json.dumps({"stream": "after", **stream(ROOT)}), flush=True)
    if args.before:
        print(json.dumps({"stream": "before", **stream(os.path.abspath(args.before))}), flush=True)


if __name__ == "__main__":
    main()
