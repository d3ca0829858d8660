"""Host time of the clip classes: every call builds its argument arrays in Python in front of an asynchronous launch, and on short clips
that is what a call costs.  B stereo clips of 2,048 frames through each of the six classes (forward), and forward plus backward
(y.sum().backward()) through the five differentiable ones.

    python tools/bench_clip_host.py [--api PATH[=LABEL]]... [--calls 101] [--out profiles/api_host.txt]

--api PATH loads that api.py in place of the package's (--api package: the package's own), on the package's built libraries; given more
than once the versions are timed one after the other in this one process, so that they meet the same kernels, the same loaded runtime
and the same threads: `--api old.py=parent-1 --api old.py=parent-2 --api package=branch` is a version against its parent, run twice.
--out appends.  Per case: median wall-clock milliseconds per call between two synchronisations, after warm-up, with the 25th and 75th
percentile, over 101 calls: at B = 1 fifteen calls last 5 ms, less than the stretches over which a backward pass runs 0.1 ms slower
or faster (its thread's wake-up), and their median is whichever stretch they fell into.  A version is no slower than another, run
twice, if in every case its median is not above the larger of the other's two 75th percentiles.
"""
import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

FRAMES, CH, RATE = 2048, 2, 44100
BATCHES = (1, 64, 1024)


def load_api(path):
    if not path or path == "package":
        import audio_resampler_amd.api as api
        return api
    pkg = os.path.join(ROOT, "audio_resampler_amd")
    os.environ.setdefault("ARTAMD_LIB", os.path.join(pkg, "libartamd.so"))
    os.environ.setdefault("ARTAMD_LIB64", os.path.join(pkg, "libartamd64.so"))
    spec = importlib.util.spec_from_file_location("api_under_test", path)
    api = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(api)
    return api


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


def cases(A):
    """name -> (constructor, call(obj, x) -> the tensor to differentiate, differentiable)"""
    sections = [("lowpass", 0.1), ("highpass", 0.01)]
    return {
        "ClipResampler": (lambda: A.ClipResampler(CH, RATE, 16000), lambda o, x: o(x)[0], True),
        "ClipWarper": (lambda: A.ClipWarper(CH), lambda o, x: o(x, 0.75)[0], True),
        "ClipDecimator": (lambda: A.ClipDecimator(CH, 16, 2, 1.0, RATE, A.DITHER_HIGHPASS | A.SHAPING_ATH_CURVE), lambda o, x: o(x)[0], False),
        "ClipFilter": (lambda: A.ClipFilter(CH, sections), lambda o, x: o(x), True),
        "ClipBiquad": (lambda: A.ClipBiquad(CH, A.ClipBiquad.design(sections)), lambda o, x: o(x), True),
        "ClipStretcher": (lambda: A.ClipStretcher(CH, RATE), lambda o, x: o(x, 1.25)[0], True),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--api", action="append", default=None)
    ap.add_argument("--calls", type=int, default=101)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batches", default=",".join(str(b) for b in BATCHES))
    a = ap.parse_args()
    lines = ["# device: " + torch.cuda.get_device_name(0)]
    for spec in a.api or ["package"]:
        path, _, label = spec.partition("=")
        A = load_api(path)
        lines.append(f"# {label or path}: [median, 25th, 75th percentile] ms per call, {CH} channels x {FRAMES} frames per clip")
        print(lines[-1], flush=True)
        for name, (make, call, differentiable) in cases(A).items():
            for B in [int(v) for v in a.batches.split(",")]:
                obj = make()
                x = torch.randn(B, CH, FRAMES, device="cuda") * 0.25
                r = dict(case=name, B=B, forward=timed(lambda: call(obj, x), a.calls))      # (ClipFilter: in place, over and over)
                if differentiable:
                    xg = x.clone().requires_grad_()

                    def both():
                        xg.grad = None
                        call(obj, xg).sum().backward()

                    r["forward_backward"] = timed(both, a.calls)
                obj.close()
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
