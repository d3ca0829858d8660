"""artamdLagProductsBatchDevice next to the torch expression for the same nine sums, and one ClipBiquad training step.

    python tools/micro/bench_clip_biquad.py [--reps 20] [--out FILE]

Per shape (B clips, C channels, T frames, 4-byte samples): every plane is two rows of the call, (u, v, lags 0..4) and (u, v, lags
1..4) — the nine sums of one section's coefficient gradient — so a call reads 2 * 2 * B * C * T samples.  `kernel_ms`: device-event
time per call (table upload and both launches) over `reps` back-to-back calls after warm-up, median of five such windows, with the
lowest and highest; `GB_per_s`: those bytes over it.  `torch_ms`: the same nine sums as
(u[..., k:] * v[..., :T - k]).sum(-1, dtype=torch.float64), timed the same way.  `max_rel_diff`: the two results against each other.
Then, for the first shape and two sections, the wall time of one ClipBiquad forward + backward step between two synchronisations.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import audio_resampler_amd as A  # noqa: E402

SHAPES = ((64, 2, 160_000), (1, 2, 4_000_000), (2048, 1, 700))
LAGS = ((0, 5), (1, 4))


def windows(fn, reps, count=5):
    """ms per call: [median, lowest, highest] of `count` windows of `reps` calls between two device events"""
    for _ in range(3):
        fn()
    out = []
    for _ in range(count):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return [round(float(v), 4) for v in (np.median(out), min(out), max(out))]


def lag_case(B, Cn, T, reps):
    g = torch.Generator(device="cuda").manual_seed(B + T)
    u = torch.rand(B, Cn, T, generator=g, device="cuda") * 2 - 1
    v = torch.rand(B, Cn, T, generator=g, device="cuda") * 2 - 1
    sums = torch.zeros(B, Cn, 9, dtype=torch.float64, device="cuda")
    planes = np.arange(B * Cn, dtype=np.int64)
    up, vp, sp = u.data_ptr() + planes * T * 4, v.data_ptr() + planes * T * 4, sums.data_ptr() + planes * 9 * 8
    n = len(planes)
    args = (np.concatenate([up, up]), np.concatenate([vp, vp]), [T] * (2 * n), [0] * n + [1] * n, [5] * n + [4] * n,
            np.concatenate([sp, sp + 5 * 8]))
    stream = torch.cuda.current_stream()

    def kernel():
        return A.lag_products_batch_device(*args, stream=stream)

    def expression():
        return torch.stack([(u[..., k:] * v[..., :T - k]).sum(-1, dtype=torch.float64) for f, c in LAGS for k in range(f, f + c)], dim=-1)

    launches = kernel()
    want = expression()
    torch.cuda.synchronize()
    diff = float(((sums - want).abs() / want.abs().clamp_min(1e-30)).max())
    nbytes = 2 * 2 * B * Cn * T * 4
    k_ms, t_ms = windows(kernel, reps), windows(expression, max(1, reps // 4))
    return dict(B=B, C=Cn, T=T, rows=2 * n, launches=launches, bytes_read=nbytes, kernel_ms=k_ms, GB_per_s=round(nbytes / k_ms[0] / 1e6, 1),
                torch_ms=t_ms, kernel_over_torch=round(k_ms[0] / t_ms[0], 3), max_rel_diff=diff)


def step_case(B, Cn, T, calls=7):
    out = {}
    for x_tracked in (False, True):
        co = A.ClipBiquad.design([("lowpass", 44100 * 0.45 / 96000)] * 2).requires_grad_()
        cb = A.ClipBiquad(Cn, co)
        x = (torch.randn(B, Cn, T, device="cuda") * 0.25).requires_grad_(x_tracked)
        gy = torch.randn(B, Cn, T, device="cuda")

        def step():
            co.grad = None
            cb(x).backward(gy)

        for _ in range(2):
            step()
        ms = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        out["x_tracked" if x_tracked else "coefficients_only"] = dict(
            step_ms=[round(float(q), 3) for q in np.percentile(ms, [50, 25, 75])], forward_launches=cb.launches,
            backward_launches=list(cb.backward_launches))
        cb.close()
    return dict(B=B, C=Cn, T=T, S=2, clip_biquad_step=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["# artamdLagProductsBatchDevice (kernel_ms: [median, lowest, highest] ms per call by device events) against the torch",
             "# expression for the same nine sums (torch_ms), 4-byte samples; then one ClipBiquad forward + backward step (wall ms:",
             "# [median, 25th, 75th percentile]).  device: " + torch.cuda.get_device_name(0)]
    for shape in SHAPES:
        lines.append(json.dumps(lag_case(*shape, a.reps)))
        print(lines[-1], flush=True)
    lines.append(json.dumps(step_case(*SHAPES[0])))
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
