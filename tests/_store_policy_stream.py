"""Helper of test_gpu_store_policy.py: one small device-resident stream (3 calls of 8 ch x 20,000 frames, 988 x 988 interpolating) in THIS
process's environment (the ARTAMD_* switches are read once per process).  After every call the output buffer is read three ways: a device
copy enqueued on the call's own stream, a device copy on a second stream ordered behind an event, and a host read-back.
Usage: python _store_policy_stream.py KERNEL INF(0/1) OUT.npz  — prints one JSON line: per call the frames made, the fixed-point state and
kernel form; the three readings go to OUT.npz (host<k>, same<k>, other<k>)."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
from _hip import HipResampler
from _oracle import noise, BH, INTERP

CH, T, FRAMES, CALLS, RATIO = 8, 988, 20000, 3, 48000 / 44100
BAD_CALL, BAD_FRAME, BAD_CHANNEL = 1, 5000, 3                 # (far from the call's last T frames: the next call's history never holds it)


def main():
    kernel, inf, path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    x, _ = noise(CALLS * FRAMES * CH, state=0x57031)
    x = x.reshape(CALLS * FRAMES, CH).copy()
    if inf:
        x[BAD_CALL * FRAMES + BAD_FRAME, BAD_CHANNEL] = np.inf
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    r = HipResampler(CH, T, T, 0.0, BH | INTERP, kernel=kernel)
    r.advance(T / 2)
    r.set_stream(s1.cuda_stream)
    cap = int(FRAMES * RATIO) + 4000
    calls, arrays = [], {}
    with torch.cuda.stream(s1):
        d_out = torch.empty(cap, CH, device="cuda")
    for k in range(CALLS):
        with torch.cuda.stream(s1):
            d_in = torch.from_numpy(x[k * FRAMES:(k + 1) * FRAMES]).cuda()
            d_out.fill_(float("nan"))                           # (what a call does not write is told from what it does)
            u, g = r.process_device(d_in, FRAMES, d_out, cap, RATIO)
            assert u == FRAMES
            same = torch.empty_like(d_out)
            same.copy_(d_out, non_blocking=True)                # device copy behind the call, same stream
            ev = torch.cuda.Event()
            ev.record(s1)
        with torch.cuda.stream(s2):
            s2.wait_event(ev)
            other = torch.empty_like(d_out)
            other.copy_(d_out, non_blocking=True)               # device copy on another stream, behind the event
        with torch.cuda.stream(s1):
            host = d_out.cpu().numpy()[:g].copy()               # host read-back
        s1.synchronize(); s2.synchronize()
        arrays[f"host{k}"], arrays[f"same{k}"], arrays[f"other{k}"] = host, same.cpu().numpy()[:g].copy(), other.cpu().numpy()[:g].copy()
        calls.append({"frames": int(g), "state": int(r.fixed_point()[0]), "form": r.fixed_point_kernel()})
    np.savez(path, **arrays)
    print(json.dumps(calls))


if __name__ == "__main__":
    sys.exit(main())
