"""Many streams quantised to PCM on one GPU: N independent decimator contexts, 441-frame blocks (10 ms at 44.1 kHz), 16-bit output,
device-resident.  One call per context per tick (decimateProcessInterleavedLEDevice in a loop) next to one batched call per tick
(decimateProcessBatchInterleavedLEDevice).  Prints one JSON line per case: ms per tick, aggregate Msamples/s and how many real-time
streams that sustains (at 48 kHz output).

    python tools/bench_decimate_batch.py            # the table: N x {stereo, 8-channel} ATH + high-pass dither, one unshaped case,
                                                    # and resample batch -> decimate batch end to end
    python tools/bench_decimate_batch.py --sweep    # lanes per workgroup of the serial kernel, fixed (the rule's measurements):
                                                    # [median, 25th, 75th percentile] ms per tick for each L and for the rule
    python tools/bench_decimate_batch.py --trace    # a few batched ticks only (for a kernel trace)
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import audio_resampler_amd as A  # noqa: E402

B = A.binding(32)
L = B.lib()
L.artamd_decimate_batch.restype = C.c_int          # library-private: the batch call with a fixed lane count (0: the rule)
L.artamd_decimate_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
BLOCK, RATE = 441, 48000
ATH = A.DITHER_HIGHPASS | A.SHAPING_ATH_CURVE      # the -o16 defaults of the command-line tool


class Case:
    def __init__(self, n, ch, flags, frames=BLOCK):
        self.n, self.ch, self.frames = n, ch, frames
        self.decs = [B.Decimator(ch, 16, 2, 1.0, RATE, flags) for _ in range(n)]
        self.x = (torch.rand(n, frames * ch, device="cuda") * 2 - 1) * 0.9
        self.out = torch.zeros(n, frames * ch * 2, dtype=torch.uint8, device="cuda")
        # argument arrays built once: the ticks time the library, not ctypes
        self.ctx = (C.c_void_p * n)(*[C.cast(d.p, C.c_void_p) for d in self.decs])
        self.ins = (C.c_void_p * n)(*[self.x[i].data_ptr() for i in range(n)])
        self.outs = (C.c_void_p * n)(*[self.out[i].data_ptr() for i in range(n)])
        self.nin = (C.c_int * n)(*([frames] * n))
        self.single = [(d.p, self.x[i].data_ptr(), frames, self.out[i].data_ptr()) for i, d in enumerate(self.decs)]

    def loop(self):
        for a in self.single:
            L.decimateProcessInterleavedLEDevice(*a)

    def batch(self, lanes=0):
        rc = L.artamd_decimate_batch(self.ctx, self.n, self.ins, self.nin, self.outs, lanes)
        assert rc >= 1, rc

    def close(self):
        for d in self.decs:
            d.close()


def tick_times(fn, ticks, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(ticks):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return np.array(t)


def per_tick(fn, ticks, warm=3):
    return float(np.median(tick_times(fn, ticks, warm)))


def row_for(case, name, loop=True):
    row = {"case": name, "streams": case.n, "channels": case.ch, "block_frames": case.frames}
    modes = (("loop", case.loop), ("batch", case.batch)) if loop else (("batch", case.batch),)
    for mode, fn in modes:
        dt = per_tick(fn, 40 if mode == "batch" or case.n <= 1024 else 8)
        samples = case.n * case.ch * case.frames
        row[mode + "_ms_per_tick"] = round(dt * 1e3, 4)
        row[mode + "_Msamples_per_s"] = round(samples / dt / 1e6, 1)
        row[mode + "_realtime_streams"] = int(case.n * case.frames / dt / RATE)
    if loop:
        row["speedup"] = round(row["loop_ms_per_tick"] / row["batch_ms_per_tick"], 1)
    print(json.dumps(row), flush=True)


def end_to_end(n):
    """resampleProcessBatchInterleavedDevice (stereo 44.1 -> 48 kHz, 380 taps) then the decimator batch on its outputs"""
    src, dst, ch, T = 44100, 48000, 2, 380
    rs = [B.Resampler(ch, T, T, 0.0, A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE) for _ in range(n)]
    for r in rs:
        r.advance(T / 2)
    decs = [B.Decimator(ch, 16, 2, 1.0, dst, ATH) for _ in range(n)]
    x = torch.from_numpy((np.random.default_rng(1).random((BLOCK, ch)) - 0.5).astype(np.float32)).cuda()
    cap = int(BLOCK * dst / src * 1.01) + 16
    y = torch.zeros(n, cap * ch, device="cuda")
    pcm = torch.zeros(n, cap * ch * 2, dtype=torch.uint8, device="cuda")
    ratios = [dst / src * (1 + 1e-5 * ((i * 7) % 11 - 5)) for i in range(n)]
    rctx = (C.c_void_p * n)(*[C.cast(r.p, C.c_void_p) for r in rs])
    dctx = (C.c_void_p * n)(*[C.cast(d.p, C.c_void_p) for d in decs])
    ins = (C.c_void_p * n)(*([x.data_ptr()] * n))
    ys = (C.c_void_p * n)(*[y[i].data_ptr() for i in range(n)])
    pcms = (C.c_void_p * n)(*[pcm[i].data_ptr() for i in range(n)])
    nin, caps, rat = (C.c_int * n)(*([BLOCK] * n)), (C.c_int * n)(*([cap] * n)), (C.c_double * n)(*ratios)
    res, made = (B.ResampleResult * n)(), (C.c_int * n)()
    gen = [0]

    def tick():
        assert L.resampleProcessBatchInterleavedDevice(rctx, n, ins, nin, ys, caps, rat, res) == 0
        for i in range(n):
            made[i] = res[i].output_generated
        assert L.decimateProcessBatchInterleavedLEDevice(dctx, n, ys, made, pcms) >= 1
        gen[0] = sum(made)

    dt = per_tick(tick, 40)
    row = {"case": "resample_then_decimate", "streams": n, "channels": ch, "block_frames": BLOCK, "taps": T,
           "ms_per_tick": round(dt * 1e3, 4), "Msamples_per_s": round(gen[0] * ch / dt / 1e6, 1),
           "realtime_streams": int(gen[0] / dt / dst)}
    print(json.dumps(row), flush=True)
    for r in rs:
        r.close()
    for d in decs:
        d.close()


def main():
    if "--trace" in sys.argv:            # 5 ticks of 1,024 ATH-shaped and 1,024 unshaped stereo streams: two classes, one launch each
        a, b = Case(1024, 2, ATH), Case(1024, 2, A.DITHER_HIGHPASS)
        n = a.n + b.n
        ctx = (C.c_void_p * n)(*a.ctx, *b.ctx)
        ins, outs = (C.c_void_p * n)(*a.ins, *b.ins), (C.c_void_p * n)(*a.outs, *b.outs)
        nin = (C.c_int * n)(*a.nin, *b.nin)
        for _ in range(5):
            assert L.decimateProcessBatchInterleavedLEDevice(ctx, n, ins, nin, outs) == 2
        torch.cuda.synchronize()
        a.close()
        b.close()
        return
    if "--sweep" in sys.argv:
        for n, ch in ((16, 2), (128, 2), (1024, 2), (1024, 8), (8192, 2)):
            c = Case(n, ch, ATH)
            row = {"case": "lanes_sweep", "streams": n, "channels": ch, "lanes_total": n * ch,
                   "rule_lanes": L.arthip_decimate_batch_lanes(n * ch)}
            # the lane counts take turns, 5 rounds of 40 ticks each: a slow stretch of the box lands on all of them alike.  Median
            # and the 25th / 75th percentiles of the 200 ticks, ms
            t = {lanes: [] for lanes in (1, 2, 4, 8, 16, 32, 64, 0)}
            for _ in range(5):
                for lanes in t:
                    t[lanes].extend(tick_times(lambda: c.batch(lanes), 40))
            for lanes, v in t.items():
                q = np.percentile(np.array(v) * 1e3, [25, 50, 75])
                row["rule" if lanes == 0 else f"L{lanes}"] = [round(float(q[1]), 4), round(float(q[0]), 4), round(float(q[2]), 4)]
            print(json.dumps(row), flush=True)
            c.close()
        return
    for n in (16, 128, 1024, 8192):
        for ch in (2, 8):
            c = Case(n, ch, ATH)
            row_for(c, "ath_highpass")
            c.close()
        c = Case(n, 2, A.DITHER_HIGHPASS)
        row_for(c, "unshaped_highpass")
        c.close()
    for n in (16, 128, 1024, 8192):
        end_to_end(n)


if __name__ == "__main__":
    main()
