"""Many streams' integer PCM to float on one GPU: N independent buffers per tick, device-resident.  One floatIntegersLEDevice call per
stream per tick (a loop) next to one floatIntegersBatchLEDevice call per tick.  Prints one JSON line per case: median ms per tick (a
device synchronise inside the timed region) and aggregate Msamples/s.

    python tools/bench_ingest_batch.py            # N = 16, 128, 1,024, 8,192 x {441-frame stereo 16-bit, 960-frame stereo 24-in-32}
    python tools/bench_ingest_batch.py --e2e      # a PCM-to-PCM tick (ingest, resample 44.1 -> 48 kHz, decimate to 16-bit): all
                                                  # batched against the ingest looped and the rest batched
    python tools/bench_ingest_batch.py --trace    # a few ticks only (for a kernel trace)
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
SHAPES = {"s16_441": (441, 2, 16, 2), "s24in32_960": (960, 2, 24, 4)}      # frames, channels, bits, bytes per sample


class Case:
    def __init__(self, n, shape, gain=1.0):
        self.n, self.shape = n, shape
        frames, ch, bits, nbytes = SHAPES[shape]
        self.count = frames * ch
        self.pcm = torch.randint(0, 256, (n, self.count * nbytes), dtype=torch.uint8, device="cuda")
        self.x = torch.zeros(n, self.count, device="cuda")
        # argument arrays built once: the ticks time the library, not ctypes
        self.args = ((C.c_void_p * n)(*[self.pcm[i].data_ptr() for i in range(n)]), (C.c_double * n)(*([gain] * n)),
                     (C.c_int * n)(*([bits] * n)), (C.c_int * n)(*([nbytes] * n)), (C.c_int * n)(*([1] * n)),
                     (C.c_void_p * n)(*[self.x[i].data_ptr() for i in range(n)]), (C.c_int * n)(*([self.count] * n)))
        self.single = [(self.pcm[i].data_ptr(), gain, bits, nbytes, 1, self.x[i].data_ptr(), self.count, None) for i in range(n)]

    def loop(self):
        for a in self.single:
            L.floatIntegersLEDevice(*a)

    def batch(self):
        rc = L.floatIntegersBatchLEDevice(*self.args, self.n, None)
        assert rc == 1, rc


def per_tick(fn, ticks, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(ticks):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def table():
    for n in (16, 128, 1024, 8192):
        for shape in SHAPES:
            c = Case(n, shape)
            row = {"case": "ingest", "shape": shape, "streams": n, "samples_per_stream": c.count}
            for mode, fn in (("loop", c.loop), ("batch", c.batch)):
                dt = per_tick(fn, 40 if mode == "batch" or n <= 1024 else 10)
                row[mode + "_ms_per_tick"] = round(dt * 1e3, 4)
                row[mode + "_Msamples_per_s"] = round(n * c.count / dt / 1e6, 1)
            row["speedup"] = round(row["loop_ms_per_tick"] / row["batch_ms_per_tick"], 1)
            print(json.dumps(row), flush=True)


def end_to_end(n):
    """16-bit stereo PCM in (441 frames), resampleProcessBatchInterleavedDevice 44.1 -> 48 kHz (380 taps), decimator batch to 16-bit
    PCM (ATH shaping, high-pass dither); the ingest stage looped (the best form before the batch call) or batched"""
    src, dst, ch, T, block = 44100, 48000, 2, 380, 441
    ing = Case(n, "s16_441")
    rs = [B.Resampler(ch, T, T, 0.0, A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE) for _ in range(n)]
    for r in rs:
        r.advance(T / 2)
    decs = [B.Decimator(ch, 16, 2, 1.0, dst, A.DITHER_HIGHPASS | A.SHAPING_ATH_CURVE) for _ in range(n)]
    cap = int(block * dst / src * 1.01) + 16
    y = torch.zeros(n, cap * ch, device="cuda")
    pcm = torch.zeros(n, cap * ch * 2, dtype=torch.uint8, device="cuda")
    ratios = [dst / src * (1 + 1e-5 * ((i * 7) % 11 - 5)) for i in range(n)]
    rctx = (C.c_void_p * n)(*[C.cast(r.p, C.c_void_p) for r in rs])
    dctx = (C.c_void_p * n)(*[C.cast(d.p, C.c_void_p) for d in decs])
    ins = (C.c_void_p * n)(*[ing.x[i].data_ptr() for i in range(n)])
    ys = (C.c_void_p * n)(*[y[i].data_ptr() for i in range(n)])
    pcms = (C.c_void_p * n)(*[pcm[i].data_ptr() for i in range(n)])
    nin, caps, rat = (C.c_int * n)(*([block] * n)), (C.c_int * n)(*([cap] * n)), (C.c_double * n)(*ratios)
    res, made = (B.ResampleResult * n)(), (C.c_int * n)()
    gen = [0]

    def rest():
        assert L.resampleProcessBatchInterleavedDevice(rctx, n, ins, nin, ys, caps, rat, res) == 0
        for i in range(n):
            made[i] = res[i].output_generated
        assert L.decimateProcessBatchInterleavedLEDevice(dctx, n, ys, made, pcms) >= 1
        gen[0] = sum(made)

    def tick_looped():
        ing.loop()
        rest()

    def tick_batched():
        ing.batch()
        rest()

    row = {"case": "pcm_to_pcm", "streams": n, "channels": ch, "block_frames": block, "taps": T}
    for mode, fn in (("ingest_looped", tick_looped), ("all_batched", tick_batched)):
        dt = per_tick(fn, 40 if mode == "all_batched" or n <= 1024 else 10)
        row[mode + "_ms_per_tick"] = round(dt * 1e3, 4)
        row[mode + "_Msamples_per_s"] = round(gen[0] * ch / dt / 1e6, 1)
    row["speedup"] = round(row["ingest_looped_ms_per_tick"] / row["all_batched_ms_per_tick"], 2)
    print(json.dumps(row), flush=True)
    for r in rs:
        r.close()
    for d in decs:
        d.close()


def main():
    if "--trace" in sys.argv:            # 5 batched ticks of 1,024 streams of each shape, then one looped tick of the 16-bit shape
        cases = [Case(1024, s) for s in SHAPES]
        for _ in range(5):
            for c in cases:
                c.batch()
        cases[0].loop()
        torch.cuda.synchronize()
        return
    if "--e2e" in sys.argv:
        for n in (16, 128, 1024, 8192):
            end_to_end(n)
        return
    table()


if __name__ == "__main__":
    main()
