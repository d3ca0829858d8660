"""Many streams through ART's -p biquad cascade on one GPU: N independent banks of 2 low-pass sections per channel, device-resident.
One call per bank per tick (biquadBankApplyInterleavedDevice in a loop) next to one batched call per tick
(biquadBankApplyBatchInterleavedDevice).  Prints one JSON line per case: ms per tick, aggregate Msamples/s and how many real-time
streams that sustains.

    python tools/bench_biquad_batch.py            # the table: ART's post-filter (441-frame ticks at 48 kHz, 0.4134 x fs) and pre-filter
                                                  # (960-frame ticks at 96 kHz, 0.2067 x fs), stereo and 8 channels, N = 16 .. 8,192
    python tools/bench_biquad_batch.py --sweep    # lanes per workgroup, fixed (the rule's measurements), and the frame count at which one
                                                  # serial lane takes as long as the bank's time-parallel single call (serial_max)
    python tools/bench_biquad_batch.py --e2e      # config C's shape per stream (96 -> 44.1 kHz, -p, 16-bit ATH): pre-filter, resample and
                                                  # decimate all batched, against the same tick with the pre-filter looped
    python tools/bench_biquad_batch.py --trace    # a few batched ticks only (for a kernel trace)
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
L.artamd_biquad_batch.restype = C.c_int            # library-private: the batch call with a fixed lane count and bound
L.artamd_biquad_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
L.artamd_biquad_batch_serial_max.restype = C.c_int
POST = dict(name="post_filter", cutoff=44100 * 0.45 / 48000, frames=441, rate=48000,
            parallel_from=1440)    # art -p, 44.1 -> 48 kHz (the single call is time-parallel from 2L = 2 x 720 frames)
PRE = dict(name="pre_filter", cutoff=44100 * 0.45 / 96000, frames=960, rate=96000,
           parallel_from=768)      # art -p, 96 -> 44.1 kHz (2L = 2 x 384)
NO_BOUND = 1 << 30


def sections(ch, cutoff):
    co = B.BiquadCoefficients()
    L.biquad_lowpass(C.byref(co), cutoff)
    secs = (B.Biquad * (ch * 2))()
    for i in range(ch * 2):
        L.biquad_init(C.byref(secs[i]), C.byref(co), 1.0)
    return secs


class Case:
    def __init__(self, n, ch, flt, frames=None):
        self.n, self.ch, self.flt = n, ch, flt
        self.frames = frames or flt["frames"]
        secs = sections(ch, flt["cutoff"])
        self.banks = [B.BiquadBank(secs, ch, 2) for _ in range(n)]
        self.x = (torch.rand(n, self.frames * ch, device="cuda") * 2 - 1) * 0.9
        # argument arrays built once: the ticks time the library, not ctypes
        self.ptrs = (C.c_void_p * n)(*[b.p for b in self.banks])
        self.bufs = (C.c_void_p * n)(*[self.x[i].data_ptr() for i in range(n)])
        self.nf = (C.c_int * n)(*([self.frames] * n))
        self.single = [(b.p, self.x[i].data_ptr(), self.frames) for i, b in enumerate(self.banks)]

    def loop(self):
        for a in self.single:
            L.biquadBankApplyInterleavedDevice(*a)

    def batch(self, lanes=0, serial_max=-1):
        rc = L.artamd_biquad_batch(self.ptrs, self.n, self.bufs, self.nf, lanes, serial_max)
        assert rc >= 1, rc

    def close(self):
        for b in self.banks:
            b.close()


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


def row_for(case):
    row = {"case": case.flt["name"], "streams": case.n, "channels": case.ch, "block_frames": case.frames}
    for mode, fn in (("loop", case.loop), ("batch", case.batch)):
        dt = per_tick(fn, 40 if mode == "batch" or case.n <= 1024 else 8)
        samples = case.n * case.ch * case.frames
        row[mode + "_ms_per_tick"] = round(dt * 1e3, 4)
        row[mode + "_Msamples_per_s"] = round(samples / dt / 1e6, 1)
        row[mode + "_realtime_streams"] = int(case.n * case.frames / dt / case.flt["rate"])
    row["speedup"] = round(row["loop_ms_per_tick"] / row["batch_ms_per_tick"], 1)
    if case.frames > L.artamd_biquad_batch_serial_max():
        # the calls above the bound are made on the side: what gathering them all would take (no bound)
        row["batch_no_bound_ms_per_tick"] = round(per_tick(lambda: case.batch(0, NO_BOUND), 40) * 1e3, 4)
    print(json.dumps(row), flush=True)


def sweep():
    for n, ch in ((16, 2), (128, 2), (1024, 2), (1024, 8), (8192, 2)):
        c = Case(n, ch, POST)
        row = {"case": "lanes_sweep", "filter": "post_filter", "streams": n, "channels": ch, "lanes_total": n * ch,
               "rule_lanes": L.arthip_biquad_batch_lanes(n * ch)}
        # the lane counts take turns, 5 rounds of 40 ticks each: a slow stretch of the box lands on all of them alike.  Median and
        # the 25th / 75th percentiles of the 200 ticks, ms
        t = {lanes: [] for lanes in (1, 2, 4, 8, 16, 32, 64, 0)}
        for _ in range(5):
            for lanes in t:
                t[lanes].extend(tick_times(lambda: c.batch(lanes), 40))
        for lanes, v in t.items():
            q = np.percentile(np.array(v) * 1e3, [25, 50, 75])
            row["rule" if lanes == 0 else f"L{lanes}"] = [round(float(q[1]), 4), round(float(q[0]), 4), round(float(q[2]), 4)]
        print(json.dumps(row), flush=True)
        c.close()
    # serial_max: one bank, its call gathered (a serial lane per channel, no bound) against its single call (time-parallel from 2L
    # frames on); median ms per call, the two taking turns
    for flt in (PRE, POST):
        for ch in (2, 8):
            for frames in (256, 384, 512, 640, 768, 1024, 1440, 1536, 2048, 3072, 4096, 6144, 8192):
                c = Case(1, ch, flt, frames)
                t = {"serial": [], "single": []}
                for _ in range(5):
                    t["serial"].extend(tick_times(lambda: c.batch(0, NO_BOUND), 20))
                    t["single"].extend(tick_times(c.loop, 20))
                row = {"case": "serial_max", "filter": flt["name"], "channels": ch, "frames": frames,
                       "single_form": "time_parallel" if frames >= flt["parallel_from"] else "serial",
                       "serial_lane_ms": round(float(np.median(t["serial"])) * 1e3, 4),
                       "single_call_ms": round(float(np.median(t["single"])) * 1e3, 4)}
                print(json.dumps(row), flush=True)
                c.close()


def end_to_end(n):
    """config C's shape, per stream stereo: 960 frames of 96 kHz -> -p pre-filter -> 96 -> 44.1 kHz (preset -4: 988 x 988, fixed ratio,
    implicit low-pass) -> 16-bit PCM with HP-TPDF dither + ATH shaping; every stage batched, against the pre-filter looped"""
    src, dst, ch, T, frames = 96000, 44100, 2, 988, PRE["frames"]
    flags = A.BLACKMAN_HARRIS | A.INCLUDE_LOWPASS | A.SUBSAMPLE_INTERPOLATE
    pre = Case(n, ch, PRE)
    rs = [B.Resampler(ch, T, T, 0.0, flags, fixed=(src, dst, 0)) for _ in range(n)]
    for r in rs:
        r.advance(T / 2)
    decs = [B.Decimator(ch, 16, 2, 1.0, dst, A.DITHER_HIGHPASS | A.SHAPING_ATH_CURVE) for _ in range(n)]
    cap = int(frames * dst / src * 1.01) + 16
    y = torch.zeros(n, cap * ch, device="cuda")
    pcm = torch.zeros(n, cap * ch * 2, dtype=torch.uint8, device="cuda")
    rctx = (C.c_void_p * n)(*[C.cast(r.p, C.c_void_p) for r in rs])
    dctx = (C.c_void_p * n)(*[C.cast(d.p, C.c_void_p) for d in decs])
    ys = (C.c_void_p * n)(*[y[i].data_ptr() for i in range(n)])
    pcms = (C.c_void_p * n)(*[pcm[i].data_ptr() for i in range(n)])
    caps, rat = (C.c_int * n)(*([cap] * n)), (C.c_double * n)(*([0.0] * n))
    res, made = (B.ResampleResult * n)(), (C.c_int * n)()
    gen = [0]

    def rest():
        assert L.resampleProcessBatchInterleavedDevice(rctx, n, pre.bufs, pre.nf, ys, caps, rat, res) == 0
        for i in range(n):
            made[i] = res[i].output_generated
        assert L.decimateProcessBatchInterleavedLEDevice(dctx, n, ys, made, pcms) >= 1
        gen[0] = sum(made)

    def tick_batched():
        pre.batch()
        rest()

    def tick_looped():
        pre.loop()
        rest()

    def tick_no_bound():                 # every pre-filter call gathered, whatever its length
        pre.batch(0, NO_BOUND)
        rest()

    row = {"case": "config_c_shape_end_to_end", "streams": n, "channels": ch, "block_frames": frames, "taps": T}
    for name, fn in (("prefilter_looped", tick_looped), ("all_batched", tick_batched), ("all_batched_no_bound", tick_no_bound)):
        dt = per_tick(fn, 20)
        row[name + "_ms_per_tick"] = round(dt * 1e3, 4)
        row[name + "_realtime_streams"] = int(n * frames / dt / src)
    print(json.dumps(row), flush=True)
    pre.close()
    for r in rs:
        r.close()
    for d in decs:
        d.close()


def main():
    if "--trace" in sys.argv:            # 5 ticks of 1,024 post-filter stereo banks (2 sections) + 256 one-section banks: two classes
        a = Case(1024, 2, POST)
        secs1 = (B.Biquad * 2)()
        co = B.BiquadCoefficients()
        L.biquad_lowpass(C.byref(co), POST["cutoff"])
        for i in range(2):
            L.biquad_init(C.byref(secs1[i]), C.byref(co), 1.0)
        ones = [B.BiquadBank(secs1, 2, 1) for _ in range(256)]
        x1 = torch.rand(256, POST["frames"] * 2, device="cuda")
        n = a.n + len(ones)
        ptrs = (C.c_void_p * n)(*a.ptrs, *[b.p for b in ones])
        bufs = (C.c_void_p * n)(*a.bufs, *[x1[i].data_ptr() for i in range(len(ones))])
        nf = (C.c_int * n)(*([POST["frames"]] * n))
        for _ in range(5):
            assert L.biquadBankApplyBatchInterleavedDevice(ptrs, n, bufs, nf) == 2
        torch.cuda.synchronize()
        a.close()
        for b in ones:
            b.close()
        return
    print(json.dumps({"case": "library", "serial_max": L.artamd_biquad_batch_serial_max()}), flush=True)
    if "--sweep" in sys.argv:
        sweep()
        return
    if "--e2e" in sys.argv:
        for n in (16, 128, 1024):
            end_to_end(n)
        return
    for flt in (POST, PRE):
        for n in (16, 128, 1024, 8192):
            for ch in (2, 8):
                c = Case(n, ch, flt)
                row_for(c)
                c.close()


if __name__ == "__main__":
    main()
