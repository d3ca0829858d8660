"""Channels-first clips quantised to PCM: decimateProcessBatchPlanarLEDevice on [N, C, T] float rows against the two routes it
replaces or approaches, in one session, routes taking turns.

    planar   this tree's planar batch entry on the tensor's own rows -> [N, C, T * bytes]
    a        the route before the planar entry: transpose().contiguous(), decimateProcessBatchInterleavedLEDevice, the byte transpose
             back.  --parent-lib PATH takes that call from another build of the library (the commit before this entry existed);
             without it, from this tree's (whose interleaved kernels are the same code)
    b        this tree's interleaved batch alone on data transposed beforehand: the floor planar addressing may approach

Stereo, 16-bit; 441-frame ticks and 4,000-frame clips; high-pass dither + ATH shaping (the serial class) and high-pass dither alone
(the time-parallel class); N = 1, 64, 1,024, 8,192.  Then one single call of 8 channels x 1M frames, unshaped: planar against
interleaved (decimate_parallel_kernel), and the two mixed forms (one side planar, the other interleaved).  One JSON line per case: [median, 25th, 75th percentile] ms per call over 35 calls per route
after a warm-up, twice: X_ms is the wall clock around call + synchronise, X_gpu_ms the time between two events on the stream
around the call (the device's share: the host's work before the first launch is not in it).

The routes are treated alike: every buffer is allocated and every pointer table is built once, before the clock starts; a timed
call is the library call plus, for route a, the two transposes (copy_ into buffers that exist).

    python tools/bench_decimate_planar.py [--parent-lib PATH] [--quick]
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
RATE, BITS, NB, CH = 48000, 16, 2, 2
ATH = A.DITHER_HIGHPASS | A.SHAPING_ATH_CURVE


def parent_library(path):
    if not path:
        return L
    P = C.CDLL(path)
    for name in ("decimateInit", "decimateFree", "decimateProcessBatchInterleavedLEDevice"):
        getattr(P, name).restype, getattr(P, name).argtypes = B.EXPORTED_SYMBOLS[name]
    return P


def quartiles(times):
    q = np.percentile(np.array(times) * 1e3, [50, 25, 75])
    return [round(float(v), 4) for v in q]


def take_turns(routes, turns=5, ticks=7, warm=3):
    """every route `warm` calls, then `turns` rounds of `ticks` timed calls each, the routes taking turns: a slow stretch of the
    machine lands on all of them alike.  Route X gives X_ms (wall clock) and X_gpu_ms (events; every context here is on the
    null stream, which is torch's current one)"""
    for fn in routes.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in routes}
    g = {k: [] for k in routes}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(turns):
        for k, fn in routes.items():
            for _ in range(ticks):
                t0 = time.perf_counter()
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                t[k].append(time.perf_counter() - t0)
                g[k].append(e0.elapsed_time(e1) * 1e-3)
    row = {k + "_ms": quartiles(v) for k, v in t.items()}
    row.update({k + "_gpu_ms": quartiles(v) for k, v in g.items()})
    return row


def batch_case(P, n, frames, flags, name):
    x = (torch.rand(n, CH, frames, device="cuda") * 2 - 1) * 0.9
    xt = x.transpose(1, 2).contiguous()
    pcm = torch.zeros(n, CH, frames * NB, dtype=torch.uint8, device="cuda")
    out_b = torch.zeros(n, frames * CH * NB, dtype=torch.uint8, device="cuda")
    decs = {k: [B.Decimator(CH, BITS, NB, 1.0, RATE, flags) for _ in range(n)] for k in ("planar", "b")}
    pa = [P.decimateInit(CH, BITS, NB, 1.0, RATE, flags) for _ in range(n)]
    ctx = {k: (C.c_void_p * n)(*[C.cast(d.p, C.c_void_p) for d in v]) for k, v in decs.items()}
    ctx["a"] = (C.c_void_p * n)(*[C.cast(p, C.c_void_p) for p in pa])
    nin = (C.c_int * n)(*([frames] * n))
    ins = (C.c_void_p * n)(*[x[i].data_ptr() for i in range(n)])
    outs = (C.c_void_p * n)(*[pcm[i].data_ptr() for i in range(n)])
    ip, op = (C.c_long * n)(*([x.stride(1)] * n)), (C.c_long * n)(*([pcm.stride(1)] * n))
    ins_t = (C.c_void_p * n)(*[xt[i].data_ptr() for i in range(n)])
    outs_b = (C.c_void_p * n)(*[out_b[i].data_ptr() for i in range(n)])

    def planar():
        assert L.decimateProcessBatchPlanarLEDevice(ctx["planar"], n, ins, ip, nin, outs, op) >= 1

    # route a's buffers and tables, like the other routes' made once: the transposed input, the interleaved bytes, the result
    t_a = torch.empty(n, frames, CH, device="cuda")
    o_a = torch.empty(n, frames, CH, NB, dtype=torch.uint8, device="cuda")
    pcm_a = torch.empty(n, CH, frames, NB, dtype=torch.uint8, device="cuda")
    x_t, o_a_t = x.transpose(1, 2), o_a.permute(0, 2, 1, 3)
    ins_a = (C.c_void_p * n)(*[t_a[i].data_ptr() for i in range(n)])
    outs_a = (C.c_void_p * n)(*[o_a[i].data_ptr() for i in range(n)])

    def route_a():
        t_a.copy_(x_t)
        assert P.decimateProcessBatchInterleavedLEDevice(ctx["a"], n, ins_a, nin, outs_a) >= 1
        pcm_a.copy_(o_a_t)

    def route_b():
        assert L.decimateProcessBatchInterleavedLEDevice(ctx["b"], n, ins_t, nin, outs_b) >= 1

    row = {"case": name, "clips": n, "channels": CH, "frames": frames}
    row.update(take_turns({"planar": planar, "a": route_a, "b": route_b}))
    for sfx in ("_ms", "_gpu_ms"):
        row["a_over_planar" + sfx[:-3]] = round(row["a" + sfx][0] / row["planar" + sfx][0], 2)
        row["planar_over_b" + sfx[:-3]] = round(row["planar" + sfx][0] / row["b" + sfx][0], 2)
    print(json.dumps(row), flush=True)
    for v in decs.values():
        for d in v:
            d.close()
    for p in pa:
        P.decimateFree(p)


def single_case():
    ch, frames = 8, 1 << 20
    x = (torch.rand(ch, frames, device="cuda") * 2 - 1) * 0.9
    xt = x.t().contiguous()
    pcm = torch.zeros(ch, frames * NB, dtype=torch.uint8, device="cuda")
    out = torch.zeros(frames * ch * NB, dtype=torch.uint8, device="cuda")
    dp, di = B.Decimator(ch, BITS, NB, 1.0, RATE, A.DITHER_HIGHPASS), B.Decimator(ch, BITS, NB, 1.0, RATE, A.DITHER_HIGHPASS)
    row = {"case": "single_8ch_1M_unshaped", "channels": ch, "frames": frames}
    dm = [B.Decimator(ch, BITS, NB, 1.0, RATE, A.DITHER_HIGHPASS) for _ in range(2)]       # mixed sides: one planar, one interleaved
    row.update(take_turns({"planar": lambda: dp.process_planar_device(x, frames, frames, pcm, frames * NB),
                           "interleaved": lambda: di.process_device(xt, frames, out),
                           "planar_in_only": lambda: dm[0].process_planar_device(x, frames, frames, out, 0),
                           "planar_out_only": lambda: dm[1].process_planar_device(xt, 0, frames, pcm, frames * NB)}))
    for d in dm:
        d.close()
    for k in ("planar", "interleaved", "planar_in_only", "planar_out_only"):
        row[k + "_Gsamples_per_s"] = round(ch * frames / row[k + "_ms"][0] / 1e6, 1)
        row[k + "_gpu_Gsamples_per_s"] = round(ch * frames / row[k + "_gpu_ms"][0] / 1e6, 1)
    print(json.dumps(row), flush=True)
    dp.close(); di.close()


def main():
    path = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    P = parent_library(path)
    print(json.dumps({"parent_lib": path or "(this tree's library)", "device": torch.cuda.get_device_name(0)}), flush=True)
    counts = (1, 64, 1024) if "--quick" in sys.argv else (1, 64, 1024, 8192)
    for frames in (441, 4000):
        for flags, name in ((ATH, "serial_ath_highpass"), (A.DITHER_HIGHPASS, "parallel_unshaped_highpass")):
            for n in counts:
                batch_case(P, n, frames, flags, name)
    single_case()


if __name__ == "__main__":
    main()
