"""decimateProcessBatchInterleavedLEDevice: many decimator contexts in one launch per class of work.  Every context's bytes, clip
count and state afterwards are those of its own single device call, on a twin context, and the reference's goldens hold for every
flag combination in one batch."""
import ctypes as C
import statistics
import time

import numpy as np
import pytest
import torch

import _golden as G
import audio_resampler_amd as A
from _oracle import checksum_bytes
from test_oracle_golden import decimate_input

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GAP = 64                                        # bytes between two contexts' outputs in the shared buffer
S1, S2, S3, SATH = A.SHAPING_1ST_ORDER, A.SHAPING_2ND_ORDER, A.SHAPING_3RD_ORDER, A.SHAPING_ATH_CURVE
HP, FLAT, LP = A.DITHER_HIGHPASS, A.DITHER_FLAT, A.DITHER_LOWPASS


def _order(d):
    """the shaper order a context runs (0: no noise shaping)"""
    sh = d.p.contents.noise_shapers
    return sh[0].order if sh else 0


def _classes(decs, frames):
    """the classes of work the batch forms for these (context, frames): an upper bound of its launch count"""
    out = set()
    for d, n in zip(decs, frames):
        if n <= 0:
            continue
        dith = d.p.contents.flags & (HP | FLAT | LP) != 0
        order = _order(d)
        out.add(("parallel", dith) if n >= 64 and order == 0 else ("serial", order, dith))
    return out


class Layout:
    """every context's output in one buffer, with sentinel gaps between them"""
    def __init__(self, sizes):
        self.off, pos = [], GAP
        for s in sizes:
            self.off.append(pos)
            pos += s + GAP
        self.sizes = list(sizes)
        self.buf = torch.full((pos,), SENTINEL, dtype=torch.uint8, device="cuda")

    def ptr(self, i):
        return self.buf.data_ptr() + self.off[i]

    def part(self, host, i):
        return host[self.off[i]:self.off[i] + self.sizes[i]]

    def gaps_untouched(self, host):
        mask = np.ones(host.size, bool)
        for o, s in zip(self.off, self.sizes):
            mask[o:o + s] = False
        return bool(np.all(host[mask] == SENTINEL))


def _specs():
    chans = [1, 2, 3, 6, 8, 33, 64, 65, 130]
    fmts = [(8, 1), (12, 2), (16, 2), (16, 4), (20, 3), (24, 3), (24, 4)]
    dithers = [0, HP, FLAT, LP]
    shapes = [0, S1, S2, S3, SATH]
    frames = [0, 1, 63, 64, 65, 441, 4096, 100003]
    gains = [1.0, 0.5, 3.0]                      # 3.0 clips
    out = []
    for i in range(40):
        bits, nbytes = fmts[i % 7]
        out.append(dict(ch=chans[i % 9], bits=bits, nbytes=nbytes, flags=dithers[i % 4] | shapes[(i // 4) % 5],
                        frames=frames[i % 8], gain=gains[i % 3], rate=(44100, 48000, 96000)[i % 3]))
    return out


def _make(M, specs):
    return [M.Decimator(s["ch"], s["bits"], s["nbytes"], s["gain"], s["rate"], s["flags"]) for s in specs]


def _inputs(M, specs, call, dtype):
    g = torch.Generator(device="cuda").manual_seed(1234 + call)
    return [(torch.rand(max(s["frames"], 1) * s["ch"], generator=g, device="cuda", dtype=dtype) * 2.2 - 1.1) for s in specs]


def _with_lanes(M, lanes):
    """the batch call with every serial class packed `lanes` lanes to a workgroup (the library's private form of the call: the
    public one picks the count from the class's size, and gives one lane per workgroup to classes of up to 1,024 lanes)"""
    fn = M.lib().artamd_decimate_batch
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]

    def call(decs, xs, frames, ptrs):
        n = len(decs)
        rc = fn((C.c_void_p * n)(*[C.cast(d.p, C.c_void_p) for d in decs]), n, (C.c_void_p * n)(*[x.data_ptr() for x in xs]),
                (C.c_int * n)(*[int(f) for f in frames]), (C.c_void_p * n)(*ptrs), lanes)
        if rc < 0:
            raise RuntimeError("artamd_decimate_batch failed")
        return rc
    return call


def _mixed_batch_equals_twins(M, dtype, specs, batch_call=None):
    batch_call = batch_call or M.decimate_batch_device
    batch, twins = _make(M, specs), _make(M, specs)
    frames = [s["frames"] for s in specs]
    sizes = [s["frames"] * s["ch"] * s["nbytes"] for s in specs]
    for call in range(3):
        xs = _inputs(M, specs, call, dtype)
        lay = Layout(sizes)
        rc = batch_call(batch, xs, frames, [lay.ptr(i) for i in range(len(specs))])
        assert 1 <= rc <= len(_classes(batch, frames)), rc
        wants = []
        for d, x, s, n in zip(twins, xs, specs, sizes):
            o = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
            d.process_device(x, s["frames"], o)
            wants.append(o)
        torch.cuda.synchronize()
        host = lay.buf.cpu().numpy()
        assert lay.gaps_untouched(host), call
        for i, (w, n) in enumerate(zip(wants, sizes)):
            assert np.array_equal(lay.part(host, i), w.cpu().numpy()[:n]), (call, specs[i])
        for i, (a, b) in enumerate(zip(batch, twins)):
            assert a.clipped() == b.clipped(), (call, specs[i])
    # the state carried across: one single call on every context of both sets
    xs = _inputs(M, specs, 7, dtype)
    for i, (a, b, s, n) in enumerate(zip(batch, twins, specs, sizes)):
        oa = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
        ob = torch.full((max(n, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
        a.process_device(xs[i], s["frames"], oa)
        b.process_device(xs[i], s["frames"], ob)
        torch.cuda.synchronize()
        assert torch.equal(oa, ob), specs[i]
        assert a.clipped() == b.clipped(), specs[i]
    for d in batch + twins:
        d.close()


def test_reference_goldens_every_flag_combination_in_one_batch():
    z = G.load("decimate")
    ch, frames, x = decimate_input()
    x2 = torch.from_numpy(x.reshape(frames, ch).copy()).cuda()
    rows = [tuple(int(v) for v in row[:5]) for row in z["table"]]
    decs = [A.Decimator(ch, bits, nbytes, 1.0, rate, dither | shape) for (bits, nbytes, dither, shape, rate) in rows]
    outs = [torch.zeros(frames * ch * nbytes, dtype=torch.uint8, device="cuda") for (_, nbytes, _, _, _) in rows]
    classes = len(_classes(decs, [2000] * len(decs)))
    for blk in range(3):
        xin = x2[blk * 2000:(blk + 1) * 2000]
        ptrs = [o.data_ptr() + blk * 2000 * ch * r[1] for o, r in zip(outs, rows)]
        rc = A.decimate_batch_device(decs, [xin] * len(decs), [2000] * len(decs), ptrs)
        assert 1 <= rc <= classes, (rc, classes)
    torch.cuda.synchronize()
    for d, o, row, tab in zip(decs, outs, rows, z["table"]):
        buf = o.cpu().numpy()
        assert checksum_bytes(buf) == int(tab[5]), row
        assert d.clipped() == int(tab[6]), row
        key = "bytes/{}_{}_{}_{}_{}".format(*row)
        if key in z.files:
            assert np.array_equal(buf, z[key]), row
        d.close()


def test_mixed_batch_equals_single_call_twins_byte_for_byte():
    _mixed_batch_equals_twins(A, torch.float32, _specs())


@pytest.mark.parametrize("lanes", [3, 8, 64])
def test_mixed_batch_with_many_lanes_per_workgroup_equals_twins(lanes):
    """contexts of different frame counts, formats, gains and dither types in one serial wave; contexts cut across workgroups (3),
    empty lanes padding the last workgroup, the 64-lane LDS layout"""
    _mixed_batch_equals_twins(A, torch.float32, _specs(), _with_lanes(A, lanes))


def test_large_class_under_the_lane_rule_equals_twins():
    """one class big enough that the public call packs 16 lanes to a workgroup (> 8,192 lanes): frame counts, formats, gains and dither
    types mixed within it"""
    chans = [1, 2, 3, 6, 8, 33, 64, 65, 130]
    fmts = [(8, 1), (12, 2), (16, 2), (16, 4), (20, 3), (24, 3), (24, 4)]
    frames = [0, 1, 63, 64, 65, 441, 700, 130]
    specs, total, i = [], 0, 0
    while total <= 9000:
        bits, nbytes = fmts[i % 7]
        specs.append(dict(ch=chans[i % 9], bits=bits, nbytes=nbytes, flags=(HP, FLAT, LP)[i % 3] | S2, frames=frames[i % 8],
                          gain=(1.0, 0.5, 3.0)[i % 3], rate=48000))
        total += chans[i % 9] if frames[i % 8] > 0 else 0
        i += 1
    assert A.lib().arthip_decimate_batch_lanes(total) == 16
    _mixed_batch_equals_twins(A, torch.float32, specs)


def test_one_launch_for_one_class_and_side_calls_for_the_rest(monkeypatch):
    n, frames = 1024, 441
    flags = HP | SATH
    decs = [A.Decimator(2, 16, 2, 1.0, 48000, flags) for _ in range(n)]
    x = torch.rand(frames * 2, device="cuda") * 2 - 1
    out = torch.zeros(n, frames * 4, dtype=torch.uint8, device="cuda")
    assert A.decimate_batch_device(decs, [x] * n, [frames] * n, [out[i] for i in range(n)]) == 1
    torch.cuda.synchronize()
    for d in decs:
        d.close()

    monkeypatch.setenv("ARTAMD_SHARDS", "4")
    specs = [dict(ch=2, flags=flags), dict(ch=8, flags=flags | A.DECIMATE_MULTITHREADED), dict(ch=2, flags=flags), dict(ch=3, flags=flags)]
    batch = [A.Decimator(s["ch"], 16, 2, 1.0, 48000, s["flags"]) for s in specs]
    twins = [A.Decimator(s["ch"], 16, 2, 1.0, 48000, s["flags"] & ~A.DECIMATE_MULTITHREADED) for s in specs]
    assert batch[1].shards() == 4
    side = torch.cuda.Stream()                  # (non-blocking: ordered after the current stream by hand below)
    batch[2].set_stream(side.cuda_stream)
    for call in range(2):
        xs = [torch.rand(frames * s["ch"], device="cuda") * 2.4 - 1.2 for s in specs]
        outs = [torch.full((frames * s["ch"] * 2,), SENTINEL, dtype=torch.uint8, device="cuda") for s in specs]
        side.wait_stream(torch.cuda.current_stream())      # the side context's input and sentinel fill come first
        assert A.decimate_batch_device(batch, xs, [frames] * 4, outs) == 1 + 2
        wants = []
        for d, x, s in zip(twins, xs, specs):
            o = torch.full((frames * s["ch"] * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
            d.process_device(x, frames, o)
            wants.append(o)
        torch.cuda.synchronize()
        for i in range(4):
            assert torch.equal(outs[i], wants[i]), (call, specs[i])
            assert batch[i].clipped() == twins[i].clipped(), (call, specs[i])
    for d in batch + twins:
        d.close()


def test_edges_empty_duplicate_and_null():
    L = A.lib()
    assert L.decimateProcessBatchInterleavedLEDevice(None, 0, None, None, None) == 0
    specs = [dict(ch=2, bits=16, nbytes=2, flags=HP | SATH, frames=441, gain=1.0, rate=48000),
             dict(ch=6, bits=24, nbytes=3, flags=FLAT, frames=700, gain=1.0, rate=48000)]
    batch, twins = _make(A, specs), _make(A, specs)
    sizes = [s["frames"] * s["ch"] * s["nbytes"] for s in specs]
    frames = [s["frames"] for s in specs]
    xs = _inputs(A, specs, 0, torch.float32)
    lay = Layout(sizes)
    before = L.artamdErrorCount()
    with pytest.raises(RuntimeError):
        A.decimate_batch_device([batch[0], batch[1], batch[0]], xs + xs[:1], frames + frames[:1], [lay.ptr(0), lay.ptr(1), lay.ptr(0)])
    n = 2
    ctx = (C.c_void_p * n)(C.cast(batch[0].p, C.c_void_p), None)
    rc = L.decimateProcessBatchInterleavedLEDevice(ctx, n, (C.c_void_p * n)(*[x.data_ptr() for x in xs]), (C.c_int * n)(*frames),
                                                   (C.c_void_p * n)(lay.ptr(0), lay.ptr(1)))
    assert rc == -1
    torch.cuda.synchronize()
    assert np.all(lay.buf.cpu().numpy() == SENTINEL)
    assert L.artamdErrorCount() == before               # refused calls are not launch failures
    assert all(d.clipped() == 0 for d in batch)
    # the contexts are untouched: a later batch still equals the twins
    assert A.decimate_batch_device(batch, xs, frames, [lay.ptr(0), lay.ptr(1)]) >= 1
    wants = []
    for d, x, s, n_ in zip(twins, xs, specs, sizes):
        o = torch.zeros(n_, dtype=torch.uint8, device="cuda")
        d.process_device(x, s["frames"], o)
        wants.append(o)
    torch.cuda.synchronize()
    host = lay.buf.cpu().numpy()
    assert lay.gaps_untouched(host)
    for i in range(2):
        assert np.array_equal(lay.part(host, i), wants[i].cpu().numpy())
        assert batch[i].clipped() == twins[i].clipped()
    for d in batch + twins:
        d.close()


def test_wide_build_mixed_batch_equals_twins():
    W = A.wide()
    specs = [s for i, s in enumerate(_specs()) if i % 3 == 0]
    for s in specs:
        s["frames"] = min(s["frames"], 4096)
    _mixed_batch_equals_twins(W, torch.float64, specs)
    _mixed_batch_equals_twins(W, torch.float64, specs, _with_lanes(W, 3))
    _mixed_batch_equals_twins(W, torch.float64, specs, _with_lanes(W, 64))


def test_decimate_batch_bench_beats_the_loop():
    n, frames, ticks = 1024, 441, 15
    flags = HP | SATH
    loop = [A.Decimator(2, 16, 2, 1.0, 48000, flags) for _ in range(n)]
    batch = [A.Decimator(2, 16, 2, 1.0, 48000, flags) for _ in range(n)]
    x = torch.rand(n, frames * 2, device="cuda") * 2 - 1
    out = torch.zeros(n, frames * 4, dtype=torch.uint8, device="cuda")
    xs, outs = [x[i] for i in range(n)], [out[i] for i in range(n)]

    def tick_loop():
        for i, d in enumerate(loop):
            d.process_device(xs[i], frames, outs[i])

    def tick_batch():
        A.decimate_batch_device(batch, xs, [frames] * n, outs)

    def median(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = []
        for _ in range(ticks):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return statistics.median(t)

    t_loop, t_batch = median(tick_loop), median(tick_batch)
    print(f"decimate tick, 1,024 stereo x 441 frames: loop {t_loop * 1e3:.3f} ms, batch {t_batch * 1e3:.3f} ms, "
          f"{t_loop / t_batch:.1f}x")
    assert t_batch * 10 <= t_loop, (t_loop, t_batch)
    for d in loop + batch:
        d.close()
