"""decimateProcessPlanarLEDevice, decimateProcessBatchPlanarLEDevice, decimateHipReset and ClipDecimator: channels-first device
buffers through the decimator.  Everything is exact — bytes, clip counts, state — against a twin context that takes
decimateProcessInterleavedLEDevice on the transposed input (which tests/test_gpu_parity.py pins to the reference's goldens).

Planes live in sentinel-filled slabs with odd pitches and bases off by one sample / one byte, so every run has a head and a tail
around its 16-byte units, and every byte outside the written runs is checked."""
import ctypes as C

import numpy as np
import pytest
import torch

import _golden as G
import audio_resampler_amd as A
from test_gpu_decimate_batch import _classes, _specs
from test_oracle_golden import decimate_input

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
S1, S2, S3, SATH = A.SHAPING_1ST_ORDER, A.SHAPING_2ND_ORDER, A.SHAPING_3RD_ORDER, A.SHAPING_ATH_CURVE
HP, FLAT, LP = A.DITHER_HIGHPASS, A.DITHER_FLAT, A.DITHER_LOWPASS
CHANS = [1, 2, 3, 8, 33, 65]
FMTS = [(8, 1), (12, 2), (16, 2), (16, 4), (20, 3), (24, 3), (24, 4)]
DITHERS = [0, HP, FLAT, LP]
SHAPES = [0, S1, S2, S3, SATH]


def _dtype(M):
    return torch.float64 if getattr(M, "width", 32) == 64 else torch.float32


def _chunk(M, ch):
    """frames per chunk of the single call's pipelined serial kernel for the first channel group of a `ch`-channel context
    (pcm_kernels.hip: decimate_pipe_kernel, 8 channels per workgroup)"""
    dec_chunk = 2048 if getattr(M, "width", 32) == 64 else 4096
    return ((dec_chunk // min(ch, 8)) - 4) & ~3


def _frame_counts(M, ch):
    k = _chunk(M, ch)
    return [1, 31, 32, 33, 63, 64, 65, k - 1, k + 1, 2 * k - 1, 2 * k + 1, 4099]


class InSlab:
    """the planes of x [C, T] in one sentinel-filled slab: pitch T + 5 samples, the first plane one sample into the slab.  The
    pitch is not "odd": it is even for an odd T and odd for an even one, and the frame counts used here have both parities, so
    planes start at every offset within a 16-byte unit"""
    def __init__(self, x, pad=5, off=1):
        ch, T = x.shape
        self.pitch = T + pad
        size = x.element_size()
        self.buf = torch.full(((off + ch * self.pitch + 4) * size,), SENTINEL, dtype=torch.uint8, device="cuda").view(x.dtype)
        torch.as_strided(self.buf, (ch, T), (self.pitch, 1), off).copy_(x)
        self.ptr = self.buf.data_ptr() + off * size


class OutSlab:
    """C planes of `run` bytes in one sentinel-filled slab: pitch run + 7 bytes, the first plane one byte into the slab"""
    def __init__(self, ch, run, pad=7, off=1):
        self.ch, self.run, self.pitch, self.off = ch, run, run + pad, off
        self.buf = torch.full((off + ch * self.pitch + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr() + off

    def planes(self):
        return torch.as_strided(self.buf, (self.ch, self.run), (self.pitch, 1), self.off)

    def untouched_outside(self):
        rest = self.buf.clone()
        torch.as_strided(rest, (self.ch, self.run), (self.pitch, 1), self.off).fill_(SENTINEL)
        return bool(torch.all(rest == SENTINEL))


def _twin_planes(twin, x, frames, nbytes):
    """what the planar call must leave: the twin's interleaved call on the transposed input, transposed back -> [C, frames * nbytes]"""
    ch = x.shape[0]
    out = torch.full((max(frames * ch * nbytes, 1),), SENTINEL, dtype=torch.uint8, device="cuda")
    twin.process_device(x.t().contiguous(), frames, out)
    return out[:frames * ch * nbytes].view(frames, ch, nbytes).permute(1, 0, 2).reshape(ch, frames * nbytes)


def _mirrors(d):
    """the host mirrors after one host-pointer call of 5 frames (it refreshes them from the device state)"""
    ch = d.channels
    d.process(np.zeros((5, ch)))
    p = d.p.contents
    out = [np.ctypeslib.as_array(p.feedback, (ch,)).copy()]
    if p.tpdf_generators:
        out.append(np.ctypeslib.as_array(p.tpdf_generators, (ch,)).copy())
    if p.noise_shapers:
        out.append(np.frombuffer(C.string_at(p.noise_shapers, C.sizeof(A.Biquad) * ch), np.uint8).copy())
    return out


def _same_state(a, b):
    assert a.clipped() == b.clipped()
    for u, v in zip(_mirrors(a), _mirrors(b)):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))


def _single_cases(M, ci, ch, subset=None):
    for j, frames in enumerate(_frame_counts(M, ch)):
        if subset is not None and j not in subset:
            continue
        bits, nbytes = FMTS[(j + ci) % 7]
        yield dict(ch=ch, bits=bits, nbytes=nbytes, flags=DITHERS[(j + 3 * ci) % 4] | SHAPES[(j + ci) % 5], frames=frames,
                   gain=3.0 if (j + ci) % 3 == 0 else 1.0, rate=(44100, 48000, 96000)[j % 3])


def _single_equals_twin(M, s, seed):
    dt = _dtype(M)
    d, twin = [M.Decimator(s["ch"], s["bits"], s["nbytes"], s["gain"], s["rate"], s["flags"]) for _ in range(2)]
    g = torch.Generator(device="cuda").manual_seed(seed)
    frames, nb = s["frames"], s["nbytes"]
    for call in range(3):                         # state carried across calls
        x = torch.rand(s["ch"], frames, generator=g, device="cuda", dtype=dt) * 2.2 - 1.1
        src, dst = InSlab(x), OutSlab(s["ch"], frames * nb)
        d.process_planar_device(src.ptr, src.pitch, frames, dst.ptr, dst.pitch)
        want = _twin_planes(twin, x, frames, nb)
        torch.cuda.synchronize()
        assert torch.equal(dst.planes(), want), (call, s)
        assert dst.untouched_outside(), (call, s)
        assert d.clipped() == twin.clipped(), (call, s)
    if s["gain"] == 3.0:
        assert d.clipped() > 0, s
    _same_state(d, twin)
    d.close(); twin.close()


@pytest.mark.parametrize("ci", range(len(CHANS)), ids=[f"{c}ch" for c in CHANS])
def test_single_planar_call_equals_interleaved_twin(ci):
    """every channel count x every frame count (the time-parallel form's segment edge and 64-frame threshold, one frame either side
    of the pipelined serial kernel's chunk and of two chunks, 4,099), formats, dither types and shaper orders cycled so that every
    (frame count, shaper) pair and every value of every axis appears"""
    for k, s in enumerate(_single_cases(A, ci, CHANS[ci])):
        _single_equals_twin(A, s, 100 * ci + k)


def test_axes_are_covered():
    cases = [s for ci, ch in enumerate(CHANS) for s in _single_cases(A, ci, ch)]
    assert {s["ch"] for s in cases} == set(CHANS)
    assert {(s["bits"], s["nbytes"]) for s in cases} == set(FMTS)
    for dith in DITHERS:
        for shape in SHAPES:
            assert any(s["flags"] == dith | shape for s in cases), (dith, shape)
    assert any(s["gain"] == 3.0 for s in cases)


def test_unpipelined_serial_form_equals_twin():
    """more workgroups than the pipelined form takes (> 256 groups of 8 channels): decimate_lds_kernel, one frame either side of its
    512-frame chunk, and the shortest call it takes"""
    cases = [dict(ch=2056, bits=16, nbytes=2, flags=HP | SATH, frames=511, gain=3.0, rate=48000),
             dict(ch=2057, bits=20, nbytes=3, flags=S2, frames=513, gain=3.0, rate=48000),
             dict(ch=2058, bits=8, nbytes=1, flags=LP | S1, frames=64, gain=3.0, rate=48000)]
    for k, s in enumerate(cases):
        _single_equals_twin(A, s, 900 + k)


@pytest.mark.parametrize("flags,frames", [(HP | SATH, 700), (FLAT, 700), (HP | S2, 40), (0, 65)])
def test_mixed_sides_and_alternating_layouts(flags, frames):
    """planar in / interleaved out, interleaved in / planar out, and a stream that alternates planar and interleaved calls,
    against a twin that is all interleaved"""
    ch, bits, nb = 3, 20, 3
    d, twin = [A.Decimator(ch, bits, nb, 3.0, 48000, flags) for _ in range(2)]
    g = torch.Generator(device="cuda").manual_seed(frames)
    for call in range(6):
        x = torch.rand(ch, frames, generator=g, device="cuda") * 2.2 - 1.1
        want = _twin_planes(twin, x, frames, nb)
        kind = call % 3
        if kind == 0:                              # planar in, interleaved out
            src = InSlab(x)
            out = torch.full((frames * ch * nb + 9,), SENTINEL, dtype=torch.uint8, device="cuda")
            d.process_planar_device(src.ptr, src.pitch, frames, out.data_ptr() + 1, 0)
            got = out[1:1 + frames * ch * nb].view(frames, ch, nb).permute(1, 0, 2).reshape(ch, frames * nb)
            rest_ok = bool(torch.all(out[0] == SENTINEL)) and bool(torch.all(out[1 + frames * ch * nb:] == SENTINEL))
        elif kind == 1:                            # interleaved in, planar out
            dst = OutSlab(ch, frames * nb)
            d.process_planar_device(x.t().contiguous(), 0, frames, dst.ptr, dst.pitch)
            got, rest_ok = dst.planes(), None
        else:                                      # the interleaved call itself
            out = torch.zeros(frames * ch * nb, dtype=torch.uint8, device="cuda")
            d.process_device(x.t().contiguous(), frames, out)
            got, rest_ok = out.view(frames, ch, nb).permute(1, 0, 2).reshape(ch, frames * nb), True
        torch.cuda.synchronize()
        assert torch.equal(got, want), (call, kind)
        assert rest_ok if rest_ok is not None else dst.untouched_outside(), (call, kind)
        assert d.clipped() == twin.clipped(), call
    assert d.clipped() > 0
    _same_state(d, twin)
    d.close(); twin.close()


def test_reference_golden_channels_first():
    """the committed `decimate` golden's planar bytes (the reference's decimateProcessLE), from channels-first device input"""
    z = G.load("decimate")
    ch, frames, x = decimate_input()
    planes = torch.from_numpy(np.ascontiguousarray(x.reshape(frames, ch).T)).cuda()
    d = A.Decimator(ch, 16, 2, 1.0, 48000, HP | SATH)
    src, dst = InSlab(planes), OutSlab(ch, frames * 2)
    d.process_planar_device(src.ptr, src.pitch, frames, dst.ptr, dst.pitch)
    torch.cuda.synchronize()
    assert d.clipped() == int(z["planar/clips"])
    assert np.array_equal(dst.planes().cpu().numpy(), z["planar/bytes"])
    assert dst.untouched_outside()
    d.close()


# ---- the batch ------------------------------------------------------------------------------------------------------------------

def _batch_specs(M, every=1):
    specs = [dict(s) for i, s in enumerate(_specs()) if i % every == 0]
    for i, s in enumerate(specs):
        s["frames"] = {4096: 4093, 100003: 2051}.get(s["frames"], s["frames"])      # (quick: two chunks and an odd count are enough)
        s["sides"] = ("pp", "pi", "ip", "ii", "pp")[i % 5]          # input, output: p planar, i interleaved ("ii": both pitches 0)
        s["sharded"] = False
    k = next(i for i, s in enumerate(specs) if s["ch"] >= 6 and s["frames"] >= 64)      # (the first such: 8 channels in the full list)
    specs[k]["sharded"], specs[k]["sides"] = True, "pp"
    assert any(s["frames"] == 0 for s in specs) and any(s["ch"] == 1 and s["frames"] > 0 for s in specs)
    return specs


def _make_batch(M, specs, monkeypatch, shard):
    out = []
    for s in specs:
        if shard and s["sharded"]:
            monkeypatch.setenv("ARTAMD_SHARDS", "2")
            out.append(M.Decimator(s["ch"], s["bits"], s["nbytes"], s["gain"], s["rate"], s["flags"] | M.DECIMATE_MULTITHREADED))
            monkeypatch.delenv("ARTAMD_SHARDS")
            assert out[-1].shards() == 2
        else:
            out.append(M.Decimator(s["ch"], s["bits"], s["nbytes"], s["gain"], s["rate"], s["flags"]))
    return out


def _with_lanes(M, lanes):
    """the planar batch with every serial class packed `lanes` lanes to a workgroup (the library's private form of the call)"""
    fn = M.lib().artamd_decimate_batch_planar
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]

    def call(decs, ins, ipitch, frames, outs, opitch):
        n = len(decs)
        rc = fn((C.c_void_p * n)(*[C.cast(d.p, C.c_void_p) for d in decs]), n, (C.c_void_p * n)(*ins), (C.c_long * n)(*ipitch),
                (C.c_int * n)(*frames), (C.c_void_p * n)(*outs), (C.c_long * n)(*opitch), lanes)
        if rc < 0:
            raise RuntimeError("artamd_decimate_batch_planar failed")
        return rc
    return call


class Buffers:
    """one call's buffers of every item: inputs as each item's sides want them, all outputs in ONE sentinel slab"""
    def __init__(self, specs, xs):
        self.specs, self.keep, self.ins, self.ipitch, self.opitch, self.span, self.off = specs, [], [], [], [], [], []
        pos = 33
        for s, x in zip(specs, xs):
            ch, T, nb = s["ch"], s["frames"], s["nbytes"]
            if s["sides"][0] == "p":
                src = InSlab(x) if T else InSlab(x[:, :0])
                self.keep.append(src); self.ins.append(src.ptr); self.ipitch.append(src.pitch)
            else:
                t = x.t().contiguous()
                self.keep.append(t); self.ins.append(t.data_ptr()); self.ipitch.append(0)
            planar_out = s["sides"][1] == "p"
            self.opitch.append(T * nb + 7 if planar_out else 0)
            self.off.append(pos)
            self.span.append((ch - 1) * (T * nb + 7) + T * nb if planar_out else ch * T * nb)
            pos += self.span[-1] + 29
        self.slab = torch.full((pos + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
        self.outs = [self.slab.data_ptr() + o for o in self.off]

    def planes(self, i):
        """item i's output as [C, frames * nbytes]"""
        s = self.specs[i]
        ch, T, nb = s["ch"], s["frames"], s["nbytes"]
        if self.opitch[i]:
            return torch.as_strided(self.slab, (ch, T * nb), (self.opitch[i], 1), self.off[i])
        return self.slab[self.off[i]:self.off[i] + ch * T * nb].view(T, ch, nb).permute(1, 0, 2).reshape(ch, T * nb)

    def untouched_outside(self):
        rest = self.slab.clone()
        for i, s in enumerate(self.specs):
            ch, T, nb = s["ch"], s["frames"], s["nbytes"]
            if self.opitch[i]:
                torch.as_strided(rest, (ch, T * nb), (self.opitch[i], 1), self.off[i]).fill_(SENTINEL)
            else:
                rest[self.off[i]:self.off[i] + ch * T * nb] = SENTINEL
        return bool(torch.all(rest == SENTINEL))


def _batch_equals_loops(M, specs, monkeypatch, batch_call=None):
    batch_call = batch_call or M.decimate_batch_planar_device
    dt = _dtype(M)
    batch = _make_batch(M, specs, monkeypatch, True)
    singles, inter = _make_batch(M, specs, monkeypatch, False), _make_batch(M, specs, monkeypatch, False)
    frames = [s["frames"] for s in specs]
    gathered = [d for d, s in zip(batch, specs) if not s["sharded"]]
    bound = len(_classes(gathered, [s["frames"] for s in specs if not s["sharded"]])) + sum(s["sharded"] for s in specs)
    for call in range(2):
        g = torch.Generator(device="cuda").manual_seed(77 + call)
        xs = [torch.rand(s["ch"], max(s["frames"], 1), generator=g, device="cuda", dtype=dt)[:, :s["frames"]] * 2.2 - 1.1 for s in specs]
        a, b = Buffers(specs, xs), Buffers(specs, xs)
        rc = batch_call(batch, a.ins, a.ipitch, frames, a.outs, a.opitch)
        assert 1 <= rc <= bound, (rc, bound)
        for i, d in enumerate(singles):           # the loop of single planar calls
            d.process_planar_device(b.ins[i], b.ipitch[i], frames[i], b.outs[i], b.opitch[i])
        # the interleaved batch on transposed copies
        tin = [x.t().contiguous() for x in xs]
        tout = [torch.full((max(s["frames"] * s["ch"] * s["nbytes"], 1),), SENTINEL, dtype=torch.uint8, device="cuda") for s in specs]
        M.decimate_batch_device(inter, tin, frames, tout)
        torch.cuda.synchronize()
        assert a.untouched_outside() and b.untouched_outside(), call
        for i, s in enumerate(specs):
            T, ch, nb = s["frames"], s["ch"], s["nbytes"]
            want = tout[i][:T * ch * nb].view(T, ch, nb).permute(1, 0, 2).reshape(ch, T * nb)
            assert torch.equal(a.planes(i), want), (call, i, s)
            assert torch.equal(b.planes(i), want), (call, i, s)
            assert batch[i].clipped() == inter[i].clipped() == singles[i].clipped(), (call, i, s)
    assert any(d.clipped() > 0 for d in batch)
    for x, y in zip(batch, inter):
        _same_state(x, y)
    for d in batch + singles + inter:
        d.close()


def test_planar_batch_equals_single_calls_and_interleaved_batch(monkeypatch):
    """40 mixed contexts: a 0-frame item, one-channel items, items with one or both pitches 0, one context forced into 2 shards"""
    _batch_equals_loops(A, _batch_specs(A), monkeypatch)


@pytest.mark.parametrize("lanes", [1, 8, 64])
def test_planar_batch_with_fixed_lanes_per_workgroup(monkeypatch, lanes):
    _batch_equals_loops(A, _batch_specs(A), monkeypatch, _with_lanes(A, lanes))


def test_batch_argument_errors_write_nothing():
    L = A.lib()
    specs = [dict(ch=2, bits=16, nbytes=2, flags=HP | SATH, frames=441, gain=1.0, rate=48000, sides="pp"),
             dict(ch=6, bits=24, nbytes=3, flags=FLAT, frames=700, gain=1.0, rate=48000, sides="pp")]
    decs = [A.Decimator(s["ch"], s["bits"], s["nbytes"], s["gain"], s["rate"], s["flags"]) for s in specs]
    xs = [torch.rand(s["ch"], s["frames"], device="cuda") * 2 - 1 for s in specs]
    buf = Buffers(specs, xs)
    before = L.artamdErrorCount()
    with pytest.raises(RuntimeError):              # a duplicate
        A.decimate_batch_planar_device([decs[0], decs[1], decs[0]], buf.ins + buf.ins[:1], buf.ipitch + buf.ipitch[:1], [441, 700, 441],
                                       buf.outs + buf.outs[:1], buf.opitch + buf.opitch[:1])
    n = 2                                           # a NULL context
    rc = L.decimateProcessBatchPlanarLEDevice((C.c_void_p * n)(C.cast(decs[0].p, C.c_void_p), None), n, (C.c_void_p * n)(*buf.ins),
                                              (C.c_long * n)(*buf.ipitch), (C.c_int * n)(441, 700), (C.c_void_p * n)(*buf.outs),
                                              (C.c_long * n)(*buf.opitch))
    assert rc == -1
    torch.cuda.synchronize()
    assert bool(torch.all(buf.slab == SENTINEL))
    assert L.artamdErrorCount() == before
    assert all(d.clipped() == 0 for d in decs)
    for d in decs:
        d.close()


# ---- reset ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags,shards", [(HP | SATH, 0), (LP, 0), (FLAT | S3, 2)], ids=["shaped_dithered", "unshaped_dithered", "two_shards"])
def test_reset_gives_a_fresh_context(monkeypatch, flags, shards):
    ch, bits, nb, frames = 4, 16, 2, 300
    if shards:
        monkeypatch.setenv("ARTAMD_SHARDS", str(shards))
        flags |= A.DECIMATE_MULTITHREADED
    used, fresh = [A.Decimator(ch, bits, nb, 3.0, 48000, flags) for _ in range(2)]
    assert used.shards() == shards
    g = torch.Generator(device="cuda").manual_seed(5)
    for call in range(3):
        x = torch.rand(ch, frames, generator=g, device="cuda") * 2.2 - 1.1
        dst = OutSlab(ch, frames * nb)
        used.process_planar_device(x, frames, frames, dst.ptr, dst.pitch)
    total = used.clipped()
    assert total > 0
    used.reset()
    # the host mirrors are a fresh context's at once, the clip counter keeps its total
    pu, pf = used.p.contents, fresh.p.contents
    assert np.array_equal(np.ctypeslib.as_array(pu.feedback, (ch,)), np.ctypeslib.as_array(pf.feedback, (ch,)))
    assert np.array_equal(np.ctypeslib.as_array(pu.tpdf_generators, (ch,)), np.ctypeslib.as_array(pf.tpdf_generators, (ch,)))
    if pu.noise_shapers:
        assert C.string_at(pu.noise_shapers, C.sizeof(A.Biquad) * ch) == C.string_at(pf.noise_shapers, C.sizeof(A.Biquad) * ch)
    assert used.clipped() == total
    for call in range(2):                          # the next calls are a fresh context's first calls
        x = torch.rand(ch, frames, generator=g, device="cuda") * 2.2 - 1.1
        a, b = OutSlab(ch, frames * nb), OutSlab(ch, frames * nb)
        used.process_planar_device(x, frames, frames, a.ptr, a.pitch)
        fresh.process_planar_device(x, frames, frames, b.ptr, b.pitch)
        torch.cuda.synchronize()
        assert torch.equal(a.buf, b.buf), call
        assert used.clipped() - total == fresh.clipped(), call
    used.close(); fresh.close()


# ---- ClipDecimator ---------------------------------------------------------------------------------------------------------------

def _clip_twin(x, length, bits, nb, gain, rate, flags):
    d = A.Decimator(x.shape[0], bits, nb, gain, rate, flags)
    out = torch.zeros(max(length * x.shape[0] * nb, 1), dtype=torch.uint8, device="cuda")
    d.process_device(x[:, :length].t().contiguous(), length, out)
    clips = d.clipped()
    d.close()
    return out[:length * x.shape[0] * nb].view(length, x.shape[0], nb).permute(1, 0, 2).reshape(x.shape[0], length * nb), clips


def test_clip_decimator_equals_fresh_decimators():
    lengths = [1000, 999, 64, 1, 0]
    x = torch.rand(5, 2, 1000, generator=torch.Generator(device="cuda").manual_seed(3), device="cuda") * 3.0 - 1.5
    cd = A.ClipDecimator(2, 16, 2, 1.0, 48000, HP | SATH)
    pcm, clipped = cd(x, lengths)
    assert pcm.shape == (5, 2, 2000) and pcm.dtype == torch.uint8
    wants = [_clip_twin(x[i], n, 16, 2, 1.0, 48000, HP | SATH) for i, n in enumerate(lengths)]
    for i, (n, (want, clips)) in enumerate(zip(lengths, wants)):
        assert torch.equal(pcm[i, :, :n * 2], want), i
        assert bool(torch.all(pcm[i, :, n * 2:] == 0)), i
        assert int(clipped[i]) == clips, i
    assert int(clipped[0]) > 0
    pcm2, clipped2 = cd(x, torch.tensor(lengths))                   # the pool is reset for every call
    assert torch.equal(pcm, pcm2) and torch.equal(clipped, clipped2)
    ints = cd.as_int(pcm)
    assert ints.dtype == torch.int16 and ints.shape == (5, 2, 1000)
    assert torch.equal(ints.view(torch.uint8), pcm)
    assert torch.equal(ints[0, 1], (pcm[0, 1, 0::2].to(torch.int32) | (pcm[0, 1, 1::2].to(torch.int32) << 8)).to(torch.int16))
    pcm1, _ = cd(x[0])                                              # [C, T]
    assert torch.equal(pcm1[0], pcm[0])
    cd.close()


def test_clip_decimator_behind_clip_resampler():
    x = torch.rand(3, 2, 4410, generator=torch.Generator(device="cuda").manual_seed(9), device="cuda") * 2 - 1
    rs = A.ClipResampler(2, 44100, 48000)
    cd = A.ClipDecimator(2, 24, 4, 1.0, 48000, HP | SATH)
    y, out_lengths = rs(x, [4410, 2000, 441])
    pcm, clipped = cd(y, out_lengths)
    assert pcm.shape == (3, 2, y.shape[2] * 4)
    for i, n in enumerate(out_lengths.tolist()):
        want, clips = _clip_twin(y[i], n, 24, 4, 1.0, 48000, HP | SATH)
        assert torch.equal(pcm[i, :, :n * 4], want), i
        assert bool(torch.all(pcm[i, :, n * 4:] == 0)), i
        assert int(clipped[i]) == clips, i
    assert cd.as_int(pcm).dtype == torch.int32
    rs.close(); cd.close()


# ---- the 8-byte build ------------------------------------------------------------------------------------------------------------

def test_wide_build_single_calls_equal_twins():
    W = A.wide()
    for ci, ch in enumerate(CHANS):
        for k, s in enumerate(_single_cases(W, ci, ch, subset=(ci, ci + 6))):      # two frame counts per channel count: all twelve
            _single_equals_twin(W, s, 500 + 10 * ci + k)


def test_wide_build_planar_batch_equals_loops(monkeypatch):
    W = A.wide()
    _batch_equals_loops(W, _batch_specs(W, every=3), monkeypatch)
    _batch_equals_loops(W, _batch_specs(W, every=3), monkeypatch, _with_lanes(W, 8))
