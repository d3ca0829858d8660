"""floatIntegersBatchLEDevice: many buffers' integer PCM to samples in one launch.  Every item's output is, bit for bit, that of its own
floatIntegersLEDevice call into a separate buffer, in both builds; skipped and refused items leave their outputs untouched; and a
PCM-in, PCM-out tick of ingest, resampler and decimator batch calls equals the same tick made of single calls."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _golden as G
import audio_resampler_amd as A
from audio_resampler_amd.api import process_batch_device

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
GAP = 64                                        # sentinel bytes after every output (and 16-byte aligned starts)
GOLDEN_FORMATS = ((8, 1), (16, 2), (24, 3), (24, 4), (12, 2), (20, 3))
WIDTHS = [pytest.param(32, id="float"), pytest.param(64, id="double")]


def _uint(esize):
    return np.uint32 if esize == 4 else np.uint64


class Outs:
    """every item's output in one byte buffer filled with SENTINEL; skew [i]: output i starts one sample past a 16-byte boundary"""
    def __init__(self, counts, esize, skew):
        self.esize, self.counts, self.off = esize, [max(int(c), 0) for c in counts], []
        pos = GAP
        for c, k in zip(self.counts, skew):
            o = pos + (esize if k else 0)
            self.off.append(o)
            pos = (o + c * esize + GAP + 15) // 16 * 16
        self.buf = torch.full((pos,), SENTINEL, dtype=torch.uint8, device="cuda")

    def ptr(self, i):
        return self.buf.data_ptr() + self.off[i]

    def host(self):
        return self.buf.cpu().numpy()

    def part(self, h, i):
        return h[self.off[i]:self.off[i] + self.counts[i] * self.esize].view(_uint(self.esize))

    def rest_untouched(self, h, live):
        """everything but the outputs of the items in `live` still holds the sentinel"""
        mask = np.ones(h.size, bool)
        for i in live:
            mask[self.off[i]:self.off[i] + self.counts[i] * self.esize] = False
        return bool(np.all(h[mask] == SENTINEL))


def _pcm(rng, count, nbytes, stride):
    """the bytes one item reads: random, the first samples set to the extremes; no bytes after the last sample's own"""
    size = (count - 1) * stride * nbytes + nbytes
    b = rng.integers(0, 256, size, dtype=np.uint8)
    patterns = [[0x00] * nbytes, [0x00] * (nbytes - 1) + [0x80], [0xFF] * (nbytes - 1) + [0x7F], [0xFF] * nbytes, [0x80] * nbytes]
    for k, pat in enumerate(patterns[:count]):
        b[k * stride * nbytes:k * stride * nbytes + nbytes] = pat
    return torch.from_numpy(b).cuda()


def _singles(M, esize, ins, specs, stream=None):
    """each item's own floatIntegersLEDevice into a separate SENTINEL-filled buffer"""
    outs = []
    for x, s in zip(ins, specs):
        o = torch.full((max(s["count"], 1) * esize,), SENTINEL, dtype=torch.uint8, device="cuda")
        M.lib().floatIntegersLEDevice(x if isinstance(x, int) else x.data_ptr(), s["gain"], s["bits"], s["nbytes"], s["stride"],
                                      o.data_ptr(), s["count"], stream)
        outs.append(o)
    return outs


def _batch(M, ins, specs, outs, stream=None):
    return M.ingest_batch_device(ins, [s["gain"] for s in specs], [s["bits"] for s in specs], [s["nbytes"] for s in specs],
                                 [s["stride"] for s in specs], [outs.ptr(i) for i in range(len(specs))], [s["count"] for s in specs],
                                 stream)


def _equals_singles(M, esize, ins, specs, skew):
    outs = Outs([s["count"] for s in specs], esize, skew)
    assert _batch(M, ins, specs, outs) == 1
    wants = _singles(M, esize, ins, specs)
    torch.cuda.synchronize()
    h = outs.host()
    live = [i for i, s in enumerate(specs) if s["count"] > 0 and s["bits"] <= 24]
    for i in live:
        want = wants[i].cpu().numpy()[:specs[i]["count"] * esize].view(_uint(esize))
        assert np.array_equal(outs.part(h, i), want), specs[i]
    assert outs.rest_untouched(h, live)


def test_golden_formats_in_one_batch_both_widths():
    raw = torch.from_numpy(G.load("decimate")["ingest/raw"].copy()).cuda()
    wide = np.load(os.path.join(G.GOLD, "wide.npz"))
    specs = [dict(bits=b, nbytes=n, gain=0.75, stride=2, count=50) for b, n in GOLDEN_FORMATS]
    for M, esize, z in ((A, 4, G.load("decimate")), (A.wide(), 8, wide)):
        outs = Outs([50] * 6, esize, [i % 2 for i in range(6)])
        assert _batch(M, [raw] * 6, specs, outs) == 1             # (every item reads the same buffer)
        torch.cuda.synchronize()
        h = outs.host()
        for i, (b, n) in enumerate(GOLDEN_FORMATS):
            want = np.ascontiguousarray(z[f"ingest/{b}_{n}"]).view(_uint(esize))
            assert np.array_equal(outs.part(h, i), want), (esize, b, n)
        assert outs.rest_untouched(h, range(6))


def _twin_specs():
    counts, strides, gains = [1, 3, 255, 256, 257, 4097], [1, 2, 3, 8], [0.0, -1.0, 0.75, 3.7, 1e-30]
    specs, k = [], 0
    for bits in (1, 7, 8, 9, 12, 15, 16, 17, 20, 23, 24):
        for nbytes in range((bits + 7) // 8, 5):
            for _ in range(2):
                specs.append(dict(bits=bits, nbytes=nbytes, stride=strides[k % 4], gain=gains[k % 5], count=counts[k % 6]))
                k += 1
    specs.append(dict(bits=16, nbytes=2, stride=1, gain=0.75, count=1 << 20))
    specs.append(dict(bits=24, nbytes=4, stride=3, gain=-1.0, count=(1 << 20) - 1))
    return specs


@pytest.mark.parametrize("width", WIDTHS)
def test_every_format_count_stride_and_gain_equals_single_calls(width):
    M, esize = A.binding(width), width // 8
    specs = _twin_specs()
    rng = np.random.default_rng(7 + width)
    ins = [_pcm(rng, s["count"], s["nbytes"], s["stride"]) for s in specs]
    _equals_singles(M, esize, ins, specs, [i % 3 == 1 for i in range(len(specs))])


@pytest.mark.parametrize("width", WIDTHS)
def test_skipped_items_sentinels_and_refused_calls(width):
    M, esize = A.binding(width), width // 8
    L = M.lib()
    rng = np.random.default_rng(3)
    specs = [dict(bits=16, nbytes=2, stride=2, gain=1.0, count=441),
             dict(bits=16, nbytes=2, stride=1, gain=1.0, count=0),
             dict(bits=24, nbytes=3, stride=1, gain=1.0, count=-5),
             dict(bits=25, nbytes=4, stride=1, gain=1.0, count=100),
             dict(bits=32, nbytes=4, stride=1, gain=1.0, count=100),
             dict(bits=8, nbytes=1, stride=1, gain=0.5, count=17)]
    ins = [_pcm(rng, max(s["count"], 1), s["nbytes"], s["stride"]) for s in specs]
    _equals_singles(M, esize, ins, specs, [i % 2 for i in range(len(specs))])

    assert L.floatIntegersBatchLEDevice(None, None, None, None, None, None, None, 0, None) == 0
    assert L.floatIntegersBatchLEDevice(None, None, None, None, None, None, None, -1, None) == 0
    skipped = [1, 2, 3, 4]
    outs = Outs([s["count"] for s in specs], esize, [0] * len(specs))
    assert _batch(M, [ins[i] for i in skipped], [specs[i] for i in skipped], outs) == 0
    torch.cuda.synchronize()
    assert outs.rest_untouched(outs.host(), [])

    before = L.artamdErrorCount()
    for hole in ("in", "out"):
        outs = Outs([s["count"] for s in specs], esize, [0] * len(specs))
        n = len(specs)
        d_ins = [x.data_ptr() for x in ins]
        d_outs = [outs.ptr(i) for i in range(n)]
        (d_ins if hole == "in" else d_outs)[5] = None
        rc = L.floatIntegersBatchLEDevice(
            (C.c_void_p * n)(*d_ins), (C.c_double * n)(*[s["gain"] for s in specs]), (C.c_int * n)(*[s["bits"] for s in specs]),
            (C.c_int * n)(*[s["nbytes"] for s in specs]), (C.c_int * n)(*[s["stride"] for s in specs]), (C.c_void_p * n)(*d_outs),
            (C.c_int * n)(*[s["count"] for s in specs]), n, None)
        assert rc == -1
        torch.cuda.synchronize()
        assert outs.rest_untouched(outs.host(), [])
    assert L.artamdErrorCount() == before                    # refused calls are not launch failures


def test_thousands_of_items_equal_the_loop():
    """4,096 items of 882 samples (the golden formats, strides 1 and 2, one shared input buffer) and one of 2^20 samples"""
    rng = np.random.default_rng(11)
    big = torch.from_numpy(rng.integers(0, 256, 882 * 2 * 4 + 4096 * 3, dtype=np.uint8)).cuda()
    specs, ins = [], []
    for i in range(4096):
        b, n = GOLDEN_FORMATS[i % 6]
        specs.append(dict(bits=b, nbytes=n, stride=1 + (i // 6) % 2, gain=(1.0, 0.5, 2.0)[i % 3], count=882))
        ins.append(big.data_ptr() + (i * 3) % 4096)
    specs.append(dict(bits=24, nbytes=3, stride=1, gain=0.9, count=1 << 20))
    ins.append(_pcm(rng, 1 << 20, 3, 1))
    _equals_singles(A, 4, ins, specs, [i % 5 == 2 for i in range(len(specs))])


def test_runs_in_order_on_a_non_default_stream():
    rng = np.random.default_rng(5)
    specs = [dict(bits=(16, 24)[i % 2], nbytes=(2, 4)[i % 2], stride=2, gain=0.8, count=4410 + i) for i in range(64)]
    size = max((s["count"] - 1) * s["stride"] * s["nbytes"] + s["nbytes"] for s in specs)
    seed = torch.from_numpy(rng.integers(0, 256, size, dtype=np.uint8)).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        # the producer: a chain of kernels on `side`, then the batch on the same stream, then the read, nothing synchronised
        pcm = seed.to(torch.int32)
        for k in range(20):
            pcm = (pcm * 5 + k) & 255
        pcm = pcm.to(torch.uint8)
        outs = Outs([s["count"] for s in specs], 4, [i % 2 for i in range(len(specs))])
        assert _batch(A, [pcm] * len(specs), specs, outs, stream=side) == 1
        h = outs.host()
    torch.cuda.synchronize()
    wants = _singles(A, 4, [pcm] * len(specs), specs)
    torch.cuda.synchronize()
    for i, s in enumerate(specs):
        assert np.array_equal(outs.part(h, i), wants[i].cpu().numpy().view(np.uint32)), i
    assert outs.rest_untouched(h, range(len(specs)))


# --------------------------------------------------------------------------------------------------------------------------------
# PCM in, PCM out: ingest batch -> resampler batch -> decimator batch, against the same ticks made of single calls
# --------------------------------------------------------------------------------------------------------------------------------
def _stream_specs():
    rates = [(44100, 48000), (48000, 44100), (96000, 48000), (16000, 48000)]
    fmts = [(16, 2), (24, 3), (24, 4)]
    out = []
    for i in range(48):
        src, dst = rates[i % 4]
        bits, nbytes = fmts[i % 3]
        out.append(dict(ch=(1, 2, 8)[i % 3], bits=bits, nbytes=nbytes, src=src, dst=dst, block=(441, 480, 512, 960)[(i // 3) % 4],
                        taps=(64, 128)[i % 2], dec_gain=(1.0, 1.5)[(i // 2) % 2],
                        dec_flags=(A.DITHER_HIGHPASS | A.SHAPING_ATH_CURVE, A.DITHER_FLAT, 0)[(i // 4) % 3]))
    return out


def test_pcm_to_pcm_ticks_equal_single_calls():
    specs = _stream_specs()
    n = len(specs)

    def make():
        rs = []
        for s in specs:
            r = A.Resampler(s["ch"], s["taps"], s["taps"], 0.0, A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE)
            r.advance(s["taps"] / 2)
            rs.append(r)
        ds = [A.Decimator(s["ch"], 16, 2, s["dec_gain"], s["dst"], s["dec_flags"]) for s in specs]
        return rs, ds

    (rb, db), (rt, dt) = make(), make()
    caps = [int(s["block"] * s["dst"] / s["src"] * 1.02) + 16 for s in specs]
    rng = np.random.default_rng(17)
    for tick in range(6):
        ratios = [s["dst"] / s["src"] * (1 + 1e-4 * ((i + tick) % 5 - 2)) for i, s in enumerate(specs)]
        pcm = [_pcm(rng, s["block"] * s["ch"], s["nbytes"], 1) for s in specs]
        gains = [1.0 if i % 2 else 0.6 for i in range(n)]
        counts = [s["block"] * s["ch"] for s in specs]

        xb = [torch.zeros(c, device="cuda") for c in counts]
        assert A.ingest_batch_device(pcm, gains, [s["bits"] for s in specs], [s["nbytes"] for s in specs], [1] * n, xb, counts) == 1
        yb = [torch.zeros(cap * s["ch"], device="cuda") for cap, s in zip(caps, specs)]
        made_b = process_batch_device(rb, xb, [s["block"] for s in specs], yb, caps, ratios)
        ob = [torch.full((cap * s["ch"] * 2,), SENTINEL, dtype=torch.uint8, device="cuda") for cap, s in zip(caps, specs)]
        assert A.decimate_batch_device(db, yb, [g for _, g in made_b], ob) >= 1

        made_t, ot = [], []
        for i, s in enumerate(specs):
            x = torch.zeros(counts[i], device="cuda")
            A.lib().floatIntegersLEDevice(pcm[i].data_ptr(), gains[i], s["bits"], s["nbytes"], 1, x.data_ptr(), counts[i], None)
            y = torch.zeros(caps[i] * s["ch"], device="cuda")
            made_t.append(rt[i].process_device(x, s["block"], y, caps[i], ratios[i]))
            o = torch.full((caps[i] * s["ch"] * 2,), SENTINEL, dtype=torch.uint8, device="cuda")
            dt[i].process_device(y, made_t[-1][1], o)
            ot.append(o)
        torch.cuda.synchronize()
        assert made_b == made_t, tick
        for i in range(n):
            assert torch.equal(ob[i], ot[i]), (tick, specs[i])
            assert db[i].clipped() == dt[i].clipped(), (tick, specs[i])
    assert any(d.clipped() > 0 for d in db)
    for obj in rb + rt + db + dt:
        obj.close()
