"""GPU (-m gpu): the batch entries gather matrix-core calls.  resampleProcessBatchInterleavedDevice (and the process phase of
resampleProcessAndFlushBatchInterleavedDevice) runs the calls whose single call would be ONE un-split launch of the f32 streaming
matrix kernel on rows kept across calls — calls big enough for the matrix path under kernel preference 6 (or 0 / 2 where that is the
library's own choice), every anchored call of a context under the cut-invariant policy — as one grouped launch per shape
(fir_mfma_group_kernel).  A tile never mixes streams, so every output is bit for bit the single call's: the oracle of this file is the
loop of single calls on twin contexts (counts, every output bit, state(), last_kernel()), and the fp64-accumulating oracle for one
gathered round per shape.  A stream's first matrix launch builds its rows and stays a single call: from round 2 on every eligible
context reports last_gathered() == 1, every context whose call the general kernel's shared launch runs too, and every other context 0."""
import hashlib

import numpy as np
import pytest

import audio_resampler_amd as A
from _hip import tolerance_ok
from _oracle import noise, OracleResampler, BH, INTERP, PRECISE

pytestmark = pytest.mark.gpu
LP = A.INCLUDE_LOWPASS
UP, DOWN = (44100.0, 48000.0), (96000.0, 44100.0)


def S(ch, T, F, rates=UP, flags=BH | INTERP, pref=6, policy=False, extra=0, ratio=0.0, sharded=False):
    return dict(ch=ch, T=T, F=F, rates=rates, flags=flags | extra, pref=pref, policy=policy, ratio=ratio, sharded=sharded)


def make(B, s):
    fl = s["flags"] | (A.RESAMPLE_MULTITHREADED if s["sharded"] else 0)
    r = B.Resampler(s["ch"], s["T"], s["F"], 0.0, fl, None if s["rates"] is None else (s["rates"][0], s["rates"][1], 0))
    if s["pref"]:
        r.set_kernel(s["pref"])
    if s["policy"]:
        r.set_cut_invariant(True)
    r.advance(s["T"] / 2)
    return r


def gain(s):
    return s["ratio"] if s["rates"] is None else s["rates"][1] / s["rates"][0]


def bits(a, width=32):
    return np.ascontiguousarray(a).view(np.uint32 if width == 32 else np.uint64)


def drive(width, specs, sizes, eligible, offsets=None, after=None, loose=(), general=()):
    """Twin sets of contexts: one through the batch entry, one through single calls; sizes [round][context] input frames.  eligible:
    the contexts whose calls are gathered from round 2 on (width 32).  offsets [context]: floats the context's input starts behind an
    aligned buffer.  general: the contexts whose calls the general kernel's shared launch runs; every
    other context's calls are single calls, checked every round.  loose: rounds in which a
    call may be made either way (the round after a reset may rebuild a set).  Returns the batch-side contexts and their twins (open)."""
    import torch
    B = A.binding(width)
    dt, tdt = (np.float32, torch.float32) if width == 32 else (np.float64, torch.float64)
    batch, single = [make(B, s) for s in specs], [make(B, s) for s in specs]
    rng = np.random.default_rng(len(specs) * 1000 + width)
    n = len(specs)
    for rnd, row in enumerate(sizes):
        if after and rnd in after:
            after[rnd](batch, single)
        d_in, caps = [], []
        for i, s in enumerate(specs):
            k, off = row[i], (offsets[i] if offsets else 0)
            flat = torch.from_numpy((rng.random(off + max(k, 1) * s["ch"]) - 0.5).astype(dt)).cuda()
            d_in.append(flat[off:off + max(k, 1) * s["ch"]].view(max(k, 1), s["ch"]))
            caps.append(int(k * max(gain(s), 1.0) * 1.02) + 4 * s["T"] + 64)
        d_out_b = [torch.zeros(c, s["ch"], device="cuda", dtype=tdt) for c, s in zip(caps, specs)]
        d_out_s = [torch.zeros(c, s["ch"], device="cuda", dtype=tdt) for c, s in zip(caps, specs)]
        ratios = [s["ratio"] for s in specs]
        got = B.process_batch_device(batch, d_in, row, d_out_b, caps, ratios)
        for i in range(n):
            u, g = single[i].process_device(d_in[i], row[i], d_out_s[i], caps[i], ratios[i])
            assert got[i] == (u, g), (rnd, i, got[i], (u, g))
            assert u == row[i], (rnd, i, u)
            diff = int(np.count_nonzero(bits(d_out_b[i][:g].cpu().numpy(), width) != bits(d_out_s[i][:g].cpu().numpy(), width)))
            assert diff == 0, (rnd, i, diff, g)
            assert batch[i].state() == single[i].state(), (rnd, i)
            assert batch[i].last_kernel() == single[i].last_kernel(), (rnd, i, batch[i].last_kernel(), single[i].last_kernel())
            assert single[i].last_gathered() == 0
            if rnd >= 1 and g and rnd not in loose:
                want = 1 if (i in eligible and width == 32) else None
                if want is not None:
                    assert batch[i].last_gathered() == 1 and batch[i].last_kernel() == 2, (rnd, i, batch[i].last_gathered(), batch[i].last_kernel())
                elif i in general:
                    assert batch[i].last_gathered() == 1 and batch[i].last_kernel() == 1, (rnd, i, batch[i].last_gathered(), batch[i].last_kernel())
                else:                              # (also the eligible ones in the 8-byte build: no streaming kernel, no kept rows)
                    assert batch[i].last_gathered() == 0, (rnd, i, batch[i].last_kernel())
        for i in range(n):
            assert batch[i].cut_invariant_fallbacks() == single[i].cut_invariant_fallbacks(), (rnd, i)
    return batch, single


def finish(width, specs, batch, single):
    for s, b, q in zip(specs, batch, single):
        ub, gb, yb = b.process(None, 3 * s["T"], s["ratio"] or 1.0, flush=True)
        us, gs, ys = q.process(None, 3 * s["T"], s["ratio"] or 1.0, flush=True)
        assert (ub, gb) == (us, gs) and np.array_equal(bits(yb, width), bits(ys, width))
        b.close(); q.close()


# shape -> (spec, call sizes of the rounds): three contexts of each shape per test
SHAPES = {
    "stereo380_fixup": (S(2, 380, 380), [24576, 24576, 4096, 65536]),                  # nearest filter, no low-pass: the pass-through pass
    "c8_988_interp": (S(8, 988, 988), [16384, 16384, 65536, 8000]),                    # 988 filters, 160 phases: interpolating rows
    "mono380": (S(1, 380, 380), [30000, 30000, 9000]),
    "c4_256": (S(4, 256, 256), [20000, 20000, 5000]),
    "c8_988_lowpass": (S(8, 988, 160, flags=BH | LP), [16384, 16384, 40000]),          # nearest filter with a low-pass: no pass
    "down_c2_380": (S(2, 380, 380, rates=DOWN, policy=True, pref=0), [9000, 3 * 320 * 7, 5000, 700]),      # several periods at a time, head_pad > 64
    "down_c8_988": (S(8, 988, 988, rates=DOWN, policy=True, pref=0), [9000, 4000, 12000]),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_grouped_calls_equal_the_loop_of_single_calls(shape):
    pytest.importorskip("torch")
    spec, rounds = SHAPES[shape]
    specs = [spec] * 3
    # (call sizes differ inside the class: the second context's calls are a little shorter, the third's a period longer)
    sizes = [[k, max(k - 37, 1), k + 147] for k in rounds]
    batch, single = drive(32, specs, sizes, eligible={0, 1, 2})
    finish(32, specs, batch, single)


def test_two_classes_among_calls_the_batch_makes_otherwise(monkeypatch):
    """two matrix classes, general-kernel streams (gathered into their own launch), a strict-order, a sharded and an extrapolating
    context, a class of one (made as its single call) — all in one batch call"""
    pytest.importorskip("torch")
    monkeypatch.setenv("ARTAMD_SHARDS", "8")                # (one device: the multi-device context's shards all live on it)
    specs = [S(2, 380, 380), S(8, 988, 988), S(2, 48, 48, rates=None, pref=0, ratio=48000 / 44100), S(2, 380, 380),
             S(2, 48, 48, rates=None, pref=0, ratio=48000 / 44100, extra=A.RESAMPLE_STRICT_ORDER), S(8, 988, 988),
             S(1, 156, 320, rates=None, pref=0, ratio=0.731), S(8, 380, 380, sharded=True), S(4, 256, 256),
             S(2, 64, 64, rates=None, pref=0, ratio=1.25, extra=A.EXTRAPOLATE_ENDPOINTS), S(8, 988, 988)]
    big = {0: 24576, 1: 16384, 3: 20000, 5: 30000, 7: 20000, 8: 20000, 10: 9000}
    sizes = [[big.get(i, 700 + 13 * i) + 100 * r for i in range(len(specs))] for r in range(4)]
    # (2, 6 and — once past its first output's call — the extrapolating 9: the general kernel's gathered launch is still made;
    #  4 strict order, 7 sharded, 8 a class of one: single calls, every round)
    batch, single = drive(32, specs, sizes, eligible={0, 1, 3, 5, 10}, general={2, 6, 9})
    assert len(batch[7].shards()) == 8
    finish(32, specs, batch, single)


def test_policy_calls_of_any_size_in_one_class():
    """under the cut-invariant policy every call of a rational-ratio stream is an anchored launch: a sub-period call shares the grouped
    launch with a 65,536-frame one and a 441-frame tick"""
    pytest.importorskip("torch")
    specs = [S(8, 988, 988, policy=True, pref=0)] * 4 + [S(2, 380, 380, policy=True, pref=0)] * 3
    sizes = [[5000, 5000, 5000, 5000, 4000, 4000, 4000],
             [100, 65536, 441, 441, 50, 65536, 441],
             [441, 441, 441, 441, 441, 441, 441],
             [1, 146, 147, 148, 1, 3, 20000]]
    batch, single = drive(32, specs, sizes, eligible=set(range(7)))
    for b in batch:
        assert b.cut_invariant_fallbacks() == 0
    finish(32, specs, batch, single)


def test_unaligned_inputs_decline_as_the_single_call_does():
    """an 8-channel input 4 bytes off a 16-byte boundary cannot take the vector-load instantiation: the single call declines anchoring
    (a counted fall-back under the policy), and so does the batch — next to aligned members of the same class, which are gathered"""
    pytest.importorskip("torch")
    specs = [S(8, 988, 988, policy=True, pref=0)] * 4 + [S(8, 988, 988)] * 3
    offsets = [0, 1, 0, 3, 0, 0, 1]
    sizes = [[6000] * 7, [6000, 6000, 441, 441, 16384, 16384, 16384], [441] * 4 + [20000] * 3]
    batch, single = drive(32, specs, sizes, eligible={0, 2, 4, 5}, offsets=offsets)
    for i in (1, 3, 6):
        assert batch[i].last_gathered() == 0, i
    assert batch[1].cut_invariant_fallbacks() > 0
    finish(32, specs, batch, single)


def test_state_after_a_group():
    """a single call after gathered calls, and gathered calls after a reset, equal the loop: the rows-cache upkeep of a gathered call is
    the single launch's, and the canonical period survives"""
    pytest.importorskip("torch")
    import torch
    specs = [S(2, 380, 380), S(2, 380, 380), S(8, 988, 988, policy=True, pref=0), S(8, 988, 988, policy=True, pref=0)]
    sizes = [[24576, 24576, 6000, 6000], [24576, 20000, 441, 300], [10000, 24576, 441, 441], [24576, 24576, 441, 441], [24576, 24576, 100, 441]]

    def reset(batch, single):
        for r in batch + single:
            r.reset()
        for r, s in zip(batch + single, specs + specs):
            r.advance(s["T"] / 2)

    def single_calls(batch, single):                       # one call of every context outside the batch entry, both sides alike
        for k, (b, q, s) in enumerate(zip(batch, single, specs)):
            n = 7777 + k
            x = torch.rand(n, s["ch"], device="cuda") - 0.5
            yb, ys = torch.zeros(n + 4000, s["ch"], device="cuda"), torch.zeros(n + 4000, s["ch"], device="cuda")
            rb, rs = b.process_device(x, n, yb, n + 4000, 0.0), q.process_device(x, n, ys, n + 4000, 0.0)
            assert rb == rs and torch.equal(yb, ys) and b.last_gathered() == 0 and b.state() == q.state()

    batch, single = drive(32, specs, sizes, eligible={0, 1, 2, 3}, after={2: single_calls, 3: reset}, loose={3})
    finish(32, specs, batch, single)


def test_width_64_makes_matrix_calls_one_by_one():
    pytest.importorskip("torch")
    specs = [S(2, 380, 380)] * 2 + [S(8, 988, 988, policy=True, pref=0)] * 2
    sizes = [[24576, 24576, 6000, 6000], [24576, 20000, 441, 300], [10000, 24576, 441, 441]]
    batch, single = drive(64, specs, sizes, eligible={0, 1, 2, 3})
    for b in batch:
        assert b.last_gathered() == 0
    finish(64, specs, batch, single)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_gathered_round_against_the_oracle(shape):
    """not only against ourselves: the whole stream — round 1 single, later rounds gathered — inside the default-mode bar
    |y - y_precise| <= 2^-23 max (1, |y|) of the fp64-accumulating oracle, counts and position exact"""
    torch = pytest.importorskip("torch")
    spec, rounds = SHAPES[shape]
    B = A.binding(32)
    ch, T = spec["ch"], spec["T"]
    rs = [make(B, spec) for _ in range(2)]
    os_ = [OracleResampler(ch, T, spec["F"], 0.0, spec["flags"] | PRECISE, fixed=(spec["rates"][0], spec["rates"][1], 0)) for _ in range(2)]
    for o in os_:
        o.advance(T / 2)
    for rnd, k in enumerate(rounds):
        ks = [k, k + 147]
        xs = [noise(n * ch, state=(0xBA7C + 2 * (rnd * 2 + j)) | 1)[0].reshape(n, ch) for j, n in enumerate(ks)]
        caps = [int(n * max(gain(spec), 1.0) * 1.02) + 4 * T + 64 for n in ks]
        d_in = [torch.from_numpy(x).cuda() for x in xs]
        d_out = [torch.zeros(c, ch, device="cuda") for c in caps]
        got = B.process_batch_device(rs, d_in, ks, d_out, caps, [0.0, 0.0])
        for j in range(2):
            uo, go, yo = os_[j].process(xs[j], caps[j], 0.0)
            assert got[j] == (uo, go), (rnd, j, got[j], (uo, go))
            ok, worst, rms = tolerance_ok(d_out[j][:go].cpu().numpy(), np.array(yo))
            print(f"{shape} round {rnd} stream {j}: gathered {rs[j].last_gathered()}  max |err| {worst:.3e}  rms {rms:.3e}")
            assert ok, (rnd, j, worst, rms)
            assert rs[j].state()[:2] == os_[j].state()[:2], (rnd, j, rs[j].state(), os_[j].state())
            if rnd >= 1:
                assert rs[j].last_gathered() == 1 and rs[j].last_kernel() == 2, (rnd, j)


def _compiled_width(ch):
    return ch in (1, 2, 4, 8, 16, 32)


def _cut_invariance_through_the_batch(stream, rates, flush):
    """N copies of one policy stream, N different cuts, driven call after call through the batch entry (with flush: a copy's last call
    through the and-flush entry): every copy's sha256 is the one-call sha256, and the policy's fall-back count is what the same cuts give
    through single calls.  A stream of a compiled width is gathered; a stream in channel groups is asked, declines, and is made one by one."""
    import torch
    B = A.binding(32)
    ch, T, F, flags = stream
    total = 120000
    x, _ = noise(total * ch, state=0xC07B | 1)
    x = x.reshape(total, ch)
    d_x = torch.from_numpy(x).cuda()
    rng = np.random.default_rng(ch * T)
    period_in = int(round(rates[0] / np.gcd(int(rates[0]), int(rates[1]))))
    cuts = [[total], [65536, total - 65536], [16384] * (total // 16384) + [total % 16384], [4096] * (total // 4096) + [total % 4096],
            [period_in * 3] * (total // (period_in * 3)) + [total % (period_in * 3)], []]
    while sum(cuts[-1]) < total:
        cuts[-1].append(int(min(rng.integers(1, 3000), total - sum(cuts[-1]))))
    cuts = [[c for c in cs if c > 0] for cs in cuts]
    spec = S(ch, T, F, rates=rates, flags=flags, policy=True, pref=0)

    def play(batched):
        rs = [make(B, spec) for _ in cuts]
        pos, at = [0] * len(cuts), [0] * len(cuts)
        outs = [[] for _ in cuts]
        gathered = 0
        while any(a < len(c) for a, c in zip(at, cuts)):
            live = [j for j in range(len(cuts)) if at[j] < len(cuts[j])]
            ns = [cuts[j][at[j]] for j in live]
            last = [flush and at[j] == len(cuts[j]) - 1 for j in live]
            caps = [int(n * rates[1] / rates[0]) + 4000 for n in ns]
            d_in = [d_x[pos[j]:pos[j] + n] for j, n in zip(live, ns)]
            d_out = [torch.zeros(c, ch, device="cuda") for c in caps]
            res = [None] * len(live)
            for fl in (False, True):                   # the streams that end with this call go through the and-flush entry
                idx = [k for k in range(len(live)) if last[k] == fl]
                if not idx:
                    continue
                if batched:
                    fn = B.process_and_flush_batch_device if fl else B.process_batch_device
                    out = fn([rs[live[k]] for k in idx], [d_in[k] for k in idx], [ns[k] for k in idx], [d_out[k] for k in idx], [caps[k] for k in idx], [0.0] * len(idx))
                else:
                    out = [rs[live[k]].process_device(d_in[k], ns[k], d_out[k], caps[k], 0.0, and_flush=fl) for k in idx]
                for k, r in zip(idx, out):
                    res[k] = r
                    gathered += rs[live[k]].last_gathered() if not fl else 0
            for k, j in enumerate(live):
                u, g = res[k]
                assert u == ns[k], (j, at[j], u, ns[k])
                outs[j].append(d_out[k][:g].cpu().numpy().copy()); pos[j] += ns[k]; at[j] += 1
        falls = [r.cut_invariant_fallbacks() for r in rs]
        for r in rs:
            r.close()
        return [hashlib.sha256(np.concatenate(o).tobytes()).hexdigest() for o in outs], falls, gathered

    want, falls_single, _ = play(False)
    got, falls_batch, gathered = play(True)
    print(f"{ch} ch x {T} taps {rates}: gathered calls {gathered}, fall-backs {falls_batch}")
    assert len(set(want)) == 1, (ch, T, rates, want)
    assert got == want, (ch, T, rates, [a == b for a, b in zip(got, want)])
    assert falls_batch == falls_single, (ch, T, rates, falls_batch, falls_single)
    if _compiled_width(ch):
        assert gathered > 10, (ch, T, rates, gathered)
    else:
        assert gathered == 0, (ch, T, rates, gathered)


from test_gpu_cut_invariance import POLICY_STREAMS, INTERP_POLICY_STREAMS      # noqa: E402  (the neighbouring file's lists)


@pytest.mark.parametrize("stream,rates", POLICY_STREAMS, ids=[f"c{s[0]}_t{s[1]}_{int(r[0])}_{int(r[1])}" for s, r in POLICY_STREAMS])
def test_cut_invariance_through_the_batch(stream, rates):
    pytest.importorskip("torch")
    _cut_invariance_through_the_batch(stream, rates, flush=True)


@pytest.mark.parametrize("stream,rates", INTERP_POLICY_STREAMS, ids=[f"c{s[0]}_t{s[1]}x{s[2]}" for s, r in INTERP_POLICY_STREAMS])
def test_cut_invariance_through_the_batch_interpolating_stream_without_flush(stream, rates):
    """interpolating rows under the policy (the phases do not fit the filters): the same bits for any cut up to the flush, as through single calls"""
    pytest.importorskip("torch")
    _cut_invariance_through_the_batch(stream, rates, flush=False)
