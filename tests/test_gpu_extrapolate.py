"""GPU: the end-point LPC extrapolation on the device.

- artamdExtrapolateBatchDevice against the reference's extrapolate_forward / extrapolate_reverse (tests/golden/extrapolate.npz): every
  case in ONE launch, mixed counts and directions, strides 1 and C (a channel of an interleaved buffer), both widths;
- the resampler end to end on TONAL input in strict mode against the oracle, bit for bit (its fits are the long ones);
- extrapolating streams inside resampleProcessBatchInterleavedDevice / resampleProcessScheduleInterleavedDevice: gathered, and equal
  to their single-call twins."""
import numpy as np
import pytest

import audio_resampler_amd as A
import _extrapolate as X
import _oracle

pytestmark = pytest.mark.gpu
BH, IN, LP, EXTRAP, STRICT = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS, A.EXTRAPOLATE_ENDPOINTS, A.RESAMPLE_STRICT_ORDER
PREFILL = 0x80                               # (resampler.h: set until an extrapolating stream's first output)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _launch(width, cases, stride):
    """cases: (known, extras, backward).  One call; every run's input and output live in one device buffer each, `stride` apart, with
    NaN between them (never read) and a sentinel around each output (never written).  Returns the outputs."""
    torch = pytest.importorskip("torch")
    dt = X.dtype(width)
    in_len = sum(len(k) * stride + 8 for k, _, _ in cases)
    out_len = sum(e * stride + 8 for _, e, _ in cases)
    h_in = np.full(in_len, np.nan, dt)
    sentinel = dt(-12345.5)
    h_out = np.full(out_len, sentinel, dt)
    ins, outs, pos_in, pos_out = [], [], 0, 0
    for known, e, _ in cases:
        h_in[pos_in:pos_in + len(known) * stride:stride] = known
        ins.append(pos_in); outs.append(pos_out)
        pos_in += len(known) * stride + 8; pos_out += e * stride + 8
    d_in = torch.from_numpy(h_in).cuda()
    d_out = torch.from_numpy(h_out).cuda()
    size = h_in.itemsize
    B = A.binding(width)
    B.extrapolate_batch_device([d_in.data_ptr() + p * size for p in ins], [len(k) for k, _, _ in cases], [stride] * len(cases),
                               [b for _, _, b in cases], [d_out.data_ptr() + p * size for p in outs], [e for _, e, _ in cases])
    torch.cuda.synchronize()
    got = d_out.cpu().numpy()
    res, mask = [], np.ones(out_len, bool)
    for (known, e, _), p in zip(cases, outs):
        res.append(got[p:p + e * stride:stride].copy())
        mask[p:p + e * stride:stride] = False
    assert np.array_equal(bits(got[mask]), bits(np.full(mask.sum(), sentinel, dt))), "a run wrote outside its output"
    return res


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("stride", [1, 3])
def test_every_golden_case_bit_for_bit_in_one_launch(width, stride):
    g = np.load(X.GOLDEN)
    cases, keys = [], []
    for kind in X.KINDS:
        for count in X.COUNTS:
            for backward in (False, True):
                known = X.place(kind, count, width, backward)
                for e in X.extras_of(count):
                    cases.append((known, e, backward)); keys.append((X.key(width, kind, count, backward), e))
    got = _launch(width, cases, stride)
    bad = []
    for (k, e), y in zip(keys, got):
        longest = max(X.extras_of(int(k.split("/")[2])))
        ok = X.digest(y) == g[f"{k}/{e}"] and np.array_equal(bits(y[:X.HEAD]), bits(g[k + "/head"][:e]))
        if e == longest:
            ok = ok and np.array_equal(bits(y[-X.TAIL:]), bits(g[k + "/tail"]))
        if not ok:
            bad.append((k, e))
    assert not bad, f"{len(bad)} of {len(keys)} runs differ from the reference: {bad[:8]}"


@pytest.mark.ref
@pytest.mark.parametrize("width", [32, 64])
def test_fresh_tonal_runs_against_the_reference(width):
    if not X.ref_available(width):
        pytest.skip("oracle/_ref (the reference built by oracle/Makefile) is not here")
    R = X.RefExtrapolator(width)
    rng = np.random.default_rng(2024 + width)
    cases = []
    for i in range(48):
        count = int(rng.integers(8, 1024))
        n = np.arange(count)
        x = sum(rng.uniform(0.05, 0.6) * np.sin(2 * np.pi * rng.uniform(0.0005, 0.2) * n + rng.uniform(0, 6.3)) for _ in range(rng.integers(1, 4)))
        x = (x + rng.uniform(0, 1e-3) * rng.standard_normal(count)).astype(X.dtype(width))
        cases.append((x, int(rng.integers(1, 1100)), bool(i % 2)))
    got = _launch(width, cases, 1)
    for i, ((x, e, b), y) in enumerate(zip(cases, got)):
        assert np.array_equal(bits(y), bits(R.run(x, e, b))), (i, len(x), e, b)


# ---- the resampler end to end, strict order, tonal input ---------------------------------------------------------------------------

def tonal(frames, ch, width, seed=1):
    rng = np.random.default_rng(seed)
    n = np.arange(frames)[:, None]
    f = rng.uniform(0.001, 0.05, (1, ch))
    x = 0.5 * np.sin(2 * np.pi * f * n + rng.uniform(0, 6.3, (1, ch))) + 0.2 * np.sin(2 * np.pi * 3.1 * f * n)
    return np.ascontiguousarray((x + 1e-4 * rng.standard_normal((frames, ch))).astype(X.dtype(width)))


# name: (ctor args, ctor kw, advance, blocks of the session, then a flush)
SESSIONS = {
    "art_8ch_988": ((8, 988, 988), dict(flags=BH | IN | LP | EXTRAP, fixed=(44100.0, 48000.0, 0)), 494.0, [700, 3000, 2200]),
    "first_inside_a_call": ((2, 380, 380, 0.0, BH | IN | EXTRAP), {}, 190.0, [120, 50, 2600, 900]),
    "first_by_the_flush": ((2, 380, 380, 0.0, BH | IN | EXTRAP), {}, 190.0, [150]),
    "first_by_the_flush_fixed": ((3, 156, 320), dict(flags=BH | IN | LP | EXTRAP, fixed=(96000.0, 44100.0, 0)), 78.0, [60]),
    "first_after_a_rewind": ((2, 380, 380, 0.0, BH | IN | EXTRAP), {}, 190.0 + 15 * 380 + 100, [8000, 1500]),
}


def _session(make, x, blocks, ratio, cap):
    outs, pos = [], 0
    for n in blocks:
        u, g, y = make.process(x[pos:pos + n], cap, ratio)
        outs.append((u, g, y.copy()))
        pos += n
    u, g, y = make.process(None, cap, ratio, flush=True)
    outs.append((u, g, y.copy()))
    return outs


def _compare(gpu_outs, ora_outs):
    assert [o[:2] for o in gpu_outs] == [o[:2] for o in ora_outs]
    for k, (a, b) in enumerate(zip(gpu_outs, ora_outs)):
        assert np.array_equal(bits(a[2]), bits(b[2])), k


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_resampler_strict_tonal_equals_the_oracle(width, name):
    args, kw, adv, blocks = SESSIONS[name]
    B, O = A.binding(width), _oracle.binding(width)
    ch = args[0]
    x = tonal(sum(blocks), ch, width)
    ratio = 48000 / 44100 if "fixed" not in kw else kw["fixed"][1] / kw["fixed"][0]
    cap = int(sum(blocks) * ratio) + 4 * args[1]
    gkw = dict(kw)
    if "flags" in gkw:
        gkw["flags"] |= STRICT
        gargs = args
    else:
        gargs = args[:4] + (args[4] | STRICT,)
    gpu, ora = B.Resampler(*gargs, **gkw), O.OracleResampler(*args, **kw)
    gpu.advance(adv); ora.advance(adv)
    _compare(_session(gpu, x, blocks, ratio, cap), _session(ora, x, blocks, ratio, cap))


@pytest.mark.parametrize("width", [32, 64])
def test_planar_input_strict_tonal_equals_the_oracle(width):
    torch = pytest.importorskip("torch")
    B, O = A.binding(width), _oracle.binding(width)
    ch, T, ratio = 4, 380, 44100 / 48000
    blocks = [100, 1700, 1200]
    x = tonal(sum(blocks), ch, width, seed=5)
    tdt = torch.float32 if width == 32 else torch.float64
    gpu, ora = B.Resampler(ch, T, T, 0.0, BH | IN | EXTRAP | STRICT), O.OracleResampler(ch, T, T, 0.0, BH | IN | EXTRAP)
    gpu.advance(T / 2); ora.advance(T / 2)
    want = _session(ora, x, blocks, ratio, 4000)
    pos = 0
    for k, n in enumerate(blocks):
        planes = torch.from_numpy(np.ascontiguousarray(x[pos:pos + n].T)).cuda()          # [ch][n]
        d_out = torch.zeros(4000, ch, dtype=tdt, device="cuda")
        u, g = gpu.process_planar_device(planes, n, n, d_out, 0, 4000, ratio)
        assert (u, g) == want[k][:2], k
        assert np.array_equal(bits(d_out[:g].cpu().numpy()), bits(want[k][2])), k
        pos += n


def test_sharded_context_strict_tonal_equals_the_oracle(monkeypatch):
    monkeypatch.setenv("ARTAMD_SHARDS", "4")
    B, O = A.binding(32), _oracle.binding(32)
    ch, T, ratio = 8, 988, 48000 / 44100
    blocks = [600, 2500]
    x = tonal(sum(blocks), ch, 32, seed=9)
    gpu = B.Resampler(ch, T, T, 0.0, BH | IN | EXTRAP | STRICT | A.RESAMPLE_MULTITHREADED)
    ora = O.OracleResampler(ch, T, T, 0.0, BH | IN | EXTRAP)
    assert len(gpu.shards()) == 4
    gpu.advance(T / 2); ora.advance(T / 2)
    _compare(_session(gpu, x, blocks, ratio, 6000), _session(ora, x, blocks, ratio, 6000))


# ---- sharing launches ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [32, 64])
def test_batch_gathers_extrapolating_streams_and_equals_single_calls(width):
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    tdt = torch.float32 if width == 32 else torch.float64
    # (channels, taps, flags, ratio, advance); the extrapolating streams' first outputs come in different calls
    streams = [(8, 988, BH | IN | EXTRAP, 1.0884317, 494.0), (2, 380, BH | IN | EXTRAP, 0.731, 190.0),
               (2, 48, BH | IN, 1.25, 24.0), (3, 156, BH | IN | EXTRAP, 2.0, 78.0), (1, 64, BH, 0.5, 0.0)]
    mk = lambda s: B.Resampler(s[0], s[1], s[1], 0.0, s[2])
    batch, single = [mk(s) for s in streams], [mk(s) for s in streams]
    for r, s in zip(batch + single, streams + streams):
        r.advance(s[4])
    x = [torch.from_numpy(tonal(20000, s[0], width, seed=i)).cuda() for i, s in enumerate(streams)]
    caps = [8000] * len(streams)
    d_b = [torch.zeros(8000, s[0], dtype=tdt, device="cuda") for s in streams]
    d_s = [torch.zeros(8000, s[0], dtype=tdt, device="cuda") for s in streams]
    rounds = [[300, 200, 500, 100, 700], [2000, 700, 900, 300, 100], [1500, 1500, 40, 2000, 1000], [900, 20, 800, 700, 1200]]
    pos = [0] * len(streams)
    firsts, later = set(), set()
    for rnd, n_in in enumerate(rounds + [[-1] * len(streams)]):
        flush = n_in[0] < 0
        d_in = [x[i][pos[i]:] for i in range(len(streams))]
        prefill = [bool(r.c.flags & PREFILL) for r in single]
        got = B.process_batch_device(batch, d_in, n_in, d_b, caps, [s[3] for s in streams])
        for i, s in enumerate(streams):
            u, g = single[i].process_device(d_in[i], n_in[i], d_s[i], caps[i], s[3])
            assert got[i] == (u, g), (rnd, i)
            assert np.array_equal(bits(d_b[i][:g].cpu().numpy()), bits(d_s[i][:g].cpu().numpy())), (rnd, i)
            assert batch[i].state() == single[i].state(), (rnd, i)
            assert batch[i].last_kernel() == single[i].last_kernel(), (rnd, i)
            assert single[i].last_gathered() == 0
            if s[2] & EXTRAP:
                if flush:
                    assert batch[i].last_gathered() == 0, (rnd, i)
                elif g:
                    assert batch[i].last_gathered() == 1, (rnd, i, prefill[i])
                    (firsts if prefill[i] else later).add(i)
            if not flush:
                pos[i] += u
    extrap = {i for i, s in enumerate(streams) if s[2] & EXTRAP}
    assert firsts == extrap and later == extrap, (firsts, later)


@pytest.mark.parametrize("width", [32, 64])
def test_schedule_gathers_an_extrapolating_streams_later_blocks(width):
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    tdt = torch.float32 if width == 32 else torch.float64
    ch, T = 2, 256
    blocks = [600, 3000, 4096, 2048, 4096]
    ratios = [48000 / 44100 * (1 + 50e-6 * k) for k in range(len(blocks))]
    caps = [int(n * r) + 64 for n, r in zip(blocks, ratios)]
    x = torch.from_numpy(tonal(sum(blocks), ch, width, seed=3)).cuda()
    sched, loop = B.Resampler(ch, T, T, 0.0, BH | IN | EXTRAP), B.Resampler(ch, T, T, 0.0, BH | IN | EXTRAP)
    sched.advance(T / 2); loop.advance(T / 2)
    d_a = torch.zeros(sum(caps), ch, dtype=tdt, device="cuda")
    d_b = torch.zeros(sum(caps), ch, dtype=tdt, device="cuda")
    # the first output's block runs as its single call; the blocks after it are one launch
    made, res = sched.process_schedule_device(x, blocks[:1], d_a, caps[:1], ratios[:1])
    assert made == 1 and sched.last_gathered() == 0
    made2, res2 = sched.process_schedule_device(x[blocks[0]:], blocks[1:], d_a[res[0][1]:], caps[1:], ratios[1:])
    assert made2 == len(blocks) - 1 and sched.last_gathered() == 1
    want, pos, opos = [], 0, 0
    for n, c, r in zip(blocks, caps, ratios):
        want.append(loop.process_device(x[pos:], n, d_b[opos:], c, r))
        pos += n; opos += want[-1][1]
    assert res + res2 == want
    total = sum(g for _, g in want)
    assert np.array_equal(bits(d_a[:total].cpu().numpy()), bits(d_b[:total].cpu().numpy()))
    assert sched.state() == loop.state()
