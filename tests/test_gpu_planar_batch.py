"""GPU: the planar batch entries — resampleProcessBatchPlanarDevice, resampleProcessAndFlushBatchPlanarDevice and the single
resampleProcessAndFlushPlanarDevice.  Every comparison is bit for bit:

- a mixed batch over four ticks equals twin contexts driven by single resampleProcessPlanarDevice calls AND twin contexts driven by the
  interleaved batch entry on transposed copies: counts, output bits, resampleGetPosition, resampleHipLastKernel,
  resampleHipCutInvariantFallbacks — in both builds.  The buffers of the batch under test lie in one sentinel-filled slab (pitches equal to
  the frame count, frames + 5, and rows of a padded block): gaps, row padding and frames past output_generated stay untouched;
- calls above the size rule of the single planar call (staged, grouped from the second on) and one just below it (the general kernel);
- whole clips against resampleProcessAndFlushPlanarDevice twins, the interleaved flush batch and the oracle (the bars of DESIGN.md section 5,
  through the helpers of test_gpu_flush_batch.py);
- the refusals, and NULL pitch arrays."""
import ctypes as C

import numpy as np
import pytest

import audio_resampler_amd as A
import _oracle

pytestmark = pytest.mark.gpu
BH, IN, LP, EXTRAP, STRICT = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS, A.EXTRAPOLATE_ENDPOINTS, A.RESAMPLE_STRICT_ORDER
GENERAL, MFMA = 1, 2                          # resampleHipLastKernel
UP, DOWN = 48000 / 44100, 16000 / 44100
SENTINEL, GAP, ROW = -12345.5, 7, 517         # (an odd gap and an odd row: bases and planes at every alignment)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def spec(name, ch, T, flags, ticks, ratio=UP, rates=None, policy=False, pref=0, lay="pp", pad="exact", adv=None):
    """lay: layout of input and output, p(lanar) or i(nterleaved).  pad: the planar pitches — exact (the frame count / the output room),
    odd (+ 5) or rows (ROW samples: rows of a padded block)"""
    return dict(name=name, ch=ch, T=T, flags=flags, ticks=ticks, ratio=ratio, rates=rates, policy=policy, pref=pref, lay=lay, pad=pad,
                adv=T / 2 if adv is None else adv)


def make(B, s):
    r = B.Resampler(s["ch"], s["T"], s["T"], 0.0, s["flags"], None if s["rates"] is None else (s["rates"][0], s["rates"][1], 0))
    if s["pref"]:
        r.set_kernel(s["pref"])
    if s["policy"]:
        r.set_cut_invariant(True)
    r.advance(s["adv"])
    return r


def pitch_of(s, side, frames):
    if s["lay"][side] == "i":
        return 0
    return {"exact": frames, "odd": frames + 5, "rows": max(ROW, frames)}[s["pad"]]


class Slab:
    """every buffer of one batched call in one device buffer, with sentinel gaps between them; `want` is the host's picture of it.
    Planar buffers start wherever the odd gaps leave them; an interleaved one (aligned [i]) starts on a 16-byte boundary, as its twins'
    own tensors do: the matrix-core kernels choose their instantiation, and the batch what it gathers, by the alignment of interleaved frames"""
    def __init__(self, torch, sizes, tdt, dt, aligned=None):
        self.off, pos = [], GAP
        for i, n in enumerate(sizes):
            if aligned and aligned[i]:
                pos = (pos + 3) & ~3
            self.off.append(pos)
            pos += n + GAP
        self.want = np.full(pos, SENTINEL, dt)
        self.torch, self.tdt = torch, tdt

    def upload(self):
        self.buf = self.torch.from_numpy(self.want).cuda()

    def ptr(self, i):
        return self.buf.data_ptr() + self.off[i] * self.buf.element_size()


def put(want, off, pitch, x):
    """x [frames, ch] into the host picture: planes `pitch` apart, or interleaved (pitch 0)"""
    n, ch = x.shape
    if pitch:
        for c in range(ch):
            want[off + c * pitch:off + c * pitch + n] = x[:, c]
    else:
        want[off:off + n * ch] = x.reshape(-1)


def region(pitch, frames, ch):
    return ch * pitch if pitch else frames * ch


def drive(width, specs, nticks, torch, interleaved_twin=True):
    """the batch under test against its two twins, tick by tick; yields (tick, batch, single, inter contexts).  interleaved_twin False: the
    single planar calls only — a planar call the single call leaves on the general kernel although its interleaved form is big enough for the
    matrix cores has the planar call's bits, not the interleaved call's"""
    B = A.binding(width)
    L = B.lib()
    dt, tdt = (np.float32, torch.float32) if width == 32 else (np.float64, torch.float64)
    n = len(specs)
    batch, single, inter = ([make(B, s) for s in specs] for _ in range(3))
    rng = np.random.default_rng(7 + width)
    for t in range(nticks):
        frames = [s["ticks"][t] for s in specs]
        ratios = [s["ratio"] * (1 + 1e-5 * t) if s["rates"] is None and not s["policy"] and not s["pref"] else s["ratio"] for s in specs]
        caps = [int(f * r) + 8 for f, r in zip(frames, ratios)]
        x = [(0.25 * rng.standard_normal((f, s["ch"]))).astype(dt) for f, s in zip(frames, specs)]
        ip = [pitch_of(s, 0, f) for s, f in zip(specs, frames)]
        op = [pitch_of(s, 1, c) for s, c in zip(specs, caps)]
        slab = Slab(torch, [region(p, f, s["ch"]) for p, f, s in zip(ip, frames, specs)] + [region(p, c, s["ch"]) for p, c, s in zip(op, caps, specs)], tdt, dt,
                    aligned=[p == 0 for p in ip + op])
        for i in range(n):
            put(slab.want, slab.off[i], ip[i], x[i])
        slab.upload()

        # twin 1: single planar calls, the same layouts in buffers of their own
        got_single, y_single = [], []
        for i, s in enumerate(specs):
            w = np.zeros(region(ip[i], frames[i], s["ch"]), dt)
            put(w, 0, ip[i], x[i])
            d_in = torch.from_numpy(w).cuda() if w.size else torch.zeros(1, dtype=tdt, device="cuda")
            d_out = torch.zeros(max(region(op[i], caps[i], s["ch"]), 1), dtype=tdt, device="cuda")
            u, g = single[i].process_planar_device(d_in, ip[i], frames[i], d_out, op[i], caps[i], ratios[i])
            single[i].synchronize()
            y = d_out.cpu().numpy()
            y = np.stack([y[c * op[i]:c * op[i] + g] for c in range(s["ch"])], axis=1) if op[i] else y[:g * s["ch"]].reshape(g, s["ch"])
            got_single.append((u, g)); y_single.append(y)
        # twin 2: the interleaved batch entry on transposed copies
        d_xi = [torch.from_numpy(v).cuda() if v.size else torch.zeros(1, dtype=tdt, device="cuda") for v in x]
        d_yi = [torch.zeros(c, s["ch"], dtype=tdt, device="cuda") for c, s in zip(caps, specs)]
        got_inter = B.process_batch_device(inter, d_xi, frames, d_yi, caps, ratios) if interleaved_twin else None
        torch.cuda.synchronize()

        got = B.process_batch_planar_device(batch, [slab.ptr(i) for i in range(n)], ip, frames, [slab.ptr(n + i) for i in range(n)], op, caps, ratios)
        torch.cuda.synchronize()
        for i, s in enumerate(specs):
            tag = (width, t, s["name"], frames[i])
            assert got[i] == got_single[i], (tag, got[i], got_single[i])
            g = got[i][1]
            if interleaved_twin:
                assert got[i] == got_inter[i], (tag, got[i], got_inter[i])
                assert np.array_equal(bits(y_single[i]), bits(d_yi[i][:g].cpu().numpy())), tag        # (the two references agree)
            put(slab.want, slab.off[n + i], op[i], y_single[i])
            for twin in (single[i], inter[i]) if interleaved_twin else (single[i],):
                assert L.resampleGetPosition(batch[i].p) == L.resampleGetPosition(twin.p), tag
                assert batch[i].state() == twin.state(), tag
                assert batch[i].cut_invariant_fallbacks() == twin.cut_invariant_fallbacks(), tag
                assert batch[i].last_kernel() == twin.last_kernel(), (tag, batch[i].last_kernel(), twin.last_kernel())
            if interleaved_twin:
                assert batch[i].last_gathered() == inter[i].last_gathered(), (tag, batch[i].last_gathered(), inter[i].last_gathered())
        # outputs, and everything that is not output: inputs, gaps, row padding, frames past output_generated
        have = slab.buf.cpu().numpy()
        bad = np.flatnonzero(bits(have) != bits(slab.want))
        assert bad.size == 0, (width, t, bad[:8], [(s["name"], o) for s, o in zip(specs + specs, slab.off)])
        yield t, batch, single, inter


def the_mix():
    asrc = [0, 1, 63, 441]
    tick = [441] * 4
    return [
        spec("a_stereo_48_asrc_exact", 2, 48, BH | IN, asrc, pad="exact"),
        spec("a_stereo_48_asrc_odd", 2, 48, BH | IN, asrc[::-1], pad="odd"),
        spec("b_eight_380_policy_rows", 8, 380, BH | IN, tick, policy=True, rates=(44100.0, 48000.0), pad="rows"),
        spec("b_eight_380_policy_odd", 8, 380, BH | IN, tick, policy=True, rates=(44100.0, 48000.0), pad="odd"),
        spec("c_mono_156", 1, 156, BH | IN, [441, 63, 441, 1], ratio=DOWN, pad="odd"),
        spec("d_three_156", 3, 156, BH | IN, [63, 441, 441, 441], pad="rows"),
        spec("d_three_380_policy", 3, 380, BH | IN, tick, policy=True, rates=(44100.0, 48000.0), pad="odd"),
        spec("e_strict_48", 2, 48, BH | IN | STRICT, tick, ratio=DOWN, pad="odd"),
        spec("f_extrapolating_988", 2, 988, BH | IN | EXTRAP, tick, pad="rows"),          # (first output in the second tick)
        spec("f_extrapolating_380_mixed", 4, 380, BH | IN | EXTRAP, tick, lay="pi", pad="odd"),
        spec("g_interleaved_in", 2, 380, BH | IN, tick, ratio=DOWN, lay="ip", pad="odd"),
        spec("g_interleaved_out", 8, 156, BH | IN, tick, lay="pi", pad="exact"),
        spec("g_policy_interleaved_in", 8, 380, BH | IN, tick, policy=True, rates=(44100.0, 48000.0), lay="ip", pad="rows"),
        spec("g_policy_interleaved_out", 8, 380, BH | IN, tick, policy=True, rates=(44100.0, 48000.0), lay="pi", pad="exact"),
    ]


@pytest.mark.parametrize("width", [32, 64])
def test_mixed_batch_equals_the_single_planar_calls_and_the_interleaved_batch(width):
    torch = pytest.importorskip("torch")
    specs = the_mix()
    first_output = {}
    for t, batch, single, inter in drive(width, specs, 4, torch):
        for i, s in enumerate(specs):
            if s["name"].startswith("b_") and t >= 1:
                # staged at every size, in a grouped matrix-core launch from the second tick on (the 8-byte build has no streaming kernel:
                # its staged calls are made singly)
                assert batch[i].last_gathered() == (1 if width == 32 else 0), (width, t, s["name"])
                assert batch[i].last_kernel() == (MFMA if width == 32 else batch[i].last_kernel())
            if s["name"].startswith(("a_", "c_", "g_interleaved")) and s["ticks"][t] >= 63:
                assert batch[i].last_gathered() == 1 and batch[i].last_kernel() == GENERAL, (width, t, s["name"])
            if s["name"].startswith("e_"):
                assert batch[i].last_gathered() == 0, (width, t)
            if s["name"].startswith("f_") and s["name"] not in first_output and not batch[i].c.flags & 0x80:
                first_output[s["name"]] = t
    assert first_output["f_extrapolating_988"] >= 1, first_output             # (inside the run, not in its first call)


def test_calls_above_and_just_below_the_size_rule():
    """two stereo 988-tap contexts under kernel preference 6: 102,400 frames x 2 x 988 = 2.02e8 >= 2e8, staged, the second call in a grouped
    launch; 100,000 frames (1.98e8) stay planar on the general kernel, in the batch as in the single call"""
    torch = pytest.importorskip("torch")
    big = [spec("above_exact", 2, 988, BH | IN, [102400] * 2, rates=(44100.0, 48000.0), pref=6, pad="exact"),
           spec("above_odd", 2, 988, BH | IN, [102400] * 2, rates=(44100.0, 48000.0), pref=6, pad="odd")]
    for t, batch, single, inter in drive(32, big, 2, torch):
        for b, q in zip(batch, single):
            assert b.last_kernel() == q.last_kernel() == MFMA, (t, b.last_kernel(), q.last_kernel())
            assert b.last_gathered() == (1 if t else 0), t
    below = [spec("below_exact", 2, 988, BH | IN, [100000], rates=(44100.0, 48000.0), pref=6, pad="exact"),
             spec("below_odd", 2, 988, BH | IN, [100000], rates=(44100.0, 48000.0), pref=6, pad="odd")]
    for t, batch, single, inter in drive(32, below, 1, torch, interleaved_twin=False):
        for b, q in zip(batch, single):
            assert b.last_kernel() == GENERAL and q.last_kernel() == GENERAL, (b.last_kernel(), q.last_kernel())


CLIP_FRAMES = [0, 7, 300, 3000, 3000, 4000]


@pytest.mark.parametrize("ch,extrap", [(2, False), (2, True), (8, False), (8, True)])
def test_whole_clips_equal_the_single_planar_flush_the_interleaved_batch_and_the_oracle(ch, extrap):
    """clip 0 is a pure flush (NULL input, 0 frames), clip 4's output room ends inside its process call: the early return, no flush"""
    torch = pytest.importorskip("torch")
    from test_gpu_flush_batch import spec as clip, make as make_clip, make_oracle, within_bar, tonal, room_of
    B, O = A.binding(32), _oracle.binding(32)
    flags = BH | IN | (EXTRAP if extrap else 0)
    mix = [clip(f"clip{k}", ch, 380, flags, f, ratio=DOWN) for k, f in enumerate(CLIP_FRAMES)]
    n = len(mix)
    batch, single, inter = ([make_clip(B, s, None) for s in mix] for _ in range(3))
    ora = [make_oracle(O, s, 32) for s in mix]
    x = [tonal(max(s["frames"], 1), ch, np.float32, seed=40 + k)[:s["frames"]] for k, s in enumerate(mix)]
    caps = [room_of(s, s["frames"]) for s in mix]
    caps[4] = 1000                                     # (3,000 frames make 1,088 and more)
    ip = [CLIP_FRAMES[k] + (5 if k % 2 else 0) for k in range(n)]
    ip[0] = 0
    op = [c + (5 if k % 2 else 0) for k, c in enumerate(caps)]
    slab = Slab(torch, [ch * p for p in ip] + [ch * p for p in op], torch.float32, np.float32)
    for i in range(n):
        put(slab.want, slab.off[i], ip[i], x[i])
    slab.upload()
    ratios = [DOWN] * n

    want, y_single = [], []
    for i, s in enumerate(mix):
        d_in = torch.from_numpy(np.ascontiguousarray(x[i].T)).cuda() if x[i].size else None
        d_out = torch.zeros(ch, caps[i], device="cuda")
        want.append(single[i].process_and_flush_planar_device(d_in, s["frames"], s["frames"], d_out, caps[i], caps[i], DOWN))
        single[i].synchronize()
        y_single.append(np.ascontiguousarray(d_out[:, :want[i][1]].cpu().numpy().T))
    d_xi = [torch.from_numpy(v).cuda() if v.size else None for v in x]
    d_yi = [torch.zeros(c, ch, device="cuda") for c in caps]
    got_inter = B.process_and_flush_batch_device(inter, d_xi, CLIP_FRAMES, d_yi, caps, ratios)

    got = B.process_and_flush_batch_planar_device(batch, [slab.ptr(i) if CLIP_FRAMES[i] else None for i in range(n)], ip, CLIP_FRAMES,
                                                  [slab.ptr(n + i) for i in range(n)], op, caps, ratios)
    torch.cuda.synchronize()
    assert got == want == got_inter, (got, want, got_inter)
    assert got[4][1] == 1000 and got[4][0] < 3000 and not batch[4].c.flags & A.RESAMPLER_FLUSHED
    assert all(batch[i].c.flags & A.RESAMPLER_FLUSHED for i in range(n) if i != 4)
    bad = []
    for i, s in enumerate(mix):
        g = got[i][1]
        assert np.array_equal(bits(y_single[i]), bits(d_yi[i][:g].cpu().numpy())), s["name"]
        put(slab.want, slab.off[n + i], op[i], y_single[i])
        for twin in (single[i], inter[i]):
            assert batch[i].state() == twin.state() and batch[i].last_kernel() == twin.last_kernel(), s["name"]
        assert batch[i].last_gathered() == inter[i].last_gathered() == 1, s["name"]
        uo, go, yo = ora[i].process(x[i], caps[i], DOWN, and_flush=True)
        assert got[i] == (uo, go), (s["name"], got[i], (uo, go))
        if go:
            ok, worst = within_bar(s, 32, y_single[i], np.asarray(yo))
            print(f"{ch} ch extrapolating {extrap} {s['name']} frames {go}: {'ok' if ok else 'OUT OF BAR'} worst {worst}")
            if not ok:
                bad.append((s["name"], worst))
    assert not bad, bad
    have = slab.buf.cpu().numpy()
    assert np.array_equal(bits(have), bits(slab.want)), np.flatnonzero(bits(have) != bits(slab.want))[:8]


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("entry", ["resampleProcessBatchPlanarDevice", "resampleProcessAndFlushBatchPlanarDevice"])
def test_refusals_enqueue_nothing_and_null_pitches_are_the_interleaved_entry(width, entry):
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    L = B.lib()
    fn, twin_fn = getattr(L, entry), getattr(L, entry.replace("Planar", "Interleaved"))
    dt, tdt = (np.float32, torch.float32) if width == 32 else (np.float64, torch.float64)
    ch, T = 2, 380
    rs, twins = ([B.Resampler(ch, T, T, 0.0, BH | IN | EXTRAP) for _ in range(3)] for _ in range(2))
    for r in rs + twins:
        r.advance(T / 2)
    x = torch.from_numpy((0.25 * np.random.default_rng(3).standard_normal((2000, ch))).astype(dt)).cuda()
    ys, yt = ([torch.full((4000, ch), SENTINEL, dtype=tdt, device="cuda") for _ in range(3)] for _ in range(2))
    states, errors = [r.state() for r in rs], L.artamdErrorCount()
    res, res_t = (B.ResampleResult * 3)(), (B.ResampleResult * 3)()
    arr = lambda ps: (C.c_void_p * 3)(*ps)
    ins, outs, outs_t = arr([x.data_ptr()] * 3), arr([y.data_ptr() for y in ys]), arr([y.data_ptr() for y in yt])
    nin, caps, ratios = (C.c_int * 3)(2000, 2000, 2000), (C.c_int * 3)(4000, 4000, 4000), (C.c_double * 3)(UP, UP, UP)
    pitch = (C.c_long * 3)(2000, 2000, 2000)
    p = [C.cast(r.p, C.c_void_p).value for r in rs]
    assert fn(arr(p), 0, ins, pitch, nin, outs, pitch, caps, ratios, res) == 0
    assert fn(arr(p), -1, ins, pitch, nin, outs, pitch, caps, ratios, res) == 0
    assert fn(arr([p[0], p[1], p[0]]), 3, ins, pitch, nin, outs, pitch, caps, ratios, res) == -1
    assert fn(arr([p[0], None, p[2]]), 3, ins, None, nin, outs, None, caps, ratios, res) == -1
    torch.cuda.synchronize()
    assert [r.state() for r in rs] == states
    assert all(bool((y == SENTINEL).all()) for y in ys)
    assert L.artamdErrorCount() == errors
    # NULL pitch arrays: the interleaved entry, bit for bit
    assert fn(arr(p), 3, ins, None, nin, outs, None, caps, ratios, res) == 0
    assert twin_fn(arr([C.cast(r.p, C.c_void_p).value for r in twins]), 3, ins, nin, outs_t, caps, ratios, res_t) == 0
    torch.cuda.synchronize()
    for i in range(3):
        assert (res[i].input_used, res[i].output_generated) == (res_t[i].input_used, res_t[i].output_generated) and res[i].input_used == 2000
        assert np.array_equal(bits(ys[i].cpu().numpy()), bits(yt[i].cpu().numpy())), i
        assert rs[i].state() == twins[i].state() and rs[i].last_gathered() == twins[i].last_gathered() == 1
