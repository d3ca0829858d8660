"""biquadBankApplyPlanarDevice, biquadBankApplyBatchPlanarDevice, biquadBankReset and ClipFilter: channels-first device buffers
through the biquad banks, in place.  Everything is bit-exact: the twin of a planar call is the interleaved entry on a transposed copy
(which test_gpu_biquad_parallel.py and test_gpu_biquad_batch.py pin to the oracle), and the comparison is equality of bytes and of
the state biquadBankRead returns (x, y, index of every section)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import audio_resampler_amd as A
import test_gpu_biquad_batch as TB
from _oracle import load_oracle, Biquad as OBiquad, BiquadCoeffs as OCoeffs, f32p

pytestmark = pytest.mark.gpu

SENTINEL = 12345.5
FRONT = 4                                       # sentinel samples in front of a buffer (a multiple of 16 bytes in both builds)
WIDE = 0.25                                     # a wide low-pass: forgets its state within a few dozen frames
FLOOR = 128                                     # the chunk length under ARTAMD_BIQUAD_WARMUP=2 (pcm_host.c, spec_chunk: 4 * S * 2 < 128)
CHANNELS = [1, 2, 3, 8, 33, 70]                 # 70: past one 64-lane workgroup
KINDS = ["one", "art", "chain4"]
FRAMES = [1, 3, 63, 64, 2 * FLOOR - 1, 2 * FLOOR, 2 * FLOOR + 5]
LAYOUTS = [("dense", 0, 0), ("plus1", 1, 0), ("plus7", 7, 0), ("offset", 2, 1)]      # (name, pitch - frames, base offset in samples)
_bits, _state = TB._bits, TB._state


def _width(M):
    return getattr(M, "width", 32)                # (the package itself is the 4-byte binding)


def _dtype(M):
    return torch.float64 if _width(M) == 64 else torch.float32


def _sections(M, ch, kind):
    """(M.Biquad * (ch * S), S).  'one': one order-2 low-pass; 'art': ART's -p, two of them; 'chain4': orders 1, 2, 3 and 4 in a row,
    hand-filled stable coefficients; 'pre': ART's pre-filter at its real cut-off.  Channels differ a little, so that a mixed-up
    plane shows."""
    L = M.lib()
    S = {"one": 1, "art": 2, "chain4": 4, "pre": 2}[kind]
    secs = (M.Biquad * (ch * S))()
    for c in range(ch):
        for s in range(S):
            if kind == "chain4":
                co = M.BiquadCoefficients(**TB.HAND[s + 1])
            else:
                co = M.BiquadCoefficients()
                L.biquad_lowpass(C.byref(co), TB.PRE if kind == "pre" else WIDE - 0.01 * (c % 3))
            L.biquad_init(C.byref(secs[c * S + s]), C.byref(co), 1.0 - 0.02 * (c % 4) if kind == "chain4" else 1.0)
    return secs, S


def _bank(M, ch, kind, multi=False):
    secs, S = _sections(M, ch, kind)
    return M.BiquadBank(secs, ch, S, multi=multi)


class Planes:
    """a channels-first clip in a sentinel-filled device buffer: FRONT + offset sentinels, then ch planes `pitch` apart"""
    def __init__(self, x, pitch, offset=0):
        ch, frames = x.shape
        self.frames, self.at = frames, FRONT + offset
        self.buf = torch.full((self.at + ch * pitch + FRONT,), SENTINEL, dtype=x.dtype, device="cuda")
        self.rows = self.buf[self.at:self.at + ch * pitch].view(ch, pitch)
        self.rows[:, :frames] = x
        self.pitch = pitch

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.at * self.buf.element_size()

    def clip(self):
        return self.rows[:, :self.frames]

    def padding_untouched(self):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        mask[self.at:self.at + self.rows.numel()].view_as(self.rows)[:, :self.frames] = False
        return bool(torch.all(self.buf[mask] == SENTINEL))


def _signal(ch, frames, seed, dtype):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(ch, max(frames, 1), generator=g, device="cuda", dtype=dtype)[:, :frames] * 2 - 1


def _twin(bank, x):
    """the interleaved entry on the transposed clip x [ch, frames], transposed back"""
    t = x.t().contiguous()
    bank.apply_device(t, x.shape[1])
    return t.t()


def _single_equals_twin(M, monkeypatch, ch, kind, frames, layout, seed):
    """the planar call on a bank whose time-parallel form has chunks of FLOOR frames (warm-up forced to 2 frames: from 2 * FLOOR
    frames on nearly every chunk is repaired) against the interleaved call on a bank with the filter's own warm-up"""
    _, extra, offset = layout
    monkeypatch.setenv("ARTAMD_BIQUAD_WARMUP", "2")
    bank = _bank(M, ch, kind)
    monkeypatch.delenv("ARTAMD_BIQUAD_WARMUP")
    twin = _bank(M, ch, kind)
    x = _signal(ch, frames, seed, _dtype(M))
    p = Planes(x, frames + extra, offset)
    bank.apply_planar_device(p.ptr, p.pitch, frames)
    want = _twin(twin, x)
    torch.cuda.synchronize()
    what = (_width(M), ch, kind, frames, layout)
    assert torch.equal(_bits(p.clip()), _bits(want)), what
    assert p.padding_untouched(), what
    assert _state(bank) == _state(twin), what
    # the form the call took: the serial forms repair nothing; the time-parallel form starts at 2 chunks, and 2 frames of warm-up fail
    assert (bank.repairs() > 0) == (frames >= 2 * FLOOR), what
    bank.close(); twin.close()


def _grid():
    return [(ch, kind, frames, layout) for kind in KINDS for ch in CHANNELS for frames in FRAMES for layout in LAYOUTS]


def test_the_grid_has_every_axis():
    grid = _grid()
    assert {g[0] for g in grid} == {1, 2, 3, 8, 33, 70}
    assert {g[1] for g in grid} == {"one", "art", "chain4"}
    assert {g[2] for g in grid} == {1, 3, 63, 64, 2 * FLOOR - 1, 2 * FLOOR, 2 * FLOOR + 5}
    assert {(g[3][1], g[3][2]) for g in grid} >= {(0, 0), (1, 0), (7, 0)} and any(g[3][2] == 1 for g in grid)
    secs, S = _sections(A, 2, "chain4")
    assert S == 4 and [secs[s].order for s in range(4)] == [1, 2, 3, 4]
    assert [_sections(A, 2, k)[1] for k in ("one", "art")] == [1, 2] and _sections(A, 2, "art")[0][1].order == 2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ch", CHANNELS)
def test_single_call_equals_twin(monkeypatch, kind, ch):
    for k, (c, kd, frames, layout) in enumerate(g for g in _grid() if g[0] == ch and g[1] == kind):
        _single_equals_twin(A, monkeypatch, c, kd, frames, layout, 1000 * ch + k)


@pytest.mark.parametrize("kind,frames", [("one", 2000), ("art", 2000), ("pre", 4001), ("chain4", 6000)])
def test_long_calls_with_the_filters_own_warm_up(kind, frames):
    """no override: the warm-up and the chunk length are the filter's own (the time-parallel form where its single call takes it)"""
    for ch, extra, offset in ((2, 1, 0), (33, 0, 1), (3, 6, 0)):
        bank, twin = _bank(A, ch, kind), _bank(A, ch, kind)
        x = _signal(ch, frames, frames + ch, torch.float32)
        p = Planes(x, frames + extra, offset)
        bank.apply_planar_device(p.ptr, p.pitch, frames)
        want = _twin(twin, x)
        torch.cuda.synchronize()
        assert torch.equal(_bits(p.clip()), _bits(want)), (kind, ch)
        assert p.padding_untouched() and _state(bank) == _state(twin), (kind, ch)
        assert bank.repairs() == twin.repairs(), (kind, ch)
        bank.close(); twin.close()


CHILD = """
import sys
import numpy as np, torch
import audio_resampler_amd as A
sys.path.insert(0, sys.argv[1])
import test_gpu_biquad_planar as T
x = torch.from_numpy(np.load(sys.argv[2])).cuda()
bank = T._bank(A, x.shape[0], "art")
p = T.Planes(x, x.shape[1] + 3)
bank.apply_planar_device(p.ptr, p.pitch, x.shape[1])
torch.cuda.synchronize()
assert p.padding_untouched() and bank.repairs() == 0
np.save(sys.argv[3], p.clip().cpu().numpy())
open(sys.argv[3] + ".state", "wb").write(T._state(bank))
"""


def test_time_parallel_planar_form_ran_and_its_repairs_are_exact(monkeypatch, tmp_path):
    ch, frames = 8, 4 * FLOOR + 37
    monkeypatch.setenv("ARTAMD_BIQUAD_WARMUP", "2")
    bank = _bank(A, ch, "art")
    monkeypatch.delenv("ARTAMD_BIQUAD_WARMUP")
    twin = _bank(A, ch, "art")
    x = _signal(ch, frames, 77, torch.float32)
    p = Planes(x, frames + 3)
    bank.apply_planar_device(p.ptr, p.pitch, frames)
    want = _twin(twin, x)
    torch.cuda.synchronize()
    assert bank.repairs() > 0 and twin.repairs() == 0          # chunks of FLOOR frames, a warm-up far too short: repaired
    assert torch.equal(_bits(p.clip()), _bits(want)) and p.padding_untouched()
    assert _state(bank) == _state(twin)
    # the serial forms: ARTAMD_BIQUAD_SERIAL is read once per process, so a process of its own
    src, dst = str(tmp_path / "x.npy"), str(tmp_path / "y.npy")
    np.save(src, x.cpu().numpy())
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, ARTAMD_BIQUAD_SERIAL="1", PYTHONPATH=os.pathsep.join([os.path.dirname(here)] + sys.path))
    env.pop("ARTAMD_BIQUAD_WARMUP", None)
    done = subprocess.run([sys.executable, "-c", CHILD, here, src, dst], env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    assert np.array_equal(np.load(dst).view(np.uint32), want.cpu().numpy().view(np.uint32))
    assert open(dst + ".state", "rb").read() == _state(twin)
    bank.close(); twin.close()


@pytest.mark.parametrize("first", [0, 1])
def test_streaming_alternates_planar_and_interleaved_calls(first):
    """one signal cut into calls, planar and interleaved by turns on one bank, against a bank fed the same cuts interleaved only"""
    ch, cuts = 3, [40, 700, 1, 64, 1000]
    mixed, plain = _bank(A, ch, "art"), _bank(A, ch, "art")
    x = _signal(ch, sum(cuts), 5, torch.float32)
    pos = 0
    for k, n in enumerate(cuts):
        part = x[:, pos:pos + n]
        want = _twin(plain, part)
        if k % 2 == first:
            p = Planes(part, n + 1 + k, offset=k % 2)
            mixed.apply_planar_device(p.ptr, p.pitch, n)
            got = p.clip()
        else:
            got = _twin(mixed, part)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got), _bits(want)), (first, k)
        assert _state(mixed) == _state(plain), (first, k)
        pos += n
    mixed.close(); plain.close()


def test_art_low_pass_on_a_channels_first_clip_against_the_oracle():
    """ART's two-section pre-filter on an 8-channel [C, T] clip; every plane against the reference's recurrence"""
    OL = load_oracle()
    ch, frames = 8, 4001
    co, oc = A.BiquadCoefficients(), OCoeffs()
    A.lib().biquad_lowpass(C.byref(co), TB.PRE)
    OL.ora_biquad_lowpass(C.byref(oc), TB.PRE)
    secs = (A.Biquad * (ch * 2))()
    osecs = [OBiquad() for _ in range(ch * 2)]
    for k in range(ch * 2):
        A.lib().biquad_init(C.byref(secs[k]), C.byref(co), 1.0)
        OL.ora_biquad_init(C.byref(osecs[k]), C.byref(oc), 1.0)
    bank = A.BiquadBank(secs, ch, 2)
    x = np.ascontiguousarray(np.random.default_rng(31).random((ch, frames), dtype=np.float32) * 2 - 1)
    p = Planes(torch.from_numpy(x.copy()).cuda(), frames + 5)
    bank.apply_planar_device(p.ptr, p.pitch, frames)
    for c in range(ch):
        for s in range(2):
            OL.ora_biquad_buffer(C.byref(osecs[c * 2 + s]), C.cast(x.ctypes.data + 4 * frames * c, f32p), frames, 1)
    torch.cuda.synchronize()
    assert np.array_equal(p.clip().cpu().numpy().view(np.uint32), x.view(np.uint32))
    assert p.padding_untouched()
    hist = lambda q, arr: [arr[(q.index - i) & 3] for i in range(4)]
    st = bank.read()
    for k in range(ch * 2):
        assert hist(st[k], st[k].x) == hist(osecs[k], osecs[k].x) and hist(st[k], st[k].y) == hist(osecs[k], osecs[k].y)
    bank.close()


# ---- the batch entry -------------------------------------------------------------------------------------------------------------

def _batch_specs(M):
    """planar and interleaved items, section counts 1, 2 and 4, 1 to 512 frames, one call above the library's bound that its single
    call makes time-parallel (on the side), one empty"""
    over = max(TB._serial_max(M) + 1, 1300)
    rows = [(2, "art", 441, True), (3, "one", 1, True), (8, "chain4", 512, True), (2, "art", 300, False), (33, "one", 64, True),
            (1, "art", 77, True), (2, "art", over, True), (6, "chain4", 63, False), (5, "art", 0, True), (70, "one", 129, True),
            (4, "one", 512, False), (2, "chain4", 3, True)]
    return [dict(ch=c, kind=k, frames=f, planar=p, extra=(3 * i) % 8, offset=i % 2) for i, (c, k, f, p) in enumerate(rows)]


def _with_lanes(M, lanes):
    fn = M.lib().artamd_biquad_batch_planar
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]

    def call(banks, bufs, pitches, frames):
        n = len(banks)
        rc = fn((C.c_void_p * n)(*[b.p for b in banks]), n, (C.c_void_p * n)(*[int(p) for p in bufs]),
                (C.c_long * n)(*[int(p) for p in pitches]), (C.c_int * n)(*[int(f) for f in frames]), lanes, -1)
        assert rc >= 0
        return rc
    return call


def _batch_equals_loop(M, specs, batch_call=None, ticks=2):
    """the batch entry on one set of banks, the loop of single planar calls on a second, the interleaved batch entry on transposed
    copies on a third: equal bytes and states, tick after tick (the state carries), and the two batch entries' return values equal"""
    batch_call = batch_call or M.biquad_batch_planar_device
    dtype = _dtype(M)
    sets = [[_bank(M, s["ch"], s["kind"]) for s in specs] for _ in range(3)]
    frames = [s["frames"] for s in specs]
    for tick in range(ticks):
        xs = [_signal(s["ch"], s["frames"], 100 * tick + i, dtype) for i, s in enumerate(specs)]

        def lay(i):                             # item i's buffer: planes, or interleaved frames between sentinels (one plane, transposed)
            s = specs[i]
            if s["planar"]:
                return Planes(xs[i], s["frames"] + s["extra"], s["offset"])
            return Planes(xs[i].t().contiguous().view(1, -1), s["frames"] * s["ch"], s["offset"])
        pitch = lambda i, p: p.pitch if specs[i]["planar"] else 0
        mine, loop = [lay(i) for i in range(len(specs))], [lay(i) for i in range(len(specs))]
        rc = batch_call(sets[0], [p.ptr for p in mine], [pitch(i, p) for i, p in enumerate(mine)], frames)
        for i, p in enumerate(loop):
            sets[1][i].apply_planar_device(p.ptr, pitch(i, p), frames[i])
        turned = [x.t().contiguous() for x in xs]
        assert rc == M.biquad_batch_device(sets[2], turned, frames), tick
        torch.cuda.synchronize()
        for i, s in enumerate(specs):
            assert mine[i].padding_untouched() and loop[i].padding_untouched(), (tick, s)
            assert torch.equal(_bits(mine[i].buf), _bits(loop[i].buf)), (tick, s)
            got = mine[i].clip() if s["planar"] else mine[i].clip().view(s["frames"], s["ch"]).t()
            assert torch.equal(_bits(got), _bits(turned[i].t())), (tick, s)
            assert _state(sets[0][i]) == _state(sets[1][i]) == _state(sets[2][i]), (tick, s)
    for b in sum(sets, []):
        b.close()


def test_mixed_batch_equals_the_loop_of_single_planar_calls():
    specs = _batch_specs(A)
    assert {_sections(A, 1, s["kind"])[1] for s in specs} == {1, 2, 4} and {s["planar"] for s in specs} == {True, False}
    assert min(s["frames"] for s in specs if s["frames"]) == 1 and sum(s["frames"] > TB._serial_max(A) for s in specs) == 1
    _batch_equals_loop(A, specs, ticks=3)


@pytest.mark.parametrize("lanes", [1, 8, 64])
def test_forced_lane_counts_equal_the_loop(lanes):
    _batch_equals_loop(A, _batch_specs(A), _with_lanes(A, lanes))


def test_pitches_none_is_the_interleaved_entry():
    specs = [dict(ch=2, kind="art", frames=441), dict(ch=6, kind="chain4", frames=64)]
    banks, twins = [_bank(A, s["ch"], s["kind"]) for s in specs], [_bank(A, s["ch"], s["kind"]) for s in specs]
    xs = [_signal(s["ch"], s["frames"], 9 + i, torch.float32).t().contiguous() for i, s in enumerate(specs)]
    ys = [x.clone() for x in xs]
    frames = [s["frames"] for s in specs]
    assert A.biquad_batch_planar_device(banks, xs, None, frames) == A.biquad_batch_device(twins, ys, frames) == 2
    torch.cuda.synchronize()
    for x, y, b, t in zip(xs, ys, banks, twins):
        assert torch.equal(_bits(x), _bits(y)) and _state(b) == _state(t)
        b.close(); t.close()


def test_batch_edges_empty_duplicate_and_null():
    """refusals the host makes before any launch: nothing is written and no failure is counted"""
    L = A.lib()
    assert L.biquadBankApplyBatchPlanarDevice(None, 0, None, None, None) == 0
    specs = [dict(ch=2, kind="art", frames=441), dict(ch=6, kind="one", frames=300)]
    banks = [_bank(A, s["ch"], s["kind"]) for s in specs]
    ps = [Planes(_signal(s["ch"], s["frames"], i, torch.float32), s["frames"] + 2) for i, s in enumerate(specs)]
    before = [p.buf.clone() for p in ps]
    frames, pitches, ptrs = [s["frames"] for s in specs], [p.pitch for p in ps], [p.ptr for p in ps]
    assert A.biquad_batch_planar_device(banks, ptrs, pitches, [0, 0]) == 0
    assert A.biquad_batch_planar_device(banks, ptrs, pitches, [-5, 0]) == 0
    errors, states = L.artamdErrorCount(), [_state(b) for b in banks]
    with pytest.raises(RuntimeError):
        A.biquad_batch_planar_device([banks[0], banks[1], banks[0]], ptrs + ptrs[:1], pitches + pitches[:1], frames + frames[:1])
    n = 2
    rc = L.biquadBankApplyBatchPlanarDevice((C.c_void_p * n)(banks[0].p, None), n, (C.c_void_p * n)(*ptrs), (C.c_long * n)(*pitches),
                                            (C.c_int * n)(*frames))
    assert rc == -1
    torch.cuda.synchronize()
    assert L.artamdErrorCount() == errors
    for p, b in zip(ps, before):
        assert torch.equal(_bits(p.buf), _bits(b))
    assert [_state(b) for b in banks] == states
    for b in banks:
        b.close()


# ---- reset and sharded banks -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shards", [0, 2])
def test_reset_puts_a_bank_back_to_a_fresh_one(monkeypatch, shards):
    ch, frames = 8, 1000
    if shards:
        monkeypatch.setenv("ARTAMD_SHARDS", str(shards))
    bank, fresh = _bank(A, ch, "art", multi=bool(shards)), _bank(A, ch, "art")
    assert bank.shards() == shards
    for k, n in enumerate((frames, 37, 300)):                   # arbitrary calls, both layouts
        p = Planes(_signal(ch, n, 40 + k, torch.float32), n + k)
        if k == 1:
            _twin(bank, p.clip())
        else:
            bank.apply_planar_device(p.ptr, p.pitch, n)
    assert _state(bank) != _state(fresh)
    repairs = bank.repairs()
    bank.reset()
    assert _state(bank) == _state(fresh) and bank.repairs() == repairs
    x = _signal(ch, frames, 50, torch.float32)
    p = Planes(x, frames + 3)
    bank.apply_planar_device(p.ptr, p.pitch, frames)
    want = _twin(fresh, x)
    torch.cuda.synchronize()
    assert torch.equal(_bits(p.clip()), _bits(want)) and p.padding_untouched()
    assert _state(bank) == _state(fresh)
    bank.close(); fresh.close()


def test_sharded_planar_call_equals_the_unsharded_twin(monkeypatch):
    ch, frames = 8, 700
    monkeypatch.setenv("ARTAMD_SHARDS", "2")
    bank, twin = _bank(A, ch, "art", multi=True), _bank(A, ch, "art")
    assert bank.shards() == 2 and twin.shards() == 0
    for tick in range(2):
        x = _signal(ch, frames, 60 + tick, torch.float32)
        p = Planes(x, frames + 3)
        bank.apply_planar_device(p.ptr, p.pitch, frames)
        want = _twin(twin, x)
        torch.cuda.synchronize()
        assert torch.equal(_bits(p.clip()), _bits(want)) and p.padding_untouched(), tick
        assert _state(bank) == _state(twin), tick
    bank.close(); twin.close()


# ---- ClipFilter ------------------------------------------------------------------------------------------------------------------

ART_P = [("lowpass", TB.PRE), ("lowpass", TB.PRE)]
LENGTHS = [3000, 0, 1, 257, 2999]


def _fresh_bank(M, ch, sections):
    secs = (M.Biquad * (ch * len(sections)))()
    for s, (kind, freq) in enumerate(sections):
        co = M.BiquadCoefficients()
        (M.lib().biquad_lowpass if kind == "lowpass" else M.lib().biquad_highpass)(C.byref(co), freq)
        for c in range(ch):
            M.lib().biquad_init(C.byref(secs[c * len(sections) + s]), C.byref(co), 1.0)
    return M.BiquadBank(secs, ch, len(sections))


def _clip_wants(x, lengths, sections):
    wants = []
    for i, n in enumerate(lengths):
        b = _fresh_bank(A, x.shape[1], sections)
        wants.append(_twin(b, x[i, :, :n]).contiguous() if n else x[i, :, :0])
        torch.cuda.synchronize()
        b.close()
    return wants


@pytest.fixture(scope="module")
def clips():
    x = _signal(5 * 2, 3000, 8, torch.float32).view(5, 2, 3000)
    return x, _clip_wants(x, LENGTHS, ART_P)


@pytest.mark.parametrize("max_batch", [1024, 2])
def test_clip_filter_equals_fresh_banks_on_each_slice(clips, max_batch):
    x0, wants = clips
    cf = A.ClipFilter(2, ART_P, max_batch=max_batch)
    for rnd in range(2):                                        # (the second call: the pool's banks are reset)
        x = x0.clone()
        y = cf(x, LENGTHS if rnd == 0 else torch.tensor(LENGTHS))
        torch.cuda.synchronize()
        assert y is x
        for i, n in enumerate(LENGTHS):
            assert torch.equal(_bits(x[i, :, :n]), _bits(wants[i])), (rnd, i)
            assert torch.equal(_bits(x[i, :, n:]), _bits(x0[i, :, n:])), (rnd, i)
    assert len(cf.pool) == min(5, max_batch)
    cf.close()


def test_clip_filter_takes_one_clip_a_padded_view_and_refuses_the_rest(clips):
    x0, wants = clips
    cf = A.ClipFilter(2, ART_P)
    x = x0[0].clone()                                           # [C, T]
    assert cf(x) is x
    assert torch.equal(_bits(x), _bits(wants[0]))
    wide = torch.full((2, 3011), SENTINEL, device="cuda")
    wide[:, 6:3006] = x0[0]
    cf(wide[:, 6:3006])                                         # a view into a wider tensor: its row pitch, in place
    assert torch.equal(_bits(wide[:, 6:3006]), _bits(wants[0]))
    assert bool(torch.all(wide[:, :6] == SENTINEL)) and bool(torch.all(wide[:, 3006:] == SENTINEL))
    for bad in (x0[0].double(), x0[0, :1], x0[0].cpu(), x0[0].t().contiguous().t()):
        with pytest.raises(ValueError):
            cf(bad)
    with pytest.raises(ValueError):
        cf(x0.clone(), [3000, 0, 1, 257, 3001])
    cf.close()


def test_clip_filter_in_front_of_clip_resampler_and_clip_decimator():
    """ClipFilter -> ClipResampler -> ClipDecimator on [B, C, T] against the same chain made clip by clip with the interleaved entries
    on transposed copies: equal PCM"""
    HP, SATH = A.DITHER_HIGHPASS, A.SHAPING_ATH_CURVE
    lengths, ch = [4410, 2000, 441], 2
    x = _signal(3 * ch, 4410, 21, torch.float32).view(3, ch, 4410)
    cf, rs, cd = A.ClipFilter(ch, ART_P), A.ClipResampler(ch, 96000, 44100), A.ClipDecimator(ch, 16, 2, 1.0, 44100, HP | SATH)
    y, out_lengths = rs(cf(x.clone(), lengths), lengths)
    pcm, _ = cd(y, out_lengths)
    torch.cuda.synchronize()
    for i, n in enumerate(lengths):
        bank = _fresh_bank(A, ch, ART_P)
        r = A.Resampler(ch, 380, 380, 0.0, A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.INCLUDE_LOWPASS, (96000.0, 44100.0, 0))
        d = A.Decimator(ch, 16, 2, 1.0, 44100, HP | SATH)
        t = x[i, :, :n].t().contiguous()
        bank.apply_device(t, n)
        cap = y.shape[2] + 64
        z = torch.zeros(cap, ch, device="cuda")
        used, made = r.process_device(t, n, z, cap, 44100.0 / 96000.0, and_flush=True)
        assert used == n and made == int(out_lengths[i]), i
        out = torch.zeros(made * ch * 2, dtype=torch.uint8, device="cuda")
        d.process_device(z, made, out)
        torch.cuda.synchronize()
        assert torch.equal(pcm[i, :, :made * 2], out.view(made, ch, 2).permute(1, 0, 2).reshape(ch, made * 2)), i
        bank.close(); r.close(); d.close()
    cf.close(); rs.close(); cd.close()


# ---- the 8-byte build ------------------------------------------------------------------------------------------------------------

def test_wide_build_grid_corners_equal_twins(monkeypatch):
    W = A.wide()
    corners = [g for g in _grid() if g[0] in (CHANNELS[0], CHANNELS[-1], 3) and g[2] in (FRAMES[0], FRAMES[-1], 2 * FLOOR - 1)
               and g[3][0] in ("dense", "offset", "plus1")]
    assert len(corners) == 3 * 3 * 3 * 3
    for k, (ch, kind, frames, layout) in enumerate(corners):
        _single_equals_twin(W, monkeypatch, ch, kind, frames, layout, 7000 + k)


def test_wide_build_mixed_batch_equals_the_loop():
    W = A.wide()
    _batch_equals_loop(W, _batch_specs(W))
    _batch_equals_loop(W, _batch_specs(W), _with_lanes(W, 8))
