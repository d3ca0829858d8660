"""biquadBankFilterClipsPlanarDevice and ClipFilter's autograd: whole clips OUT OF PLACE from the banks' first state, forwards or with
time reversed.  The yardstick is the CPU oracle's recurrence (ora_biquad_buffer on the library's own section records, whose layout
is the oracle's): the forward result is the oracle's, the reversed result is the flipped oracle result of the flipped input, both
bit for bit; the reversed call is the transpose of the forward map entry by entry; and everything else (batch size, one bank for
all, layout, pitch, rounds, dirty banks) changes no bit.

The shapes follow each filter's chunk length L (test_gpu_biquad_clips._chunk mirrors the host's rule): a call is time-parallel from
2 L frames on and above the batch entry's serial bound, else one serial lane per channel."""
import ctypes as C

import numpy as np
import pytest
import torch

import audio_resampler_amd as A
import test_gpu_biquad_batch as TB
import test_gpu_biquad_clips as TC
import test_gpu_biquad_planar as TP
import _adjoint_ref as R
import _oracle as O

pytestmark = pytest.mark.gpu

Planes, _bits, _state, _signal, _dtype, _width, _spec, _bank = TP.Planes, TB._bits, TB._state, TP._signal, TP._dtype, TP._width, TC._spec, TC._bank
FILL = -777.25                                  # what an output buffer holds before the call
CLASS_LAUNCHES = 3                              # spec, check and commit of one (section count, layout) class; no copy launch


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def _np(M):
    return np.float64 if _width(M) == 64 else np.float32


def _oracle_forward(M, secs, S, x):
    """x: numpy [ch, n] -> what fresh sections `secs` (the library's records, channel-major) make of every channel, by the oracle"""
    OB = O.binding(_width(M))
    OL = OB.load_oracle()
    y = np.ascontiguousarray(x, dtype=_np(M)).copy()
    ch, n = y.shape
    for c in range(ch):
        for s in range(S):
            sec = OB.Biquad.from_buffer_copy(bytes(memoryview(secs[c * S + s])))
            if n:
                OL.ora_biquad_buffer(C.byref(sec), C.cast(y[c].ctypes.data, OB.f32p), n, 1)
    return y


def _oracle_reversed(M, secs, S, x):
    return np.ascontiguousarray(_oracle_forward(M, secs, S, np.ascontiguousarray(x[:, ::-1]))[:, ::-1])


def _same_bits(a, b):
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(u), np.ascontiguousarray(b).view(u))


# ---- the call --------------------------------------------------------------------------------------------------------------------
def _raw(M, banks, ins, in_pitches, outs, out_pitches, frames, reverse, round_bytes=0):
    """the entry (or, with a byte bound per round, its private form) on raw addresses; returns what it returns"""
    n = len(banks)
    arr = lambda t, v: None if v is None else (t * n)(*v)
    args = [(C.c_void_p * n)(*[b.p if b is not None else None for b in banks]), n, arr(C.c_void_p, ins), arr(C.c_long, in_pitches),
            arr(C.c_void_p, outs), arr(C.c_long, out_pitches), (C.c_int * n)(*[int(f) for f in frames]), int(reverse)]
    if round_bytes:
        fn = M.lib().artamd_biquad_filter_clips_planar
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_long]
        return fn(*args, round_bytes)
    return M.lib().biquadBankFilterClipsPlanarDevice(*args)


def _lay(s, x, extra=None, offset=None):
    """an item's buffer: planes, or interleaved frames between sentinels (one plane, transposed)"""
    extra, offset = s["extra"] if extra is None else extra, s["offset"] if offset is None else offset
    if s["planar"]:
        return Planes(x, s["frames"] + extra, offset)
    return Planes(x.t().contiguous().view(1, -1), s["frames"] * s["ch"], offset)


def _unlay(s, p):
    """the item's clip as [ch, frames]"""
    return p.clip() if s["planar"] else p.clip().view(s["frames"], s["ch"]).t()


def _out_layout(s, i):
    """every other item's output differs from its input in pitch (by 3: the parity too) and in base (by one sample)"""
    return (s["extra"], s["offset"]) if i % 2 == 0 else (s["extra"] + 3, 1 - s["offset"])


def _run(M, specs, banks, xs, reverse, round_bytes=0, out_layout=_out_layout):
    """one call on fresh buffers; returns (rc, input Planes, output Planes)"""
    ins = [_lay(s, x) for s, x in zip(specs, xs)]
    outs = [_lay(s, torch.full_like(x, FILL), *out_layout(s, i)) for i, (s, x) in enumerate(zip(specs, xs))]
    pitch = lambda s, p: p.pitch if s["planar"] else 0
    torch.cuda.synchronize()
    rc = _raw(M, banks, [p.ptr for p in ins], [pitch(s, p) for s, p in zip(specs, ins)], [p.ptr for p in outs],
              [pitch(s, p) for s, p in zip(specs, outs)], [s["frames"] for s in specs], reverse, round_bytes)
    torch.cuda.synchronize()
    return rc, ins, outs


def _mixed(M):
    return TC._mixed_specs(M) + [_spec(M, 2, 2, "pre", 64, extra=1), _spec(M, 3, 1, "post", 63, extra=2, offset=1),
                                 _spec(M, 8, 3, "hp", 3, planar=False), _spec(M, 2, 2, "hand", 3, extra=1)]


_cache = {}


def _mixed_case(M):
    """the mixed list of a build with its inputs and the oracle's two results, made once and shared (never written)"""
    key = _width(M)
    if key not in _cache:
        specs = _mixed(M) if key == 32 else TC._corner_specs(M) + [_spec(M, 33, 1, "hand", 63, extra=1, offset=1), _spec(M, 2, 4, "post", 0)]
        secs = [TB._sections(M, s["ch"], s["S"], s["kind"]) for s in specs]
        xs = [_signal(s["ch"], s["frames"], 300 + i, _dtype(M)) for i, s in enumerate(specs)]
        hx = [x.cpu().numpy() for x in xs]
        fwd = [_oracle_forward(M, q, s["S"], h) for q, s, h in zip(secs, specs, hx)]
        rev = [_oracle_reversed(M, q, s["S"], h) for q, s, h in zip(secs, specs, hx)]
        _cache[key] = (specs, xs, fwd, rev)
    return _cache[key]


def _classes(specs):
    return {(s["S"], s["planar"] and s["ch"] > 1) for s in specs if s["gathered"]}, {s["S"] for s in specs if s["frames"] > 0 and not s["gathered"]}


def _check_against_oracle(M, specs, xs, ins, outs, want, what):
    for i, s in enumerate(specs):
        assert ins[i].padding_untouched() and outs[i].padding_untouched(), (what, i, s)
        assert torch.equal(_bits(_unlay(s, ins[i])), _bits(xs[i])), (what, i, s)                  # the input keeps its bits
        assert _same_bits(_unlay(s, outs[i]).cpu().numpy(), want[i]), (what, i, s)


# ---- 1. bits against the CPU oracle, both directions -------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_both_directions_give_the_oracles_bits(width):
    """(the 8-byte build: the corner list, test 10's wide case)"""
    M = A.binding(width)
    specs, xs, fwd, rev = _mixed_case(M)
    if width == 32:
        TC._assert_the_mixed_specs_have_every_case(M, specs[:len(TC._mixed_specs(M))])
        assert {64, 63, 3, 1, 0} <= {s["frames"] for s in specs}
    banks = [_bank(M, s) for s in specs]
    classes, serial = _classes(specs)
    for reverse, want in ((0, fwd), (1, rev)):
        rc, ins, outs = _run(M, specs, banks, xs, reverse)
        assert rc == CLASS_LAUNCHES * len(classes) + len(serial), (reverse, rc)
        _check_against_oracle(M, specs, xs, ins, outs, want, (width, reverse))
    for b in banks:
        b.close()


# ---- 2. the forward call is the in-place entry from the start ----------------------------------------------------------------------
def test_forward_equals_the_in_place_entry_from_the_start():
    specs, xs, _, _ = _mixed_case(A)
    banks = [_bank(A, s) for s in specs]
    rc, ins, outs = _run(A, specs, banks, xs, 0)
    assert rc > 0
    copies = [_lay(s, x) for s, x in zip(specs, xs)]
    torch.cuda.synchronize()
    A.biquad_clips_planar_device(banks, [p.ptr for p in copies], [p.pitch if s["planar"] else 0 for s, p in zip(specs, copies)],
                                 [s["frames"] for s in specs], from_start=True)
    torch.cuda.synchronize()
    for i, s in enumerate(specs):
        assert torch.equal(_bits(_unlay(s, outs[i])), _bits(_unlay(s, copies[i]))), (i, s)
    for b in banks:
        b.close()


# ---- 3. verification and repair ----------------------------------------------------------------------------------------------------
def test_verification_and_repair_in_both_directions(monkeypatch):
    """a warm-up far too short: nearly every chunk boundary mismatches and is repaired; the bits stay the oracle's and the repairs
    are counted on the leading bank"""
    monkeypatch.setenv("ARTAMD_BIQUAD_WARMUP", "2")
    over = lambda L, m: m + 1 + 3 * L + 5
    specs = [_spec(A, 2, 1, "pre", over, extra=1), _spec(A, 3, 2, "pre", over, extra=2, offset=1), _spec(A, 8, 2, "hp", over, planar=False),
             _spec(A, 2, 3, "post", over), _spec(A, 33, 4, "hand", over, extra=3), _spec(A, 1, 2, "post", over)]
    assert all(s["L"] == 128 and s["gathered"] for s in specs)
    banks = [_bank(A, s) for s in specs]
    monkeypatch.delenv("ARTAMD_BIQUAD_WARMUP")
    secs = [TB._sections(A, s["ch"], s["S"], s["kind"]) for s in specs]
    xs = [_signal(s["ch"], s["frames"], 500 + i, torch.float32) for i, s in enumerate(specs)]
    others = [b.repairs() for b in banks[1:]]
    for reverse, oracle in ((0, _oracle_forward), (1, _oracle_reversed)):
        before = banks[0].repairs()
        rc, ins, outs = _run(A, specs, banks, xs, reverse)
        assert rc == CLASS_LAUNCHES * len(_classes(specs)[0])
        want = [oracle(A, q, s["S"], x.cpu().numpy()) for q, s, x in zip(secs, specs, xs)]
        _check_against_oracle(A, specs, xs, ins, outs, want, ("repair", reverse))
        assert banks[0].repairs() > before, reverse
    assert [b.repairs() for b in banks[1:]] == others            # (no other bank's counter is written)
    for b in banks:
        b.close()


# ---- 4. the transpose, entry by entry ----------------------------------------------------------------------------------------------
TRANSPOSE_FILTERS = [(2, "pre"), (1, "post"), (1, "hp"), (4, "hand")]      # (chunks of 384, 360, 1416 and 880 frames: operators of 1.2k-3.3k frames)


def _impulse_response_does_not_depend_on_the_position(M, secs, S, frames, positions):
    h = None
    for p in positions:
        e = np.zeros((1, frames), _np(M)); e[0, p] = 1
        y = _oracle_forward(M, secs, S, e)[0]
        if h is None:
            assert p == 0
            h = y
        if not (np.all(y[:p] == 0) and np.array_equal(y[p:], h[:frames - p])):
            return False
    return True


@pytest.mark.parametrize("S,kind", TRANSPOSE_FILTERS)
def test_reversed_call_is_the_transpose_entry_by_entry(S, kind):
    """A unit impulse at frame i through the reversed call is row i of the dense forward operator T, which is built column by column
    from the oracle's forward (column j: what it makes of a unit impulse at j).  Entries are compared as values, without tolerance.
    That rests on the oracle's impulse response not depending on where the impulse sits (from rest, the frames in front of the
    impulse are exact zeros and the rest is the same arithmetic on the same values): checked here first on the oracle, for every
    filter used and every position used; it held for all four, so none was dropped."""
    s0 = _spec(A, 1, S, kind, 0)
    chunk, smax = s0["L"], TB._serial_max(A)
    assert chunk
    secs = TB._sections(A, 1, S, kind)
    bank = A.BiquadBank(secs, 1, S)
    for frames in (96, smax + 2 * chunk + 1):
        gathered = frames > smax and frames >= 2 * chunk
        assert gathered == (frames != 96)
        # both ends, both sides of a cut of the reversed sequence (its frame `chunk` lives at address frames - 1 - chunk) and of the
        # forward one; the serial kernel's tile is 60 frames long
        cut = chunk if gathered else 60
        positions = sorted({0, frames - 1, frames - cut, frames - 1 - cut, cut - 1, cut, frames // 2, 1})
        assert len(positions) <= 8 and positions[0] == 0
        assert _impulse_response_does_not_depend_on_the_position(A, secs, S, frames, positions)
        T = np.zeros((frames, frames), np.float32)
        for j in range(frames):
            e = np.zeros((1, frames), np.float32); e[0, j] = 1
            T[:, j] = _oracle_forward(A, secs, S, e)[0]
        assert np.all(np.triu(T, 1) == 0) and T[0, 0] != 0
        n = len(positions)
        gy = torch.zeros(n, frames + 3, device="cuda")
        for r, i in enumerate(positions):
            gy[r, i] = 1
        gx = torch.full((n, frames + 5), FILL, device="cuda")
        torch.cuda.synchronize()
        rc = A.biquad_filter_clips_planar_device([bank] * n, [gy[r].data_ptr() for r in range(n)], None, [gx[r].data_ptr() for r in range(n)], None,
                                                 [frames] * n, reversed=True)
        torch.cuda.synchronize()
        assert rc == (CLASS_LAUNCHES if gathered else 1)
        got = gx.cpu().numpy()
        assert np.all(got[:, frames:] == FILL)
        for r, i in enumerate(positions):
            assert np.array_equal(got[r, :frames], T[i, :]), (S, kind, frames, i)
    bank.close()


# ---- 5. invariance -----------------------------------------------------------------------------------------------------------------
def _need(s):
    """the chunk-state bytes the host counts for a time-parallel 4-byte item (pcm_host.c / arthip_biquad_spec_scratch)"""
    K = -(-s["frames"] // s["L"])
    states = s["ch"] * K * s["S"] * 32 * 2 + ((s["ch"] * K + 255) & ~255)
    return (states + 4 * s["ch"] + 255) & ~255


@pytest.mark.parametrize("reverse", [0, 1])
def test_batch_bank_repetition_layout_pitch_and_rounds_change_no_bit(reverse):
    n = TB._serial_max(A) + 1 + 3 * 128
    base = _spec(A, 2, 2, "pre", 0)
    frames = [max(n, 2 * base["L"]) + 8 * i for i in range(5)]
    specs = [_spec(A, 2, 2, "pre", f, extra=i % 2, offset=i % 2) for i, f in enumerate(frames)] + [_spec(A, 2, 2, "pre", 200, extra=1)]
    assert [s["gathered"] for s in specs] == [True] * 5 + [False]
    xs = [_signal(2, s["frames"], 700 + i, torch.float32) for i, s in enumerate(specs)]
    one = _bank(A, specs[0])
    rc, _, outs = _run(A, specs, [one] * 6, xs, reverse)
    assert rc == CLASS_LAUNCHES + 1
    want = [_unlay(s, p).clone() for s, p in zip(specs, outs)]

    def same(rc_outs, specs_now, what):
        for i, (s, p) in enumerate(zip(specs_now, rc_outs[2])):
            assert p.padding_untouched(), (what, i)
            assert torch.equal(_bits(_unlay(s, p)), _bits(want[i])), (what, i)
        return rc_outs[0]

    distinct = [_bank(A, s) for s in specs]
    assert same(_run(A, specs, distinct, xs, reverse), specs, "distinct banks") == rc
    for i in range(6):                                                                          # every item alone
        alone = _run(A, specs[i:i + 1], [one], xs[i:i + 1], reverse)
        assert alone[0] == (CLASS_LAUNCHES if specs[i]["gathered"] else 1)
        assert torch.equal(_bits(_unlay(specs[i], alone[2][0])), _bits(want[i])), ("alone", i)
    inter = [dict(s, planar=False) for s in specs]
    assert same(_run(A, inter, [one] * 6, xs, reverse), inter, "interleaved") == rc
    assert same(_run(A, specs, [one] * 6, xs, reverse, out_layout=lambda s, i: (s["extra"] + 7, 1 - s["offset"])), specs, "other pitch and base") == rc
    assert same(_run(A, specs, [one] * 6, xs, reverse, out_layout=lambda s, i: (s["extra"] + 4, s["offset"])), specs, "pitch + 4") == rc
    # three rounds: the byte bound lowered to two items' chunk states
    bound = 2 * max(_need(s) for s in specs[:5])
    assert same(_run(A, specs, [one] * 6, xs, reverse, round_bytes=bound), specs, "three rounds") == 3 * CLASS_LAUNCHES + 1
    for b in [one] + distinct:
        b.close()


# ---- 6. banks are only read --------------------------------------------------------------------------------------------------------
def test_a_bank_in_the_middle_of_a_stream_is_read_as_fresh_and_left_as_it_is():
    specs, xs, fwd, rev = _mixed_case(A)
    banks = [_bank(A, s) for s in specs]
    fresh = [_state(b) for b in banks]
    for b, s in zip(banks, specs):                                       # dirty every bank: 50 frames of a stream of its own
        b.apply_device(_signal(s["ch"], 50, 3, torch.float32).t().contiguous(), 50)
    dirty = [_state(b) for b in banks]
    assert all(d != f for d, f in zip(dirty, fresh))
    repairs = [b.repairs() for b in banks]
    for reverse, want in ((0, fwd), (1, rev)):
        _, ins, outs = _run(A, specs, banks, xs, reverse)
        _check_against_oracle(A, specs, xs, ins, outs, want, ("dirty", reverse))
        assert [_state(b) for b in banks] == dirty                       # x, y and index of every section
    assert [b.repairs() for b in banks[1:]] == repairs[1:]               # (the leading bank's counter is the call's)
    for b in banks:
        b.close()


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_nothing_and_count_nothing(monkeypatch):
    long = lambda L, m: max(2 * L, m + 1) + 5
    specs = [_spec(A, 2, 2, "pre", long, extra=1), _spec(A, 2, 2, "post", 300, extra=1)]
    banks = [_bank(A, s) for s in specs]
    monkeypatch.setenv("ARTAMD_SHARDS", "4")
    sharded = _bank(A, _spec(A, 8, 2, "pre", long, extra=1), multi=True)
    monkeypatch.delenv("ARTAMD_SHARDS")
    assert sharded.shards() == 4
    xs = [_signal(2, s["frames"], 900 + i, torch.float32) for i, s in enumerate(specs)]
    ins = [_lay(s, x) for s, x in zip(specs, xs)]
    outs = [_lay(s, torch.full_like(x, FILL)) for s, x in zip(specs, xs)]
    big_in, big_out = _lay(dict(specs[0], ch=8), _signal(8, specs[0]["frames"], 5, torch.float32)), _lay(dict(specs[0], ch=8), torch.full((8, specs[0]["frames"]), FILL, device="cuda"))
    before = [p.buf.clone() for p in ins + outs + [big_in, big_out]]
    states, errors = [_state(b) for b in banks], A.lib().artamdErrorCount()
    ip, op, pi, po, fr = [p.ptr for p in ins], [p.ptr for p in outs], [p.pitch for p in ins], [p.pitch for p in outs], [s["frames"] for s in specs]
    torch.cuda.synchronize()
    cases = {
        "NULL bank": (banks[:1] + [None], ip, pi, op, po, fr),
        "NULL leading bank": ([None] + banks[1:], ip, pi, op, po, fr),
        "NULL input": (banks, [ip[0], None], pi, op, po, fr),
        "NULL output": (banks, ip, pi, [None, op[1]], po, fr),
        "sharded bank": ([banks[0], sharded], [ip[0], big_in.ptr], [pi[0], big_in.pitch], [op[0], big_out.ptr], [po[0], big_out.pitch], [fr[0], fr[0]]),
        "planar in, interleaved out": (banks, ip, pi, op, [po[0], 0], fr),
        "interleaved in, planar out": (banks, ip, [0, pi[1]], op, po, fr),
        "in place": (banks, ip, pi, [op[0], ip[1]], [po[0], pi[1]], fr),
        "overlapping by one sample": (banks, ip, pi, [ip[0] + 4 * (pi[0] + fr[0] - 1), op[1]], po, fr),
        "output in front, overlapping": (banks, [op[0] + 4 * (po[0] + fr[0] - 1), ip[1]], pi, op, po, fr),
    }
    if torch.cuda.device_count() > 1:                                    # (a bank on another device than the leading one's)
        with torch.cuda.device(1):
            far = _bank(A, specs[1])
        cases["another device"] = ([banks[0], far], ip, pi, op, po, fr)
    for reverse in (0, 1):
        for name, (bk, i_, pi_, o_, po_, f_) in cases.items():
            assert _raw(A, bk, i_, pi_, o_, po_, f_, reverse) == -1, (name, reverse)
        with pytest.raises(RuntimeError):
            A.biquad_filter_clips_planar_device(banks, ip, pi, [op[0], ip[1]], [po[0], pi[1]], fr, reversed=bool(reverse))
    torch.cuda.synchronize()
    assert A.lib().artamdErrorCount() == errors and [_state(b) for b in banks] == states
    for p, b in zip(ins + outs + [big_in, big_out], before):
        assert torch.equal(_bits(p.buf), _bits(b))
    # ... and a skipped item may have anything in its place; the same lists are taken when they are right
    assert _raw(A, banks, [ip[0], None], pi, [op[0], None], po, [fr[0], 0], 0) == CLASS_LAUNCHES
    assert _raw(A, banks, ip, pi, op, po, [0, -1], 1) == 0
    torch.cuda.synchronize()
    for b in banks + [sharded]:
        b.close()


# ---- 8. launch count ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [0, 1])
def test_launch_count_does_not_grow_with_the_batch(reverse):
    rcs = []
    for n in (40, 2):
        specs = [_spec(A, 2, 2, "pre", lambda L, m: 5 * L, extra=i % 3) for i in range(n)]
        assert all(s["gathered"] for s in specs)
        bank = _bank(A, specs[0])
        xs = [_signal(2, s["frames"], 40 + i, torch.float32) for i, s in enumerate(specs)]
        rcs.append(_run(A, specs, [bank] * n, xs, reverse)[0])
        bank.close()
    assert rcs[0] == rcs[1] and 0 < rcs[0] <= 3
    specs, xs, _, _ = _mixed_case(A)
    banks = [_bank(A, s) for s in specs]
    classes, serial = _classes(specs)
    assert len(classes) >= 6 and len(serial) >= 3
    assert _run(A, specs, banks, xs, reverse)[0] == 3 * len(classes) + len(serial)
    for b in banks:
        b.close()


# ---- 9. autograd -------------------------------------------------------------------------------------------------------------------
def _clip_filter_sections(M, ch):
    """ClipFilter(ch, ART_P)'s section records, for the oracle"""
    secs = (M.Biquad * (ch * 2))()
    co = M.BiquadCoefficients()
    M.lib().biquad_lowpass(C.byref(co), TB.PRE)
    for k in range(ch * 2):
        M.lib().biquad_init(C.byref(secs[k]), C.byref(co), 1.0)
    return secs


def test_autograd_gradient_is_the_flipped_oracles():
    """(on the parent commit this fails: ClipFilter filters in place and x.grad comes back as grad_y)"""
    lengths = [700, 513, 40]
    cf = A.ClipFilter(2, TP.ART_P)
    x0 = _signal(3 * 2, 700, 77, torch.float32).view(3, 2, 700)
    x = x0.clone().requires_grad_()
    y = cf(x, lengths)
    assert y is not x and y.requires_grad and y.grad_fn is not None and cf.launches > 0
    inplace = x0.clone()
    assert cf(inplace, lengths) is inplace
    g = _signal(3 * 2, 700, 78, torch.float32).view(3, 2, 700)
    (y * g).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(y.detach()), _bits(inplace))                # what the in-place call leaves, the tails included
    assert torch.equal(_bits(x.detach()), _bits(x0))                     # x keeps its bits
    secs, grad, hg = _clip_filter_sections(A, 2), x.grad.cpu().numpy(), g.cpu().numpy()
    for i, n in enumerate(lengths):
        assert _same_bits(grad[i][:, :n], _oracle_reversed(A, secs, 2, hg[i][:, :n])), i
        assert _same_bits(grad[i][:, n:], hg[i][:, n:]), i
    # a non-contiguous x is taken on this path; an expanded grad_y too
    xt = x0.transpose(1, 2).contiguous().transpose(1, 2).requires_grad_()
    assert xt.stride(2) != 1
    yt = cf(xt, lengths)
    yt.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(yt.detach()), _bits(inplace))
    ones = np.ones((2, 700), np.float32)
    for i, n in enumerate(lengths):
        assert _same_bits(xt.grad[i].cpu().numpy()[:, :n], _oracle_reversed(A, secs, 2, ones[:, :n])), i
        assert bool((xt.grad[i][:, n:] == 1).all()), i
    with pytest.raises(RuntimeError):                                     # (once differentiable)
        x2 = x0.clone().requires_grad_()
        (gx2,) = torch.autograd.grad(cf(x2, lengths).sum(), x2, create_graph=True)
        gx2.sum().backward()
    cf.close()


def test_autograd_through_clip_filter_and_clip_resampler():
    """ClipFilter -> ClipResampler: the gradient is the two oracles composed, link by link — the gradient that reaches the filter's
    output (read with retain_grad) is the resampler's transposed oracle operator applied to grad_y within the bound of
    test_gpu_clip_adjoint.check_sums, and x.grad is the flipped filter oracle of exactly that gradient, bit for bit"""
    import test_gpu_clip_adjoint as TA
    lengths = [600, 411]
    cf, rs = A.ClipFilter(2, TP.ART_P), A.ClipResampler(2, 44100, 16000)
    x = _signal(2 * 2, 600, 91, torch.float32).view(2, 2, 600).mul_(0.25).requires_grad_()
    mid = cf(x, lengths)
    mid.retain_grad()
    y, out_lengths = rs(mid, lengths)
    g = (0.25 * np.random.default_rng(92).standard_normal(tuple(y.shape))).astype(np.float32)
    (y * torch.from_numpy(g).cuda()).sum().backward()
    torch.cuda.synchronize()
    secs, gmid, grad = _clip_filter_sections(A, 2), mid.grad.cpu().numpy(), x.grad.cpu().numpy()
    for i, n in enumerate(lengths):
        dense = R.dense_operator(380, 380, TA.BH | TA.IN | TA.LP, n, fixed=TA.DOWN)
        assert int(out_lengths[i]) == dense.shape[0]
        TA.check_sums(gmid[i][:, :n], dense, g[i][:, :dense.shape[0]], ("chain, resampler link", i))
        assert np.all(gmid[i][:, n:] == 0), i
        assert _same_bits(grad[i][:, :n], _oracle_reversed(A, secs, 2, gmid[i][:, :n])), i
        assert _same_bits(grad[i][:, n:], gmid[i][:, n:]), i
    cf.close(); rs.close()


def test_without_grad_the_call_is_in_place_as_before_and_backward_after_close_raises():
    lengths = [700, 513, 40]
    cf = A.ClipFilter(2, TP.ART_P)
    x0 = _signal(3 * 2, 700, 77, torch.float32).view(3, 2, 700)
    plain = x0.clone()
    assert cf(plain, lengths) is plain and plain.grad_fn is None
    launches = cf.launches
    quiet = x0.clone().requires_grad_()
    with torch.no_grad():
        assert cf(quiet, lengths) is quiet
    torch.cuda.synchronize()
    assert cf.launches == launches > 0 and quiet.grad_fn is None
    assert torch.equal(_bits(quiet.detach()), _bits(plain)) and not torch.equal(plain, x0)
    with pytest.raises(ValueError):                                       # in place there is no copy to fall back on
        cf(x0.transpose(1, 2).contiguous().transpose(1, 2), lengths)
    y = cf(x0.clone().requires_grad_(), lengths)
    cf.close()
    with pytest.raises(RuntimeError):
        y.sum().backward()


# ---- 10. gradcheck on the 8-byte build ---------------------------------------------------------------------------------------------
def test_autograd_gradcheck_on_the_8_byte_build():
    """the settings of test_gpu_clip_adjoint's gradcheck: the stage is linear with gain near one, the regime they were chosen for"""
    B = A.binding(64)
    cf = B.ClipFilter(2, TP.ART_P)
    x = torch.from_numpy(0.25 * np.random.default_rng(81).standard_normal((2, 2, 40))).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda t: cf(t, [40, 23]), (x,), eps=1e-6, atol=1e-7, rtol=1e-6)
    cf.close()


# ---- 11. the shared runs' address arithmetic at its edges --------------------------------------------------------------------------
# One copy of the plane run, the interleaved run, the pipeline and its chunk mover serves this entry in both directions and the
# in-place entry: every way the runs cut a plane, at every alignment of either side.
EDGE_FRAMES = [513, 514, 519, 520, 521, 528]    # behind four chunks of 128: a last chunk of 1, 2, 7, 8, 9 and 16 frames (head only, no
                                                # whole batch, one batch exactly, a batch and a tail), and every chunk in front of it
SERIAL_FRAMES = [1, 3, 4, 5, 59, 60, 61, 121]   # the pipeline's chunk is 60 frames: a lane that sits out, both sides of the cut, a third chunk


def _q(M):
    return 16 // (_width(M) // 8)                # samples to 16 bytes


def _quick_sections(M, ch):
    """one order-1 section per channel whose pole (0.15, 0.14, ...) is forgotten within 15 frames (8-byte: 26): the shortest chunk"""
    secs = (M.Biquad * ch)()
    for c in range(ch):
        co = M.BiquadCoefficients(a0=0.3, a1=0.2 + 0.01 * c, b1=-0.15 + 0.01 * c)
        M.lib().biquad_init(C.byref(secs[c]), C.byref(co), 1.0)
    return secs


def _edge_filter(M, forced, monkeypatch):
    """(S, sections of a 2-channel bank, a function that makes such a bank, chunk length).  forced: ART's post-filter with the warm-up
    forced to 2 frames — chunks of 128 in both builds, and nearly every chunk repaired by the commit pass; else a filter with its
    own warm-up: no repairs, what the speculative pass stored is what is compared"""
    if forced:
        monkeypatch.setenv("ARTAMD_BIQUAD_WARMUP", "2")
        S, secs = 2, TB._sections(M, 2, 2, "post")
    else:
        S, secs = 1, _quick_sections(M, 2)
    L = TC._chunk(M, secs, S)
    banks = []

    def make(count):
        if forced:
            monkeypatch.setenv("ARTAMD_BIQUAD_WARMUP", "2")
        banks.extend(M.BiquadBank(secs, 2, S) for _ in range(count))
        monkeypatch.delenv("ARTAMD_BIQUAD_WARMUP", raising=False)
        return banks[-count:]
    monkeypatch.delenv("ARTAMD_BIQUAD_WARMUP", raising=False)
    return S, secs, make, L


def _edge_specs(M, S, L, out_offsets=True):
    """2-channel planar items, one for each length and each start of the input plane within 16 bytes and (out_offsets) of the
    output plane; the pitch is a multiple of 16 bytes, so that both planes of an item start alike"""
    q, smax = _q(M), TB._serial_max(M)
    specs = [dict(ch=2, S=S, kind=None, frames=n, planar=True, extra=(-n) % q, offset=oi, out_offset=oo, L=L, gathered=True)
             for n in EDGE_FRAMES for oi in range(q) for oo in (range(q) if out_offsets else [oi])]
    assert L and all(s["frames"] >= 2 * L and s["frames"] > smax for s in specs)
    return specs


def _serial_specs(M, out_offsets=True):
    """serial lanes of every length: 3-channel planar items at each start of either plane within 16 bytes, and an interleaved item
    in their middle wide enough for the class to pass 512 lanes — from there on the lane rule puts two lanes into a workgroup, and
    with an odd lane count per length the pairs straddle the items, the layouts and the lengths"""
    q, specs = _q(M), []
    for n in SERIAL_FRAMES:
        planar = [dict(ch=3, S=2, kind="hand", frames=n, planar=True, extra=(-n) % q, offset=oi, out_offset=oo, L=0, gathered=False)
                  for oi in range(q) for oo in (range(q) if out_offsets else [oi])]
        wide = 65 - 3 * len(planar) if 3 * len(planar) < 32 else 33
        wide += (3 * len(planar) + wide + 1) % 2
        inter = dict(ch=wide, S=2, kind="hand", frames=n, planar=False, extra=0, offset=1, out_offset=0, L=0, gathered=False)
        specs += planar[:len(planar) // 2] + [inter] + planar[len(planar) // 2:]
    lanes = sum(s["ch"] for s in specs)
    assert lanes // len(SERIAL_FRAMES) % 2 == 1 and lanes > 512 and M.lib().arthip_biquad_batch_lanes(lanes) == 2
    return specs


_own_out = lambda s, i: (s["extra"], s["out_offset"])


@pytest.mark.parametrize("width,forced", [(32, False), (32, True), (64, False), (64, True)])
def test_plane_runs_at_every_alignment_and_tail_in_both_directions(monkeypatch, width, forced):
    M = A.binding(width)
    S, secs, make, L = _edge_filter(M, forced, monkeypatch)
    assert L == 128 or (width == 64 and not forced)
    specs = _edge_specs(M, S, L)
    assert len(specs) == len(EDGE_FRAMES) * _q(M) ** 2
    (bank,) = make(1)
    xs = [_signal(2, s["frames"], 1100 + i, _dtype(M)) for i, s in enumerate(specs)]
    hx = [x.cpu().numpy() for x in xs]
    for reverse, oracle in ((0, _oracle_forward), (1, _oracle_reversed)):
        before = bank.repairs()
        rc, ins, outs = _run(M, specs, [bank] * len(specs), xs, reverse, out_layout=_own_out)
        assert rc == CLASS_LAUNCHES, (reverse, rc)
        _check_against_oracle(M, specs, xs, ins, outs, [oracle(M, secs, S, h) for h in hx], (width, forced, reverse))
        assert (bank.repairs() > before) == forced, (width, forced, reverse)
    bank.close()


@pytest.mark.parametrize("width", [32, 64])
def test_serial_lanes_of_every_length_and_alignment_in_both_directions(width):
    M = A.binding(width)
    specs = _serial_specs(M)
    by_ch = {ch: _bank(M, dict(ch=ch, S=2, kind="hand")) for ch in {s["ch"] for s in specs}}
    secs = {ch: TB._sections(M, ch, 2, "hand") for ch in by_ch}
    xs = [_signal(s["ch"], s["frames"], 1300 + i, _dtype(M)) for i, s in enumerate(specs)]
    hx = [x.cpu().numpy() for x in xs]
    for reverse, oracle in ((0, _oracle_forward), (1, _oracle_reversed)):
        rc, ins, outs = _run(M, specs, [by_ch[s["ch"]] for s in specs], xs, reverse, out_layout=_own_out)
        assert rc == 1, (reverse, rc)
        _check_against_oracle(M, specs, xs, ins, outs, [oracle(M, secs[s["ch"]], 2, h) for s, h in zip(specs, hx)], (width, reverse))
    for b in by_ch.values():
        b.close()


def _oracle_in_place(M, secs, S, x):
    """_oracle_forward, and the sections as the oracle leaves them"""
    OB = O.binding(_width(M))
    OL = OB.load_oracle()
    y = np.ascontiguousarray(x, dtype=_np(M)).copy()
    ch, n = y.shape
    left = [OB.Biquad.from_buffer_copy(bytes(memoryview(secs[k]))) for k in range(ch * S)]
    for c in range(ch):
        for s in range(S):
            OL.ora_biquad_buffer(C.byref(left[c * S + s]), C.cast(y[c].ctypes.data, OB.f32p), n, 1)
    return y, left


def _clips_entry_equals_the_oracle(M, specs, banks, sections, what):
    """biquadBankApplyClipsPlanarDevice from the start on dirty banks: the bits in place, the padding and the final bank state"""
    xs = [_signal(s["ch"], s["frames"], 1500 + i, _dtype(M)) for i, s in enumerate(specs)]
    bufs = [_lay(s, x) for s, x in zip(specs, xs)]
    for b, s in zip(banks, specs):                                       # (from the start: what a bank went through before does not count)
        b.apply_device(_signal(s["ch"], 9, 3, _dtype(M)).t().contiguous(), 9)
    torch.cuda.synchronize()
    rc = M.biquad_clips_planar_device(banks, [p.ptr for p in bufs], [p.pitch if s["planar"] else 0 for s, p in zip(specs, bufs)],
                                      [s["frames"] for s in specs], from_start=True)
    torch.cuda.synchronize()
    hist = lambda q, arr: [arr[(q.index - i) & 3] for i in range(4)]
    for i, (s, p, x, b) in enumerate(zip(specs, bufs, xs, banks)):
        want, left = _oracle_in_place(M, sections(s), s["S"], x.cpu().numpy())
        assert p.padding_untouched(), (what, i, s)
        assert _same_bits(_unlay(s, p).cpu().numpy(), want), (what, i, s)
        st = b.read()
        for k in range(s["ch"] * s["S"]):
            assert hist(st[k], st[k].x) == hist(left[k], left[k].x) and hist(st[k], st[k].y) == hist(left[k], left[k].y), (what, i, k, s)
    return rc


@pytest.mark.parametrize("width,forced", [(32, False), (32, True), (64, False), (64, True)])
def test_the_in_place_entry_on_the_same_planes(monkeypatch, width, forced):
    M = A.binding(width)
    S, secs, make, L = _edge_filter(M, forced, monkeypatch)
    specs = _edge_specs(M, S, L, out_offsets=False)
    banks = make(len(specs))
    assert _clips_entry_equals_the_oracle(M, specs, banks, lambda s: secs, (width, forced)) == TC.ROUND_LAUNCHES
    for b in banks:
        b.close()


@pytest.mark.parametrize("width", [32, 64])
def test_the_in_place_entry_on_the_same_serial_lanes(width):
    M = A.binding(width)
    specs = _serial_specs(M, out_offsets=False)
    banks = [_bank(M, s) for s in specs]
    rc = _clips_entry_equals_the_oracle(M, specs, banks, lambda s: TB._sections(M, s["ch"], 2, "hand"), width)
    assert rc == 2                                                       # the copy launch that puts the sections back, and one class
    for b in banks:
        b.close()
