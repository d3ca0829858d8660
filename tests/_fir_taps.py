"""TEST INFRASTRUCTURE ONLY: the forward FIR kernels pinned tap by tap on impulse trains.

A session whose every channel carries one impulse per `spacing >= T + 4` frames puts AT MOST ONE non-zero product into every
output window, so summation order and accumulator width do not enter: an output IS one weight of the operator times a signed
power of two.  The strict oracle (which the suite pins to the reference bit for bit) gives the wanted value; `attribute` says
which (phase, filter, fraction, tap, channel) each output is, from a replay of the oracle's own position arithmetic;
`bound` says how far a kernel form may legitimately sit from it; `report` localises a miss by tile coordinates.

THE BOUND, per output (derived here, not fitted to what the kernels give).  a = the impulse's amplitude (a signed power of two),
h0 = bank[fi][k], h1 = bank[fi + 1][k], frac the output's own fraction.  The reference computes, in fp64 and un-fused,
    want = float (float (h0 a) (1 - frac) + float (h1 a) frac)                                (art_oracle.c evaluate_at)
and float (h a) = h a exactly (a power of two, no underflow at the amplitudes used).
  * float forms: every kernel blends g = h0 (1 - frac') + h1 frac' in fp64 and rounds ONCE to the sample type, either per output
    (general kernel, 8-byte matrix kernel) or per row (the effective row), and g a is exact again.  With frac' == frac
    the two sides round the same fp64 value up to the order of three fp64 roundings (2^-52 relative): the same float or, across
    a rounding boundary, its neighbour -> ONE SPACING of the sample type at the reference value.
  * frac' != frac: the matrix kernels of a regular launch take the fraction of the slot's canonical lattice position; the host
    lets a launch be regular only if every output is within MF_PHASE_TOL = 2e-6 filter steps of it (fir_matrix_common.hip.h:63,
    enforced in mfma_launch_is_regular, fir_matrix.hip:953-957, and per output in fir_mfma_kernel, fir_matrix.hip:277; DESIGN 4.1
    says the same 2e-6).  The weight is piecewise linear in the position, so it moves by at most |a| |h1 - h0| eps_pos, with the
    steeper of the two segments where the output is within eps_pos of a filter boundary (the canonical position may lie across it).
    The general kernel and the 8-byte matrix kernel replay the reference's position arithmetic (locate, fir_common.hip.h:69-92)
    in their own coordinates: the base and the sum round once each, 2 x 2^-53 x |position| frames with ring positions < 16 T
    -> eps_pos = 2^-52 x 16 T x F filter steps (4e-9 at 988/988).
    Nearest-filter and pass-through outputs have no fraction: no slope term (a regular launch guarantees the same filter index).
  * fixed-point forms: the effective row is rounded once to 30 fraction bits: + |a| 2^-31.  The impulse is its channel's
    peak in every exponent block (each channel carries ONE amplitude), so the sample is exact at the channel's exponent.
  * an output whose window holds NO impulse (the silent channel, the gaps of every other) must be zero exactly, -0.0 allowed.  An
    output whose window holds one at a weight the reference evaluates to 0 (the cleared end taps at frac == 0) is held to the
    same bound as any other attributed output: spacing (0) = the smallest denormal, plus the slope term where there is one.
"""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _oracle
from _oracle import BH, INTERP, LOWPASS, PRECISE

MF_PHASE_TOL = 2e-6          # fir_matrix_common.hip.h:63 (filter steps)

# (channels, taps, filters, src, dst, fixed-ratio form, flags, calls, spacing)
# Calls: two of about 24,000 and 21,000 frames (test_gpu_fixed_point.py asserts the fixed-point kernel from 20,000 frames on) and a
# flush.  The stereo and mono trains have ONE live channel and the downsampling stream a 320-frame input period: they need more
# impulses than 45,000 frames hold to show every (phase, tap), so their calls are longer.  The spacing is one >= T + 4 with which the
# train's impulse frames take every residue of the input period (search_spacing finds the smallest; the headline's 1,001 is the issue's
# own); test_fir_taps_ref.py checks the coverage that results.
CASES = {
    "headline":     (8, 988, 988, 44100, 48000, False, BH | INTERP, (24000, 21000), 1001),
    "downsampling": (8, 988, 988, 96000, 44100, True, BH | INTERP | LOWPASS, (30000, 24000), 1137),
    "nearest":      (4, 380, 32, 44100, 48000, False, BH, (24000, 21000), 386),
    "short_period": (8, 512, 512, 48000, 32000, False, BH | INTERP, (24000, 21000), 517),
    "stereo":       (2, 380, 380, 44100, 48000, False, BH | INTERP, (36000, 24000), 386),
    "mono":         (1, 380, 380, 44100, 48000, False, BH | INTERP, (36000, 24000), 386),
    "ch16":         (16, 156, 156, 44100, 48000, False, BH | INTERP, (24000, 21000), 160),
    "ch32":         (32, 988, 988, 44100, 48000, False, BH | INTERP, (24000, 21000), 992),
    "ch6":          (6, 156, 156, 44100, 48000, False, BH | INTERP, (24000, 21000), 160),
    "ch33":         (33, 156, 156, 44100, 48000, False, BH | INTERP, (24000, 21000), 160),
}

AMPLITUDES = (1.0, -1.0, 2.0 ** -10, 2.0 ** 7, 2.0 ** -20, -2.0 ** 3, 2.0 ** -4)


def period(case):
    """(P, Q): P outputs per Q input frames"""
    r = Fraction(case[4], case[3])
    return r.numerator, r.denominator


def amplitudes(channels):
    """signed powers of two over 27 binades; the LAST channel of a stream of two or more is all zeros"""
    a = [AMPLITUDES[c % len(AMPLITUDES)] for c in range(channels)]
    if channels > 1:
        a[-1] = 0.0
    return a


def impulse_frames(frames, channels, spacing, first, c):
    return np.arange(first + (c * spacing) // channels, frames, spacing)


def train(frames, channels, spacing, amps, first, dtype=np.float32):
    """interleaved [frames, channels]: channel c has amps[c] at first + (c * spacing) // channels + j * spacing, zeros elsewhere"""
    x = np.zeros((frames, channels), dtype)
    for c in range(channels):
        if amps[c] != 0.0:
            x[impulse_frames(frames, channels, spacing, first, c), c] = amps[c]
    return x


def search_spacing(case, frames):
    """the smallest spacing >= T + 4 whose impulse frames (live channels, first = T) take every residue of the input period"""
    ch, T = case[0], case[1]
    Q = period(case)[1]
    amps = amplitudes(ch)
    for s in range(T + 4, T + 4 + 2 * Q + 64):
        seen = set()
        for c in range(ch):
            if amps[c] != 0.0:
                seen.update((impulse_frames(frames - T, ch, s, T, c) % Q).tolist())     # (the last T frames: windows cut by the flush)
        if len(seen) == Q:
            return s
    raise AssertionError("no spacing covers the period: lengthen the calls")


def session(name, offset=0, width=32):
    """(case, x, calls, meta): the train of a case.  `offset` moves every impulse (the grouped launch's contexts)."""
    case = CASES[name]
    ch, T, calls = case[0], case[1], tuple(case[7])
    frames = sum(calls)
    spacing = case[8]
    amps = amplitudes(ch)
    meta = dict(frames=frames, spacing=spacing, first=T + offset, amps=amps)
    return case, train(frames, ch, spacing, amps, T + offset, np.float64 if width == 64 else np.float32), calls, meta


def cuts(total, seed, period_in):
    """the same train in calls of 1 .. 400 frames, the first one shorter than a period of the input"""
    rng = np.random.default_rng(seed)
    c = [period_in // 2]
    while sum(c) < total:
        c.append(int(min(rng.integers(1, 401), total - sum(c))))
    return tuple(c)


# every session the GPU tests play: id -> (case name, impulse offset, sample width, seed of the cuts or None)
SESSIONS = {name: (name, 0, 32, None) for name in CASES}
SESSIONS.update({"headline_cuts": ("headline", 0, 32, 7), "downsampling_cuts": ("downsampling", 0, 32, 11),
                 "stereo_plus131": ("stereo", 131, 32, None), "stereo_plus262": ("stereo", 262, 32, None),
                 "headline_wide": ("headline", 0, 64, None), "nearest_wide": ("nearest", 0, 64, None)})
_prepared = {}


def session_of(sid):
    """(case, x, calls, meta) of a session id: the train and how it is cut into calls"""
    name, offset, width, seed = SESSIONS[sid]
    case, x, calls, meta = session(name, offset, width)
    if seed is not None:
        calls = cuts(sum(calls), seed, period(case)[1])
    return case, x, calls, meta


def prepared(sid):
    """(case, x, calls, meta, ref, att) of a session, computed once per process and shared (read-only) by the tests that need it"""
    if sid not in _prepared:
        width = SESSIONS[sid][2]
        case, x, calls, meta = session_of(sid)
        ref = reference(case, x, calls, width=width)
        att = attribute(case, ref, meta, width)
        for a in [x, ref["bank"]] + ref["outs"] + [v for v in att.values() if isinstance(v, np.ndarray)]:
            a.setflags(write=False)
        _prepared[sid] = (case, x, calls, meta, ref, att)
    return _prepared[sid]


def bank_view(oracle):
    """the oracle's own bank, writable in place (test_fir_taps_ref.py doctors it)"""
    c = oracle.c
    return np.ctypeslib.as_array(c.bank, shape=(c.filters + 1, c.taps))


def make_oracle(case, precise=False, width=32):
    ch, T, F, src, dst, fixed, flags = case[:7]
    O = _oracle.binding(width)
    fl = flags | (PRECISE if precise else 0)
    r = O.OracleResampler(ch, T, F, flags=fl, fixed=(float(src), float(dst), 0)) if fixed else O.OracleResampler(ch, T, F, 0.0, fl)
    r.advance(T / 2)
    return r


def _replay_call(c, n_in, cap, ratio):
    """art_oracle.c run_channel on the context's (read_pos, write_pos, flags) without the samples: for every output of the call the
    position it is evaluated at (ring frames, as the oracle rounds it) and the stream frame that ring frame 0 stands for; and the
    state the call must leave.  n_in < 0: the flush."""
    T, L = c["T"], 16 * c["T"]
    half, pos, wp, fed, step, made = T // 2, c["pos"], c["wp"], c["fed"], 0.0, 0
    p_out, origin = [], []
    if c["flushed"]:
        n_in = 0
    if n_in < 0:
        if L - wp < half:
            pos -= L - T; wp -= L - T
        c["flushed"] = True
        wp += half; fed += half
    used = 0
    while cap > 0:
        if pos + step >= wp - half:
            if n_in <= 0:
                break
            if wp == L:
                pos -= L - T; wp -= L - T
            wp += 1; fed += 1; used += 1; n_in -= 1
        else:
            p_out.append(pos + step); origin.append(fed - wp)
            made += 1
            step = made / ratio
            cap -= 1
    pos += step
    if c["snap"]:
        F = c["F"]
        pos = np.floor(pos) + np.floor((pos - np.floor(pos)) * F + 0.5) / F
    c["pos"], c["wp"], c["fed"] = float(pos), wp, fed
    return used, np.array(p_out, np.float64), np.array(origin, np.int64)


def reference(case, x, calls, precise=False, width=32, flush=True, oracle=None):
    """the session through the strict oracle: dict (outs = outputs per call, trace, replay, bank, flags): replay[call] = (positions,
    origins) of its outputs, from the oracle's read and write positions in front of each call.  The replay is checked against the
    oracle: counts and the position after every call."""
    r = oracle or make_oracle(case, precise, width)
    T, F = case[1], r.c.filters
    ratio = r.c.fixed_ratio if case[5] else case[4] / case[3]
    state = dict(T=T, F=F, pos=float(r.c.read_pos), wp=int(r.c.write_pos), fed=0, flushed=False, snap=bool(r.c.flags & _oracle.SNAP))
    outs, trace, replay, at = [], [], [], 0
    for n in list(calls) + ([-1] if flush else []):
        assert state["pos"] == r.c.read_pos and state["wp"] == r.c.write_pos, "replay and oracle disagree in front of a call"
        assert r.position() == r.c.read_pos + T / 2.0 - r.c.write_pos
        cap = (int(n * case[4] / case[3]) + 2 * T + 64) if n >= 0 else 4 * T + 64
        if n >= 0:
            u, g, y = r.process(x[at:at + n], cap, 0.0 if case[5] else case[4] / case[3], threads=8)
        else:
            u, g, y = r.process(None, cap, case[4] / case[3], flush=True, threads=8)
        used, p, origin = _replay_call(state, n, cap, ratio)
        assert (used, len(p)) == (u, g), ("replay and oracle disagree", (used, len(p)), (u, g))
        outs.append(np.array(y[:g], copy=True)); trace.append((int(u), int(g), float(r.position()))); replay.append((p, origin)); at += u
    assert state["pos"] == r.c.read_pos and state["wp"] == r.c.write_pos
    return dict(outs=outs, trace=trace, replay=replay, bank=r.bank(), flags=int(r.c.flags))


def attribute(case, ref, meta, width=32):
    """For every output of the session (rows in session order) and every channel: which product it is.  A dict of arrays [outputs] or
    [outputs, channels]: call, n (index in its call), N (index in the session), phase = N mod P, fi, frac, ip (stream frame of the window's
    centre), k [o, c] (tap; -1: no impulse in the window), amp [c], passthrough [o], value [o, c] (amp x weight as the reference
    evaluates it, in the sample type) and the two bank entries h0, h1 [o, c].
    Self-check (test_fir_taps_ref.py, and every GPU test through compare ()): `value` equals the oracle's output bit for bit at EVERY
    output, interpolating cases included — the zeros too."""
    ch, T = case[0], case[1]
    replay, bank = ref["replay"], ref["bank"]
    F = bank.shape[0] - 1
    interp, lowpass = bool(ref["flags"] & INTERP), bool(ref["flags"] & LOWPASS)      # (the context's own: a fixed-ratio init drops interpolation where the phases fit)
    P = period(case)[0]
    smp = np.float64 if width == 64 else np.float32
    p = np.concatenate([r[0] for r in replay]); origin = np.concatenate([r[1] for r in replay])
    call = np.concatenate([np.full(len(r[0]), i) for i, r in enumerate(replay)])
    n = np.concatenate([np.arange(len(r[0])) for r in replay])
    N = np.arange(len(p))
    whole = np.floor(p)
    fr = (p - whole) * F
    if interp:
        fi = np.floor(fr).astype(np.int64); frac = fr - fi
    else:
        fi = np.floor(fr + 0.5).astype(np.int64); frac = np.zeros_like(fr)
    ip = whole.astype(np.int64) + origin
    passthrough = (fi % F == 0) if (not interp and not lowpass) else np.zeros(len(p), bool)
    first_tap = ip - T // 2 + 1
    k = np.full((len(p), ch), -1, np.int64)
    for c in range(ch):
        if meta["amps"][c] == 0.0:
            continue
        f0 = meta["first"] + (c * meta["spacing"]) // ch
        m = np.maximum(-((f0 - first_tap) // meta["spacing"]), 0)               # ceil ((first_tap - f0) / spacing), not below 0
        f = f0 + m * meta["spacing"]
        kc = f - first_tap
        hit = (kc < T) & (f < meta["frames"]) & (kc >= 0)
        hit &= ~passthrough | (kc == T // 2 - 1 + fi // F)
        k[:, c] = np.where(hit, kc, -1)
    # the same tap counted from the window of the output's exact rational position (the stream starts on a whole frame): where the
    # reference's rounded position falls just short of a whole frame its window, and k with it, is one frame off the lattice's
    Q = period(case)[1]
    k_lat = np.where(k >= 0, k + (ip - (N * Q) // P)[:, None], -1)
    amp = np.array(meta["amps"], np.float64)
    kk = np.maximum(k, 0)
    h0 = bank[fi[:, None], kk].astype(np.float64)
    h1 = bank[np.minimum(fi + 1, F)[:, None], kk].astype(np.float64)
    live = k >= 0
    if interp:
        # art_oracle.c:274, un-fused: dot () returns the sample-type product as a double
        left = (h0.astype(smp) * amp.astype(smp)[None, :]).astype(np.float64) * (1.0 - frac)[:, None]
        right = (h1.astype(smp) * amp.astype(smp)[None, :]).astype(np.float64) * frac[:, None]
        value = (left + right).astype(smp)
    else:
        value = np.where(passthrough[:, None], amp[None, :], h0 * amp[None, :]).astype(smp)
    value = np.where(live, value, smp(0.0))
    return dict(call=call, n=n, N=N, phase=N % P, fi=fi, frac=frac, ip=ip, k=k, k_lat=k_lat, amp=amp, passthrough=passthrough, value=value,
                h0=np.where(live, h0, 0.0), h1=np.where(live, h1, 0.0), interp=interp, F=F, T=T, P=P, width=width)


def _spacing(v, width):
    mant, low = (52, -1022) if width == 64 else (23, -126)
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** low))) - mant)


def eps_pos(form, T, F):
    """position disagreement with the reference, in filter steps (module docstring)"""
    return MF_PHASE_TOL if form in ("f32", "i8") else 2.0 ** -52 * 16 * T * F


def bound(att, bank, form):
    """[outputs, channels] — module docstring.  form: 'general' (also the 8-byte matrix kernel: it blends with the output's own
    fraction), 'f32' (matrix kernels on effective rows), 'i8' (fixed point)."""
    want = att["value"].astype(np.float64)
    b = _spacing(want, att["width"])
    if att["interp"]:
        T, F = att["T"], att["F"]
        eps = eps_pos(form, T, F)
        fi, frac, k = att["fi"], att["frac"], np.maximum(att["k"], 0)
        slope = np.abs(att["h1"] - att["h0"])
        H = bank.astype(np.float64)
        # within eps of a filter boundary the other side's position may lie in the neighbouring segment: below filter 0 that is the last
        # segment of the window one frame earlier (tap k + 1 of rows F - 1, F; row F = row 0 delayed by one tap), above the last likewise
        lo = np.where(fi > 0, fi - 1, F - 1); klo = np.where(fi > 0, k.T, k.T + 1).T
        below = np.where(klo < T, np.abs(H[(lo + 1)[:, None], np.minimum(klo, T - 1)] - H[lo[:, None], np.minimum(klo, T - 1)]), 0.0)
        hi = np.where(fi + 1 < F, fi + 1, 0); khi = np.where(fi + 1 < F, k.T, k.T - 1).T
        above = np.where(khi >= 0, np.abs(H[(hi + 1)[:, None], np.maximum(khi, 0)] - H[hi[:, None], np.maximum(khi, 0)]), 0.0)
        slope = np.maximum(slope, np.where((frac <= eps)[:, None], below, 0.0))
        slope = np.maximum(slope, np.where((frac >= 1.0 - eps)[:, None], above, 0.0))
        b = b + np.abs(att["amp"])[None, :] * slope * eps
    if form == "i8":
        b = b + np.abs(att["amp"])[None, :] * 2.0 ** -31
    return np.where(att["k"] >= 0, b, 0.0)


def compare(att, bank, form, outs, want_outs):
    """(misses [outputs, channels] bool, ratio error / bound (1e300 where a zero is not kept)).  Also the instrument's self-check:
    the attributed value IS the oracle's output, bit for bit, everywhere."""
    got, want = np.concatenate(outs), np.concatenate(want_outs)
    assert got.shape == want.shape == att["value"].shape, (got.shape, want.shape, att["value"].shape)
    assert got.dtype == want.dtype == att["value"].dtype
    same = att["value"] == want
    assert same.all(), ("attribution is not the oracle", int((~same).sum()), np.argwhere(~same)[:5].tolist())
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    b = bound(att, bank, form)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err == 0, 0.0, 1e300))
    ratio = np.where(np.isfinite(got), ratio, 1e300)
    return ratio > 1.0, ratio


def coverage(att, outs=None):
    """the (phase, k) pairs seen with a non-zero value: the reference's (outs None: the attributed values) or a form's own outputs.
    k on the lattice (attribute: k_lat), so that the pair names one weight of the operator whichever way a position rounded"""
    v = att["value"] if outs is None else np.concatenate(outs)
    o, c = np.nonzero((v != 0) & (att["k"] >= 0))
    return set(zip(att["phase"][o].tolist(), att["k_lat"][o, c].tolist()))


def required_coverage(case, ref):
    """every (phase, k) whose weight is non-zero in the bank at the phase's exact rational position (stream started on a whole frame)"""
    P, Q = period(case)
    bank = ref["bank"]
    T, F = case[1], bank.shape[0] - 1
    interp, lowpass = bool(ref["flags"] & INTERP), bool(ref["flags"] & LOWPASS)
    need = set()
    H = bank.astype(np.float64)
    for ph in range(P):
        u = Fraction((ph * Q) % P, P) * F
        if interp:
            fi = u.numerator // u.denominator; frac = float(u - fi)
            w = H[fi] * (1.0 - frac) + H[fi + 1] * frac
        else:
            fi = (2 * u.numerator + u.denominator) // (2 * u.denominator)
            if not lowpass and fi % F == 0:
                w = np.zeros(T); w[T // 2 - 1 + fi // F] = 1.0
            else:
                w = H[fi]
        need.update((ph, int(k)) for k in np.nonzero(w)[0])
    return need


def small_weights(att):
    """count of compared outputs whose weight (both bank entries) is below 2^-24: what the parity bar cannot see at any amplitude <= 1"""
    live = (att["k"] >= 0) & (att["value"] != 0)
    return int(np.count_nonzero(live & (np.maximum(np.abs(att["h0"]), np.abs(att["h1"])) < 2.0 ** -24) & ~att["passthrough"][:, None]))


def report(att, outs, want_outs, misses, ratio, limit=20):
    """the text that makes a miss debuggable: the worst outputs with their tile coordinates, and where the misses pile up"""
    got, want = np.concatenate(outs), np.concatenate(want_outs)
    o, c = np.nonzero(misses)
    lines = [f"{len(o)} outputs outside the bound (of {int(np.count_nonzero(att['k'] >= 0))} attributed, {misses.size} in all)",
             "call n phase n%32 n%64 k k//32 channel got want error/bound"]
    order = np.argsort(-ratio[o, c], kind="stable")[:limit]
    for j in order:
        i, ch = o[j], c[j]
        lines.append(f"{att['call'][i]} {att['n'][i]} {att['phase'][i]} {att['n'][i] % 32} {att['n'][i] % 64} {att['k'][i, ch]} "
                     f"{att['k'][i, ch] // 32 if att['k'][i, ch] >= 0 else -1} {ch} {got[i, ch]!r} {want[i, ch]!r} {ratio[i, ch]:.3g}")
    by_tile, by_channel = {}, {}
    for i, ch in zip(o.tolist(), c.tolist()):
        key = (int(att["n"][i] % 64), int(att["k"][i, ch] // 32) if att["k"][i, ch] >= 0 else -1)
        by_tile[key] = by_tile.get(key, 0) + 1
        by_channel[ch] = by_channel.get(ch, 0) + 1
    lines.append("misses by (n mod 64, k // 32): " + ", ".join(f"{k}: {v}" for k, v in sorted(by_tile.items(), key=lambda kv: -kv[1])[:40]))
    lines.append("misses by channel: " + ", ".join(f"{k}: {v}" for k, v in sorted(by_channel.items())))
    return "\n".join(lines)


def missed_slots(att, misses):
    o, c = np.nonzero(misses)
    return set(zip(att["phase"][o].tolist(), att["k_lat"][o, c].tolist()))


def check(name, form, outs, trace, ref, att, bank, fixed_point=False, label=None):
    """what every GPU test asserts of a form's session: the oracle's call trace, the bound at every output, exact zeros, the coverage.
    Returns (worst error / bound, outputs compared, weights below 2^-24 pinned) for profiles/fir_taps.txt."""
    want_outs, want_trace = ref["outs"], ref["trace"]
    assert trace == want_trace, (name, trace, want_trace)
    misses, ratio = compare(att, bank, form, outs, want_outs)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"fir_taps {name} {label or form}: worst error/bound {worst:.4g}, {int(np.count_nonzero(att['k'] >= 0))} outputs attributed, "
          f"{small_weights(att)} weights below 2^-24")
    assert not misses.any(), name + "\n" + report(att, outs, want_outs, misses, ratio)
    # Coverage: a form shows a weight where the reference shows one — except where the bound itself admits a zero (|want| <= bound: fixed-point
    # rows on the 2^-30 grid lose the weights below its half step; a matrix form's row at the lattice position has the cleared end tap of
    # phase 0 at exactly 0 where the reference's rounded position gives it 1e-20), and never anywhere else.  The forms that blend with the
    # output's own fraction (general kernel, 8-byte matrix kernel) admit no such zero: equality.
    have, need = coverage(att, outs), coverage(att)
    b = bound(att, bank, form)
    o, c = np.nonzero((att["k"] >= 0) & (np.abs(att["value"].astype(np.float64)) > b))
    must = set(zip(att["phase"][o].tolist(), att["k_lat"][o, c].tolist()))
    assert must <= have <= need, (name, sorted(must - have)[:10], sorted(have - need)[:10])
    if form == "general":
        assert have == need, (name, sorted(need - have)[:10])
    if not fixed_point:
        assert len(need - have) <= 1, (name, sorted(need - have)[:10])
    return worst, int(np.count_nonzero(att["k"] >= 0)), small_weights(att)


# ------------------------------------------------------------------------------------------------------------------------
# the product's side (GPU)
# ------------------------------------------------------------------------------------------------------------------------
# form id -> (kernel preference, extra flags, which bound).  'general' bound: the output's own fraction; 'f32': rows at the slot's
# lattice position; 'i8': those rows on the 2^-30 grid
FORMS = {
    "general":         (1, 0, "general"),
    "general_precise": (1, PRECISE, "general"),
    "one_tile":        (5, 0, "f32"),
    "stream":          (6, 0, "f32"),
    "split":           (8, 0, "f32"),
    "fixed":           (7, 0, "i8"),
    "cut_invariant":   (9, 0, "f32"),
    "wide":            (2, 0, "general"),
}


def make_hip(case, pref, extra=0, width=32):
    import audio_resampler_amd as A
    ch, T, F, src, dst, fixed, flags = case[:7]
    r = A.binding(width).Resampler(ch, T, F, 0.0, flags | extra, (float(src), float(dst), 0) if fixed else None)
    r.set_kernel(pref)
    r.advance(T / 2)
    return r


def play_hip(sid, form):
    """the session on the library under a kernel preference: (outs, trace, kinds): kinds[call] = (last_kernel, fixed_point state,
    fixed_point_kernel) — the flush's too"""
    case, x, calls, meta = _prepared[sid][:4] if sid in _prepared else session_of(sid)
    pref, extra, _ = FORMS[form]
    r = make_hip(case, pref, extra, SESSIONS[sid][2])
    ratio = case[4] / case[3]
    outs, trace, kinds, pos = [], [], [], 0
    for n in list(calls) + [-1]:
        if n >= 0:
            u, g, y = r.process(x[pos:pos + n], int(n * ratio) + 2 * case[1] + 64, 0.0 if case[5] else ratio)
        else:
            u, g, y = r.process(None, 4 * case[1] + 64, ratio, flush=True)
        outs.append(np.array(y[:g], copy=True)); trace.append((int(u), int(g), float(r.position()))); pos += u
        kinds.append((int(r.last_kernel()), int(r.fixed_point()[0]) if SESSIONS[sid][2] == 32 else 0, r.fixed_point_kernel() if SESSIONS[sid][2] == 32 else None))
    fallbacks = int(r.cut_invariant_fallbacks()) if pref == 9 else 0
    r.close()
    return outs, trace, kinds, fallbacks
