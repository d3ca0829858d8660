"""CPU: the impulse-train instrument of tests/_fir_taps.py on the oracle alone — that its reference is unambiguous, that its
attribution IS the oracle, that its trains show every weight of the operator, and that it CAN FAIL: a bank doctored below what the
parity bar sees (tolerance_ok on artest noise passes) is flagged at exactly the doctored (phase, tap) slots."""
import numpy as np
import pytest

import _fir_taps as FT
from _hip import tolerance_ok
from _oracle import noise

SIDS = list(FT.SESSIONS)


def _bits(a):
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.parametrize("sid", SIDS)
def test_strict_and_precise_oracles_agree_bit_for_bit_on_the_train(sid):
    case, x, calls, meta, ref, att = FT.prepared(sid)
    width = FT.SESSIONS[sid][2]
    precise = FT.reference(case, x, calls, precise=True, width=width)
    assert precise["trace"] == ref["trace"]
    for a, b in zip(ref["outs"], precise["outs"]):
        assert np.array_equal(_bits(a), _bits(b))
    # the train itself: no window holds two impulses, signed powers of two, one silent channel beside the live ones
    assert meta["spacing"] >= case[1] + 4
    amps = np.array(meta["amps"])
    live = amps != 0
    assert np.all(np.abs(np.log2(np.abs(amps[live]))) % 1 == 0)
    assert case[0] == 1 or (not live[-1] and not x[:, -1].any())
    assert all(np.count_nonzero(x[:, c]) >= 20 for c in range(case[0]) if live[c])
    # impulses on both sides of the first call boundary
    edge = calls[0] if FT.SESSIONS[sid][3] is None else sum(calls) // 2
    assert x[:edge].any() and x[edge:].any()


@pytest.mark.parametrize("sid", SIDS)
def test_attribution_is_the_oracle_and_the_train_shows_every_weight(sid):
    case, x, calls, meta, ref, att = FT.prepared(sid)
    want = np.concatenate(ref["outs"])
    assert np.array_equal(att["value"], want)
    assert not np.any(want[att["k"] < 0])                          # nothing where no impulse is attributed
    if not att["interp"]:
        # nearest filter: one bank entry (or the sample itself) times the amplitude, bit for bit
        o, c = np.nonzero(att["k"] >= 0)
        fi, k = att["fi"][o], att["k"][o, c]
        w = np.where(att["passthrough"][o], 1.0, ref["bank"][fi, k].astype(np.float64))
        assert np.array_equal((w * att["amp"][c]).astype(want.dtype), want[o, c])
        if sid.startswith("nearest"):
            assert att["passthrough"].any()
    # the comparator on the reference itself: nothing to flag, under the tightest form
    misses, ratio = FT.compare(att, ref["bank"], "general", ref["outs"], ref["outs"])
    assert not misses.any() and ratio.max() == 0.0
    if FT.SESSIONS[sid][1] == 0:                                   # (the moved trains of the grouped launch: the same weights at other frames)
        need, have = FT.required_coverage(case, ref), FT.coverage(att)
        assert need <= have, sorted(need - have)[:10]
        assert len(have - need) <= 1                               # (the cleared end tap of phase 0, where a position rounds off the whole frame)
        assert case[8] >= FT.search_spacing(case, sum(case[7]))


def _doctored(doctor):
    """the headline session through an oracle whose bank `doctor` has changed in place"""
    case, x, calls, meta, ref, att = FT.prepared("headline")
    r = FT.make_oracle(case)
    doctor(FT.bank_view(r))
    return FT.reference(case, x, calls, oracle=r), r


def _noise_passes_the_parity_bar(doctor):
    """artest noise (peak 0.5) through the doctored bank against the true one, double accumulate both: what the suite's bar sees"""
    case = FT.CASES["headline"]
    x, _ = noise(6000 * case[0]); x = x.reshape(-1, case[0])
    bad, good = FT.make_oracle(case, precise=True), FT.make_oracle(case, precise=True)
    doctor(FT.bank_view(bad))
    yb, yg = bad.process(x, 8000, 48000 / 44100, and_flush=True)[2], good.process(x, 8000, 48000 / 44100, and_flush=True)[2]
    assert not np.array_equal(yb, yg)
    return tolerance_ok(yb, yg)[0]


PHASE = 37          # one of the headline's 160 (its two filter rows are no other phase's: _phase_filter)


def _phase_filter():
    case, x, calls, meta, ref, att = FT.prepared("headline")
    fi = np.unique(att["fi"][att["phase"] == PHASE])
    assert len(fi) == 1
    # no other phase blends with rows fi, fi + 1 (or fi + 2, which doctoring (c) reads)
    others = np.unique(att["fi"][att["phase"] != PHASE])
    assert not set(range(int(fi[0]) - 1, int(fi[0]) + 3)) & set(others.tolist())
    return int(fi[0])


def _flagged(doctor, form="f32"):
    case, x, calls, meta, ref, att = FT.prepared("headline")
    got, _ = _doctored(doctor)
    assert got["trace"] == ref["trace"]
    misses, ratio = FT.compare(att, ref["bank"], form, got["outs"], ref["outs"])
    return FT.missed_slots(att, misses), FT.report(att, got["outs"], ref["outs"], misses, ratio), misses


def test_a_dropped_end_tap_is_flagged_where_the_parity_bar_is_blind():
    fi = _phase_filter()
    T = FT.CASES["headline"][1]

    def doctor(bank):
        assert 0 < abs(bank[fi, T - 1]) < 2.0 ** -24
        bank[fi, T - 1] = 0.0
    slots, text, misses = _flagged(doctor)
    assert slots == {(PHASE, T - 1)}, text
    case, x, calls, meta, ref, att = FT.prepared("headline")
    there = (att["phase"] == PHASE)[:, None] & (att["k"] == T - 1)
    assert there.any() and np.array_equal(misses, there)                      # every output that reads the tap, and no other
    assert _noise_passes_the_parity_bar(doctor)


def test_a_tap_off_by_one_part_in_ten_thousand_is_flagged_where_the_parity_bar_is_blind():
    fi = _phase_filter()
    case, x, calls, meta, ref, att = FT.prepared("headline")
    k = int(np.argmin(np.abs(np.abs(ref["bank"][fi].astype(np.float64)) - 1e-3)))          # a mid-sized tap: |h| about 1e-3

    def doctor(bank):
        assert 5e-4 < abs(bank[fi, k]) < 2e-3
        bank[fi, k] = np.float32(bank[fi, k] * (1 + 1e-4))
    slots, text, misses = _flagged(doctor)
    assert slots == {(PHASE, k)}, text
    assert f" {PHASE} " in text.splitlines()[2] and f" {k} {k // 32} " in text.splitlines()[2]
    assert _noise_passes_the_parity_bar(doctor)


def test_a_neighbouring_filter_in_one_phase_is_localised_to_that_phase():
    """gross (the parity bar sees it too): what is checked is that the report points at the phase, all over its taps"""
    fi = _phase_filter()

    def doctor(bank):
        bank[fi], bank[fi + 1] = bank[fi + 1].copy(), bank[fi + 2].copy()
    slots, text, misses = _flagged(doctor)
    assert {p for p, _ in slots} == {PHASE}, text
    assert len(slots) >= 0.9 * FT.CASES["headline"][1], len(slots)
    assert all(line.split()[2] == str(PHASE) for line in text.splitlines()[2:22])
    assert "misses by (n mod 64, k // 32)" in text and "misses by channel" in text
    assert not _noise_passes_the_parity_bar(doctor)


def test_bounds_are_the_derived_ones():
    """one float spacing where there is no fraction; the slope term at MF_PHASE_TOL for the matrix forms; 2^-31 of the amplitude more in fixed point"""
    case, x, calls, meta, ref, att = FT.prepared("nearest")
    b = FT.bound(att, ref["bank"], "f32")
    live = att["k"] >= 0
    want = np.abs(att["value"].astype(np.float64))
    assert np.all(b[~live] == 0.0)
    assert np.all(b[live] == 2.0 ** (np.floor(np.log2(np.maximum(want[live], 2.0 ** -126))) - 23))
    case, x, calls, meta, ref, att = FT.prepared("headline")
    bg, bf, bi = (FT.bound(att, ref["bank"], f) for f in ("general", "f32", "i8"))
    live = att["k"] >= 0
    assert np.all(bg[live] <= bf[live]) and np.all(bf[live] < bi[live])
    amp = np.broadcast_to(np.abs(att["amp"])[None, :], bi.shape)
    assert np.allclose((bi - bf)[live], amp[live] * 2.0 ** -31, rtol=1e-9, atol=0)
    slope = np.abs(att["h1"] - att["h0"])
    inner = live & ((att["frac"] > 1e-5) & (att["frac"] < 1 - 1e-5))[:, None]
    spacing = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(att["value"].astype(np.float64)), 2.0 ** -126))) - 23)
    assert np.allclose(bf[inner], (spacing + amp * slope * FT.MF_PHASE_TOL)[inner], rtol=1e-12, atol=0)
    assert FT.eps_pos("general", 988, 988) < 5e-9
