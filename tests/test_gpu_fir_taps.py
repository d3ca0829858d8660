"""GPU (-m gpu): every forward FIR kernel form pinned TAP BY TAP on impulse trains (tests/_fir_taps.py: the instrument, the bound and
its derivation; tests/test_fir_taps_ref.py: that the instrument can fail).  The parity bar (2^-23 at full scale, white noise in every
channel) cannot see one weight wrong by less than 2.4e-7 / |x|, a weight of the window's tails dropped or misplaced, or crosstalk
below the bar; a session hash says that something moved, not where.  Here every output holds at most one product, so each is ONE
weight of the operator: within the derived bound of the strict oracle's value, exactly zero where the oracle is zero, the same
(phase, tap) coverage as the oracle, the oracle's call trace — and the kernel form that was meant to run is asserted to have run.

Sizes: two calls of 24,000 and 21,000 frames and a flush (test_gpu_fixed_point.py asserts the fixed-point kernel from 20,000 frames on;
the same calls for every form, so that one reference serves them all); the stereo, mono and downsampling trains are longer because
fewer impulses per frame reach them (tests/_fir_taps.py CASES)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _fir_taps as FT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

REGISTER_STAGED = ("stereo", "mono")                      # one or two channels per column group: fir_i8_stream_kernel
IN_GROUPS = ("ch6", "ch33")                               # no compiled width: fir_in_groups


def _assert_kinds(name, form, kinds, env=None):
    """the kernel form that was meant to run did run, in every call (the flush is the general kernel's everywhere)"""
    *calls, flush = kinds
    assert flush[0] == 1, (name, form, kinds)
    for last, state, i8 in calls:
        if form.startswith("general"):
            assert last == 1 and state == 0, (name, form, kinds)
        elif form == "fixed":
            assert last == 2 and state == 1, (name, form, kinds)
            if env and env.get("ARTAMD_I8_SLAB_MIN") == "1" and name not in REGISTER_STAGED:
                assert i8 == "fir_i8_slab_kernel", (name, form, kinds)
            elif name not in IN_GROUPS:
                assert i8 == ("fir_i8_stream_kernel" if name in REGISTER_STAGED else "fir_i8_dma_kernel"), (name, form, kinds)
            else:
                assert i8 in ("fir_i8_stream_kernel", "fir_i8_dma_kernel"), (name, form, kinds)
        else:
            assert last == 2 and state == 0 and i8 is None, (name, form, kinds)


def _check(sid, form, outs, trace, kinds, env=None):
    case, x, calls, meta, ref, att = FT.prepared(sid)
    _assert_kinds(FT.SESSIONS[sid][0], form, kinds, env)
    return FT.check(sid + ("" if not env else "[" + ",".join(f"{k}={v}" for k, v in env.items()) + "]"), FT.FORMS[form][2], outs, trace, ref, att,
                    ref["bank"], fixed_point=form == "fixed", label=form)


@pytest.mark.parametrize("form", ["general", "general_precise", "one_tile", "stream", "split", "fixed"])
@pytest.mark.parametrize("name", list(FT.CASES))
def test_every_tap_of_every_form(name, form):
    outs, trace, kinds, _ = FT.play_hip(name, form)
    _check(name, form, outs, trace, kinds)


@pytest.mark.parametrize("sid", ["headline_wide", "nearest_wide"])
def test_every_tap_of_the_8_byte_matrix_kernel(sid):
    """double samples: the same bound with the double's spacing (the kernel blends with the output's own fraction)"""
    outs, trace, kinds, _ = FT.play_hip(sid, "wide")
    assert all(k[0] == 2 for k in kinds[:-1]) and kinds[-1][0] == 1, kinds
    case, x, calls, meta, ref, att = FT.prepared(sid)
    assert outs[0].dtype == np.float64
    FT.check(sid, "general", outs, trace, ref, att, ref["bank"], label="wide")


@pytest.mark.parametrize("sid", ["headline_cuts", "downsampling_cuts"])
def test_every_tap_under_the_cut_invariant_policy_in_calls_of_1_to_400_frames(sid):
    """anchored launches, n_skip, launches shorter than a period: the same train, the same bound, and not one fallback"""
    case, x, calls, meta, ref, att = FT.prepared(sid)
    assert calls[0] < FT.period(case)[1] and max(calls) <= 400 and min(calls) >= 1
    outs, trace, kinds, fallbacks = FT.play_hip(sid, "cut_invariant")
    assert fallbacks == 0
    for (u, g, _), (last, state, i8) in list(zip(trace, kinds))[:-1]:
        assert g == 0 or (last == 2 and state == 0), (u, g, last, state)
    FT.check(sid, "f32", outs, trace, ref, att, ref["bank"], label="cut_invariant")


def test_every_tap_of_a_grouped_launch():
    """three stereo contexts, each with its own train, through resampleProcessBatchInterleavedDevice at preference 6: from the second
    call on (the first builds each stream's rows) their launches are gathered into one"""
    import torch
    import audio_resampler_amd as A
    B = A.binding(32)
    sids = ["stereo", "stereo_plus131", "stereo_plus262"]
    prep = [FT.prepared(s) for s in sids]
    case, calls = prep[0][0], prep[0][2]
    ratio = case[4] / case[3]
    rs = [FT.make_hip(case, 6) for _ in sids]
    outs, traces, pos = [[] for _ in sids], [[] for _ in sids], 0
    for j, n in enumerate(calls):
        cap = int(n * ratio) + 2 * case[1] + 64
        d_in = [torch.from_numpy(np.ascontiguousarray(p[1][pos:pos + n])).cuda() for p in prep]
        d_out = [torch.zeros(cap, case[0], device="cuda") for _ in sids]
        res = B.process_batch_device(rs, d_in, [n] * len(sids), d_out, [cap] * len(sids), [ratio] * len(sids))
        for i, (u, g) in enumerate(res):
            assert u == n and rs[i].last_kernel() == 2 and rs[i].fixed_point()[0] == 0, (j, i, u, g, rs[i].last_kernel())
            if j >= 1:
                assert rs[i].last_gathered() == 1, (j, i)
            outs[i].append(d_out[i][:g].cpu().numpy().copy()); traces[i].append((int(u), int(g), float(rs[i].position())))
        pos += n
    for i, sid in enumerate(sids):
        u, g, y = rs[i].process(None, 4 * case[1] + 64, ratio, flush=True)          # (the flush has no grouped form: singly, the general kernel)
        assert rs[i].last_kernel() == 1
        outs[i].append(np.array(y[:g], copy=True)); traces[i].append((int(u), int(g), float(rs[i].position())))
        _, _, _, _, ref, att = prep[i]
        FT.check(sid + "[grouped]", "f32", outs[i], traces[i], ref, att, ref["bank"], label="stream")
    for r in rs:
        r.close()


# ARTAMD_I8_SLAB_MIN=1: fir_i8_slab_kernel on these small launches, most of its 64-slot tiles cut by stream-K; ARTAMD_ROWS_CACHE=0: every
# launch on rows built from its own positions, tiles anchored on its own first output.  Read once per process: one child per switch.
SWITCHED = {
    "slabs_everywhere": ({"ARTAMD_I8_SLAB_MIN": "1"}, [(n, "fixed") for n in ("headline", "downsampling", "nearest", "short_period", "ch16", "ch32")]),
    "no_kept_rows": ({"ARTAMD_ROWS_CACHE": "0"}, [(n, f) for n in ("headline", "nearest", "short_period", "stereo") for f in ("stream", "fixed")]),
}


@pytest.mark.parametrize("which", list(SWITCHED))
def test_every_tap_under_the_process_wide_switches(which, tmp_path):
    env, items = SWITCHED[which]
    p = subprocess.run([sys.executable, os.path.join(HERE, "_fir_taps_sessions.py"), str(tmp_path)] + [f"{n}:{f}" for n, f in items],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]             # (a child that fails ends the test here)
    with open(tmp_path / "record.json") as f:
        record = json.load(f)
    for n, form in items:
        rec = record[f"{n}:{form}"]
        outs = [np.load(tmp_path / f"{n}.{form}.{i}.npy") for i in range(rec["calls"])]
        _check(n, form, outs, [tuple(t) for t in rec["trace"]], [tuple(k) for k in rec["kinds"]], env)
