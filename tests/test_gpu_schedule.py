"""GPU: resampleProcessScheduleInterleavedDevice — many blocks of one stream in one call — against the loop of single calls it stands for
(art_hip.h).  Every case drives twin contexts: one calls the schedule, the other makes the blocks one by one
(resampleProcessInterleavedDevice, resampleProcessAndFlushInterleavedDevice for a flushed last block).  Compared: the results, the packed
outputs bit for bit, and one more ordinary call afterwards (position and history)."""
import hashlib
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _asrc_sessions import SESSIONS  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
R = 48000 / 44100
BH, INTERP, LOWPASS, PRECISE = 0x2, 0x1, 0x4, 0x100
STRICT, EXTRAP = 0x10000, 0x40
KERNEL_GENERAL, KERNEL_MFMA = 1, 2


def config_e_ratio(i):
    """config E's ratio sequence (bench.py): every 32nd entry is exactly 160/147"""
    return R * (1 + 100e-6 * math.sin(2 * math.pi * i / 64))


def _binding(width):
    import audio_resampler_amd as A
    return A.binding(width)


def _torch_dtype(width):
    import torch
    return torch.float64 if width == 64 else torch.float32


def _cap(n, ratio):
    return int(n * ratio) + 64


class Twins:
    """a context that takes the schedule and one that makes the single calls, fed from one device input"""

    def __init__(self, width, make, prep=None, frames=0, channels=2, seed=1):
        import torch
        self.W, self.A = width, _binding(width)
        self.sched, self.single = make(self.A), make(self.A)
        for r in (self.sched, self.single):
            if prep:
                prep(r)
        self.C = channels
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((frames + 4096, channels)) * 0.25).astype(np.float64 if width == 64 else np.float32)
        self.x = torch.from_numpy(x).cuda()
        self.pos = 0
        self.torch = torch

    def _out(self, frames):
        return self.torch.zeros((max(frames, 1), self.C), dtype=_torch_dtype(self.W), device="cuda")

    def schedule(self, n_ins, caps, ratios, flush_last=False):
        """one schedule on one twin, the loop on the other; returns (blocks made, results) after comparing them"""
        d_in = self.x[self.pos:]
        out_a, out_b = self._out(sum(caps)), self._out(sum(caps))
        made, res = self.sched.process_schedule_device(d_in, n_ins, out_a, caps, ratios, flush_last)
        ref, in_off, out_off, ref_made = [], 0, 0, 0
        for k, (n, cap, ratio) in enumerate(zip(n_ins, caps, ratios)):
            u, g = self.single.process_device(self.x[self.pos + in_off:], n, out_b[out_off:], cap, ratio,
                                              and_flush=flush_last and k == len(n_ins) - 1)
            ref.append((u, g))
            ref_made = k + 1
            in_off += n
            out_off += g
            if u != n:
                break
        ref += [(0, 0)] * (len(n_ins) - len(ref))
        assert made == ref_made and res == ref, (made, res, ref_made, ref)
        self.torch.cuda.synchronize()
        a, b = out_a[:out_off].cpu().numpy(), out_b[:out_off].cpu().numpy()
        assert hashlib.sha256(a.tobytes()).hexdigest() == hashlib.sha256(b.tobytes()).hexdigest(), \
            f"outputs differ: {int(np.sum(a != b))} of {a.size} samples"
        self.pos += in_off
        return made, res

    def follow_up(self, n=3000, ratio=R):
        """one more ordinary call on both: the same position, the same history"""
        assert self.sched.state() == self.single.state()
        outs = []
        for r in (self.sched, self.single):
            d_out = self._out(_cap(n, ratio))
            outs.append((r.process_device(self.x[self.pos:], n, d_out, _cap(n, ratio), ratio), d_out.cpu().numpy()))
        assert outs[0][0] == outs[1][0]
        assert np.array_equal(outs[0][1], outs[1][1])
        assert self.sched.state() == self.single.state()

    def play(self, blocks, ratios, K):
        for j in range(0, len(blocks), K):
            n_ins = blocks[j:j + K]
            self.schedule(n_ins, [_cap(n, r) for n, r in zip(n_ins, ratios[j:j + K])], ratios[j:j + K])


WIDTHS = [32, 64]
SESSION_IDS = [f"{ch}ch_{T}x{F}_{flags:#x}_{i}" for i, (ch, T, F, _r, flags, _b, _p) in enumerate(SESSIONS)]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("session", range(len(SESSIONS)), ids=SESSION_IDS)
def test_asrc_sessions_as_schedules(session, width):
    ch, T, F, ratios, flags, blocks, pref = SESSIONS[session]
    per_block = [ratios[i % len(ratios)] for i in range(len(blocks))]
    for K in (1, 3, 16):
        tw = Twins(width, lambda A: A.Resampler(ch, T, F, 0.0, flags), lambda r: (r.advance(T / 2), r.set_kernel(pref)),
                   frames=sum(blocks) + 3000, channels=ch, seed=session * 7 + K)
        tw.play(list(blocks), per_block, K)
        tw.follow_up()


@pytest.mark.parametrize("width", WIDTHS)
def test_short_filter_blocks_of_many_ring_epochs(width):
    """16 taps, 65,536-frame blocks: ~270 ring epochs per block, more than a launch's 192-segment table"""
    blocks = [65536] * 4
    ratios = [config_e_ratio(i) for i in range(1, 5)]
    tw = Twins(width, lambda A: A.Resampler(2, 16, 16, 0.0, BH | INTERP), lambda r: r.advance(8), frames=sum(blocks) + 3000)
    tw.play(blocks, ratios, 4)
    tw.follow_up()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("advance", [False, True], ids=["fresh", "advanced"])
def test_stream_start_and_edges(width, advance):
    T = 380
    tw = Twins(width, lambda A: A.Resampler(2, T, T, 0.0, BH | INTERP), (lambda r: r.advance(T / 2)) if advance else None, frames=40000)
    # blocks shorter than T / 2 at the stream's start (the first outputs read the zeroed history), zero-frame blocks, a cap of 0
    n_ins = [100, 0, 150, 50, 0, 3000, 2000]
    ratios = [R * 1.00002, R, 0.9, R * 0.99997, 1.3, R * 1.00001, R]
    caps = [_cap(n, r) for n, r in zip(n_ins, ratios)]
    caps[3] = 0 if advance else caps[3]
    tw.schedule(n_ins[:3], caps[:3], ratios[:3])
    made, res = tw.schedule(n_ins[3:], caps[3:], ratios[3:])
    if advance:                      # the cap of 0 stops the schedule at that block
        assert made == 1 and res[1:] == [(0, 0)] * 3
    else:
        assert made == 4
    # a block capped too small: the schedule stops there, the blocks after it are not made
    n_ins, ratios = [4000, 5000, 3000, 2000], [R] * 4
    caps = [_cap(4000, R), 1000, _cap(3000, R), _cap(2000, R)]
    made, res = tw.schedule(n_ins, caps, ratios)
    assert made == 2 and res[1][1] == 1000 and res[1][0] < 5000 and res[2:] == [(0, 0), (0, 0)]
    tw.follow_up()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("flags", [BH | INTERP, BH], ids=["interpolating", "nearest"])
def test_flush_last(width, flags):
    T = 380
    tw = Twins(width, lambda A: A.Resampler(2, T, T, 0.0, flags), lambda r: r.advance(T / 2), frames=60000)
    n_ins = [16384, 4096, 16384, 5000]
    ratios = [config_e_ratio(i) for i in range(1, 5)]
    caps = [_cap(n, r) + T for n, r in zip(n_ins, ratios)]
    made, res = tw.schedule(n_ins, caps, ratios, flush_last=True)
    assert made == 4 and res[-1][0] == 5000


@pytest.mark.parametrize("width", WIDTHS)
def test_fixed_ratio_stream_mixes_small_blocks_and_a_matrix_block(width):
    """kept rows on (the default): the gathered blocks look after the canonical period as their single calls do"""
    blocks = [4096, 16384, 4096, 300000, 4096, 16384, 4096]
    tw = Twins(width, lambda A: A.Resampler(2, 380, 380, 0.0, BH, fixed=(44100, 48000, 0)), frames=sum(blocks) + 3000)
    tw.play(blocks, [R] * len(blocks), len(blocks))
    tw.follow_up()


@pytest.mark.parametrize("width", WIDTHS)
def test_config_e_schedule_splits_at_the_rational_ratio(width):
    """config E's sequence at 65,536-frame blocks: entry 32 is exactly 160/147, which the matrix path takes — the run is cut there"""
    blocks = [65536] * 32
    ratios = [config_e_ratio(i) for i in range(1, 33)]
    assert ratios[-1] == R
    tw = Twins(width, lambda A: A.Resampler(2, 380, 380, 0.0, BH), lambda r: r.advance(190), frames=sum(blocks) + 3000)
    tw.play(blocks, ratios, 32)
    if width == 32:
        assert tw.sched.last_kernel() == KERNEL_MFMA and tw.single.last_kernel() == KERNEL_MFMA
    assert tw.sched.last_kernel() == tw.single.last_kernel()
    tw.follow_up()


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("case", ["cut_invariant", "strict", "extrapolate", "extend"])
def test_contexts_made_call_by_call_or_gathered(width, case):
    blocks = [4096, 16384, 4096, 70000, 4096]
    if case == "cut_invariant":
        make, prep, ratios = (lambda A: A.Resampler(2, 380, 380, 0.0, BH, fixed=(44100, 48000, 0))), (lambda r: r.set_cut_invariant(True)), [R] * 5
    else:
        flags = BH | INTERP | {"strict": STRICT, "extrapolate": EXTRAP, "extend": PRECISE}[case]
        make, prep = (lambda A: A.Resampler(2, 256, 256, 0.0, flags)), None
        ratios = [config_e_ratio(i) for i in range(1, 6)]
    tw = Twins(width, make, prep, frames=sum(blocks) + 3000)
    tw.play(blocks, ratios, 5)
    assert tw.sched.cut_invariant_fallbacks() == tw.single.cut_invariant_fallbacks()
    tw.follow_up()


@pytest.mark.parametrize("width", WIDTHS)
def test_sixteen_blocks_are_one_launch(width):
    blocks = [65536] * 16
    ratios = [config_e_ratio(i) for i in range(1, 17)]
    assert all(r != R for r in ratios)
    tw = Twins(width, lambda A: A.Resampler(2, 380, 380, 0.0, BH), lambda r: (r.advance(190), r.set_timing(True)), frames=sum(blocks) + 3000)
    tw.play(blocks, ratios, 16)
    ms_a, launches_a = tw.sched.read_timing()
    ms_b, launches_b = tw.single.read_timing()
    assert launches_a == 1 and launches_b == 16, (launches_a, launches_b)
    assert ms_a > 0.0 and tw.sched.last_kernel() == KERNEL_GENERAL


CHILD = r'''
import sys, json, hashlib, math
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import audio_resampler_amd as A
L = A.lib()
R = 48000 / 44100
ratios = [R * (1 + 100e-6 * math.sin(2 * math.pi * i / 64)) for i in range(1, 9)]
n_ins = [16384] * 8
caps = [int(n * r) + 64 for n, r in zip(n_ins, ratios)]
rng = np.random.default_rng(5)
x = torch.from_numpy((rng.standard_normal((sum(n_ins), 2)) * 0.25).astype(np.float32)).cuda()
r = A.Resampler(2, 380, 380, 0.0, A.BLACKMAN_HARRIS); r.advance(190)
d_out = torch.zeros((sum(caps), 2), device="cuda")
log, k, pos, out_pos = [], 0, 0, 0
while k < len(n_ins):
    before = r.state()
    try:
        made, res = r.process_schedule_device(x[pos:], n_ins[k:k + 4], d_out[out_pos:], caps[k:k + 4], ratios[k:k + 4])
    except RuntimeError:
        assert tuple(r.state()) == tuple(before), (before, r.state())
        log.append(("failed", k, L.artamdErrorCount()))
        continue
    for u, g in res[:made]:
        pos += u; out_pos += g
    k += made
torch.cuda.synchronize()
y = d_out[:out_pos].cpu().numpy()
print(json.dumps({"sha256": hashlib.sha256(y.tobytes()).hexdigest(), "frames": out_pos, "errors": L.artamdErrorCount(), "log": log}))
'''


def _child(fail_at):
    env = dict(os.environ)
    env.pop("ARTAMD_TEST_FAIL_FIR", None)
    if fail_at:
        env["ARTAMD_TEST_FAIL_FIR"] = str(fail_at)
    p = subprocess.run([sys.executable, "-c", CHILD % dict(root=os.path.dirname(HERE), tests=HERE)], capture_output=True, text=True,
                       env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_a_failed_run_moves_nothing_and_is_counted():
    """ARTAMD_TEST_FAIL_FIR=k fails the k-th FIR launch of the process on the host, before anything is enqueued: here a run's launch"""
    clean, _ = _child(0)
    assert clean["errors"] == 0 and clean["log"] == []
    for fail_at in (1, 2):
        got, err = _child(fail_at)
        assert got["errors"] == 1 and len(got["log"]) == 1 and got["log"][0][1] == 4 * (fail_at - 1), got
        assert "schedule launch failed" in err
        assert got["frames"] == clean["frames"] and got["sha256"] == clean["sha256"], (fail_at, got, clean)
