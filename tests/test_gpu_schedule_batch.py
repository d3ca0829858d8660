"""GPU: the schedule entries for many streams and for planes (art_hip.h) — resampleProcessScheduleBatchInterleavedDevice,
resampleProcessScheduleBatchPlanarDevice, resampleProcessSchedulePlanarDevice — against the loop of single
resampleProcessScheduleInterleavedDevice calls they stand for.  Every stream of a case has twin contexts: one is an item of the batch
call, the other takes its own interleaved schedule (on transposed copies where the item is planar).  Compared per stream: blocksMade,
every result, the packed outputs bit for bit (and the padding of output planes, which must keep its sentinel), state(), last_kernel(),
last_gathered(), cut_invariant_fallbacks(), and one more ordinary call on both twins."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
R = 48000 / 44100
BH, INTERP, PRECISE = 0x2, 0x1, 0x100
STRICT, EXTRAP = 0x10000, 0x40
KERNEL_GENERAL = 1
SENTINEL = -7.25
WIDTHS = [32, 64]


def _cap(n, ratio, extra=0):
    return int(n * ratio) + 64 + extra


class Item:
    """one stream of a batch call: its twin contexts, its input in the item's layout and interleaved, its two outputs.
    in_pad / out_pad: None = that side interleaved, else the planes' pitch exceeds the frames by that many samples"""

    def __init__(self, make, prep=None, channels=2, n_ins=(), ratios=(), caps=None, flush=False, in_pad=None, out_pad=None, taps=0):
        self.make, self.prep, self.C = make, prep, channels
        self.n_ins, self.ratios, self.flush = list(n_ins), list(ratios), flush
        self.caps = list(caps) if caps is not None else [_cap(n, r, taps if flush else 0) for n, r in zip(self.n_ins, self.ratios)]
        self.in_pad, self.out_pad = in_pad, out_pad

    def build(self, B, width, seed):
        import torch
        self.torch, self.dtype = torch, (torch.float64 if width == 64 else torch.float32)
        self.batch, self.loop = self.make(B), self.make(B)
        for r in (self.batch, self.loop):
            if self.prep:
                self.prep(r)
        frames = sum(self.n_ins) + 4096                       # (the follow-up call's input behind the blocks')
        rng = np.random.default_rng(seed)
        x = (rng.standard_normal((frames, self.C)) * 0.25).astype(np.float64 if width == 64 else np.float32)
        self.x = torch.from_numpy(x).cuda()
        self.in_pitch = 0 if self.in_pad is None else frames + self.in_pad
        if self.in_pitch:
            self.x_item = torch.full((self.C, self.in_pitch), 0.5, dtype=self.dtype, device="cuda")
            self.x_item[:, :frames] = self.x.T
        else:
            self.x_item = self.x
        room = max(sum(self.caps), 1)
        self.out_loop = torch.zeros((room, self.C), dtype=self.dtype, device="cuda")
        self.out_pitch = 0 if self.out_pad is None else room + self.out_pad
        if self.out_pitch:
            self.out_item = torch.full((self.C, self.out_pitch), SENTINEL, dtype=self.dtype, device="cuda")
        else:
            self.out_item = torch.zeros((room, self.C), dtype=self.dtype, device="cuda")

    def run_loop(self):
        if not self.n_ins:
            return 0, []
        return self.loop.process_schedule_device(self.x, self.n_ins, self.out_loop, self.caps, self.ratios, self.flush)

    def check(self, made, res, tag):
        ref_made, ref = self.run_loop()
        assert (made, res) == (ref_made, ref), (tag, made, res, ref_made, ref)
        self.torch.cuda.synchronize()
        frames = sum(g for _u, g in res)
        b = self.out_loop[:frames].cpu().numpy()
        if self.out_pitch:
            planes = self.out_item.cpu().numpy()
            a = np.ascontiguousarray(planes[:, :frames].T)
            assert np.all(planes[:, frames:] == SENTINEL), (tag, "the padding behind the planes' frames was written")
        else:
            a = self.out_item[:frames].cpu().numpy()
        assert a.tobytes() == b.tobytes(), (tag, f"outputs differ: {int(np.sum(a != b))} of {a.size} samples")
        self.same_state(tag)
        self.gathered, self.kernel = self.batch.last_gathered(), self.batch.last_kernel()      # (before the follow-up call)
        return frames

    def same_state(self, tag):
        for what in ("state", "last_kernel", "last_gathered", "cut_invariant_fallbacks"):
            assert getattr(self.batch, what)() == getattr(self.loop, what)(), (tag, what)

    def follow_up(self, tag, n=3000, ratio=R):
        """one more ordinary call on both twins: the same position, the same history"""
        pos, outs = sum(self.n_ins), []
        for r in (self.batch, self.loop):
            d_out = self.torch.zeros((_cap(n, ratio), self.C), dtype=self.dtype, device="cuda")
            self.torch.cuda.synchronize()
            outs.append((r.process_device(self.x[pos:], n, d_out, _cap(n, ratio), ratio), d_out))
        self.torch.cuda.synchronize()
        assert outs[0][0] == outs[1][0], tag
        assert np.array_equal(outs[0][1].cpu().numpy(), outs[1][1].cpu().numpy()), tag
        assert self.batch.state() == self.loop.state(), tag


def run_case(width, items, follow_up=True, seed=100):
    """the batch call over `items` (the planar entry where an item has a pitch) against every item's own schedule; returns
    (launches, [(made, results), ...])"""
    import torch
    import audio_resampler_amd as A
    B = A.binding(width)
    for i, it in enumerate(items):
        it.build(B, width, seed + i)
    torch.cuda.synchronize()
    flush = [it.flush for it in items] if any(it.flush for it in items) else None
    ctxs, d_ins, d_outs = [it.batch for it in items], [it.x_item for it in items], [it.out_item for it in items]
    n_ins, caps, ratios = [it.n_ins for it in items], [it.caps for it in items], [it.ratios for it in items]
    if any(it.in_pitch or it.out_pitch for it in items):
        in_p = [it.in_pitch for it in items] if any(it.in_pitch for it in items) else None
        out_p = [it.out_pitch for it in items] if any(it.out_pitch for it in items) else None
        launches, got = B.process_schedule_batch_planar_device(ctxs, d_ins, in_p, n_ins, d_outs, out_p, caps, ratios, flush)
    else:
        launches, got = B.process_schedule_batch_device(ctxs, d_ins, n_ins, d_outs, caps, ratios, flush)
    for i, (it, (made, res)) in enumerate(zip(items, got)):
        it.check(made, res, f"item {i}")
    if follow_up:
        for i, it in enumerate(items):
            if not it.flush:
                it.follow_up(f"item {i}")
    return launches, got


def plain(ch, T, F=None, flags=BH | INTERP):
    return lambda B: B.Resampler(ch, T, F or T, 0.0, flags)


def advanced(T):
    return lambda r: r.advance(T / 2)


def drifting(count, base=R, first=1):
    return [base * (1 + 100e-6 * math.sin(2 * math.pi * (first + i) / 64)) for i in range(count)]


def small_stream(blocks=(480, 480, 480), ch=2, T=380, first=1, **kw):
    return Item(plain(ch, T), advanced(T), ch, blocks, drifting(len(blocks), first=first), taps=T, **kw)


@pytest.mark.parametrize("width", WIDTHS)
def test_mixed_variants_in_one_call(width):
    """every channel group, every lane group, interpolating and nearest, EXTEND_CONVOLUTION_MATH; a stream at ratio ~0.25 beside one
    at ~2 (the launch's LDS is the largest any item needs)"""
    rng = np.random.default_rng(3)
    shapes = [(1, 16, BH | INTERP, R), (2, 256, BH | INTERP, R), (4, 380, BH, R), (8, 988, BH | INTERP, R), (2, 380, BH | INTERP | PRECISE, R),
              (2, 380, BH | INTERP, 0.25), (2, 380, BH | INTERP, 2.0), (1, 988, BH, R), (8, 256, BH | PRECISE, 0.9), (4, 16, BH | INTERP, 1.7)]
    items = []
    for i, (ch, T, flags, base) in enumerate(shapes):
        count = (1, 3, 7)[i % 3]
        blocks = [int(v) for v in rng.integers(100, 5001, count)]
        items.append(Item(plain(ch, T, min(T, 256), flags), advanced(T), ch, blocks, drifting(count, base, first=1 + i)))
    launches, got = run_case(width, items)
    assert all(made == len(it.n_ins) for it, (made, _r) in zip(items, got))
    assert launches >= 7                                  # (as many kernel variants at least: one fewer where EXTEND changes nothing)
    if width == 32:
        assert launches == 8 and all(it.gathered == 1 for it in items)


@pytest.mark.parametrize("width", WIDTHS)
def test_stream_starts_and_edges(width):
    T = 380
    short = [100, 0, 150, 50, 0, 3000, 2000]
    short_ratios = [R * 1.00002, R, 0.9, R * 0.99997, 1.3, R * 1.00001, R]
    zero_cap = [_cap(n, R) for n in (480, 480, 480, 480)]
    zero_cap[1] = 0
    small_cap = [_cap(4000, R), 1000, _cap(3000, R), _cap(2000, R)]
    items = [small_stream(),
             Item(plain(2, T), None, 2, short, short_ratios),                                        # blocks shorter than T / 2 on a fresh context, zero-frame blocks
             Item(plain(2, T), advanced(T), 2, [480] * 4, [R] * 4, caps=zero_cap),                   # a cap of 0
             Item(plain(2, T), advanced(T), 2, [4000, 5000, 3000, 2000], [R] * 4, caps=small_cap),   # a cap too small in the middle
             Item(plain(2, T), advanced(T), 2, [], []),                                              # numBlocks 0
             small_stream((1000, 300, 2000), first=9)]
    launches, got = run_case(width, items)
    assert got[0][0] == 3 and got[5][0] == 3 and got[1][0] == 7
    assert got[2][0] == 2 and got[2][1][1] == (0, 0) and got[2][1][2:] == [(0, 0), (0, 0)]
    made, res = got[3]
    assert made == 2 and res[1][1] == 1000 and res[1][0] < 5000 and res[2:] == [(0, 0), (0, 0)]
    assert got[4] == (0, [])
    # the call with n == 1
    launches, got = run_case(width, [small_stream((480, 960, 100, 480))], seed=7)
    assert launches == 1 and got[0][0] == 4


@pytest.mark.parametrize("width", WIDTHS)
def test_short_filter_blocks_of_many_ring_epochs(width):
    """16 taps x 65,536-frame blocks: ~270 ring epochs per block, so the segment array is per item"""
    long_a = Item(plain(2, 16), advanced(16), 2, [65536, 65536], drifting(2))
    long_b = Item(plain(2, 16), advanced(16), 2, [65536, 65536, 65536], drifting(3, first=5))
    launches, got = run_case(width, [long_a, small_stream(), long_b])
    assert [made for made, _r in got] == [2, 3, 3]
    assert launches >= 1 and long_a.gathered == 1 and long_b.gathered == 1


@pytest.mark.parametrize("width", WIDTHS)
def test_a_matrix_block_in_the_middle_takes_two_rounds(width):
    fixed = Item(lambda B: B.Resampler(2, 380, 380, 0.0, BH, fixed=(44100, 48000, 0)), None, 2, [4096, 300000, 4096], [R] * 3)
    items = [small_stream(flush=True), fixed, small_stream((480, 200, 960, 480), first=17)]
    launches, got = run_case(width, items)
    assert [made for made, _r in got] == [3, 3, 4]
    assert fixed.batch.last_kernel() == fixed.loop.last_kernel()
    # the shared launches of the two rounds, and the blocks made singly between them
    assert launches >= 3
    if width == 32:
        # (round one's two variants — the fixed-ratio stream is a nearest-filter one —, the matrix block, the flush, round two)
        assert fixed.gathered == 1 and launches == 5


@pytest.mark.parametrize("width", WIDTHS)
def test_contexts_made_on_the_side(width):
    import torch
    side = torch.cuda.Stream()
    blocks, T = [2048, 4096, 1000, 2048], 256
    ratios = drifting(4)
    items = [small_stream(),
             Item(plain(2, T, flags=BH | INTERP | STRICT), None, 2, blocks, ratios),
             Item(lambda B: B.Resampler(2, 380, 380, 0.0, BH, fixed=(44100, 48000, 0)), lambda r: r.set_cut_invariant(True), 2, blocks, [R] * 4),
             Item(plain(2, T, flags=BH | INTERP | EXTRAP), None, 2, blocks, ratios),
             Item(plain(2, T), lambda r: (r.advance(T / 2), r.set_timing(True)), 2, blocks, ratios),
             Item(plain(2, T), lambda r: (r.advance(T / 2), r.set_stream(side.cuda_stream)), 2, blocks, ratios)]
    launches, got = run_case(width, items)
    assert [made for made, _r in got] == [3, 4, 4, 4, 4, 4]
    assert items[0].gathered == 1
    assert items[3].gathered == 1            # the extrapolating stream's blocks behind its first output are gathered
    assert items[1].gathered == 0
    ms, timed = items[4].batch.read_timing()
    assert (ms > 0.0, timed) == (True, items[4].loop.read_timing()[1])


@pytest.mark.parametrize("width", WIDTHS)
def test_planar_items(width):
    """odd pitches that are no multiple of 4 and exceed the frames (the padding keeps its sentinel), planar and interleaved items in
    one call, one side planar only, a one-channel item"""
    items = [small_stream((480, 1001, 333), in_pad=13, out_pad=7),
             Item(plain(8, 256), advanced(256), 8, [1000, 2047, 480], drifting(3, first=3), in_pad=2, out_pad=3),
             small_stream((480, 480), first=5),                                           # interleaved on both sides
             small_stream((999, 480, 77), first=7, in_pad=5),                             # planes in, frames out
             small_stream((480, 2000), first=11, out_pad=9),                              # frames in, planes out
             Item(plain(1, 380), advanced(380), 1, [480, 1500], drifting(2, first=13), in_pad=3, out_pad=5),
             small_stream((480, 480, 480), first=15, in_pad=11, out_pad=1, flush=True)]
    assert all(it.in_pad is None or (sum(it.n_ins) + 4096 + it.in_pad) % 2 for it in items)      # (odd pitches)
    launches, got = run_case(width, items)
    assert [made for made, _r in got] == [len(it.n_ins) for it in items]
    assert all(it.gathered == (0 if it.flush else 1) for it in items)


@pytest.mark.parametrize("width", WIDTHS)
def test_the_single_planar_schedule(width):
    """resampleProcessSchedulePlanarDevice against the interleaved schedule on transposed copies: gathered runs, a matrix-path block
    in the middle, a flushed last block"""
    import torch
    import audio_resampler_amd as A
    B = A.binding(width)
    for ch, in_pad, out_pad in ((2, 13, 7), (8, 3, 0), (2, 0, 5)):
        blocks = [4096, 300000, 480, 2000] if ch == 2 else [4096, 1001, 480, 2000]
        it = Item(lambda B: B.Resampler(ch, 380, 380, 0.0, BH, fixed=(44100, 48000, 0)), None, ch, blocks, [R] * 4, flush=True, taps=380,
                  in_pad=in_pad or None, out_pad=out_pad or None)
        it.build(B, width, 40 + ch)
        torch.cuda.synchronize()
        made, res = it.batch.process_schedule_planar_device(it.x_item, it.in_pitch, it.n_ins, it.out_item, it.out_pitch, it.caps, it.ratios, True)
        it.check(made, res, f"{ch} channels")
        assert made == 4 and res[-1][0] == blocks[-1]


@pytest.mark.parametrize("width", WIDTHS)
def test_launch_count(width):
    """64 stereo streams x 4 blocks of one shape, all gatherable: one launch; a strict-order stream beside them: its own schedule"""
    def streams():
        return [small_stream((480,) * 4, first=1 + 4 * (i % 7)) for i in range(64)]
    items = streams()
    launches, _got = run_case(width, items, follow_up=False)
    assert launches == 1
    assert all(it.gathered == 1 and it.kernel == KERNEL_GENERAL for it in items)
    items = streams() + [Item(plain(2, 380, flags=BH | INTERP | STRICT), None, 2, [480] * 4, drifting(4))]
    launches, _got = run_case(width, items, follow_up=False)
    assert launches == 2


@pytest.mark.parametrize("width", WIDTHS)
def test_refusals_move_nothing(width):
    import torch
    import audio_resampler_amd as A
    B = A.binding(width)
    L = B.lib()
    items = [small_stream(), small_stream(first=5)]
    for i, it in enumerate(items):
        it.build(B, width, 60 + i)
    torch.cuda.synchronize()
    before, errors = [it.batch.state() for it in items], L.artamdErrorCount()

    def call(ctxs, n_ins):
        its = [items[0], items[1], items[0]][:len(ctxs)]
        return B.process_schedule_batch_device(ctxs, [it.x_item for it in its], n_ins, [it.out_item for it in its],
                                               [it.caps for it in its], [it.ratios for it in its])
    with pytest.raises(RuntimeError):                      # a context listed twice
        call([items[0].batch, items[1].batch, items[0].batch], [it.n_ins for it in (items[0], items[1], items[0])])
    with pytest.raises(RuntimeError):                      # a negative frame count
        call([items[0].batch, items[1].batch], [items[0].n_ins, [480, -1, 480]])
    assert [it.batch.state() for it in items] == before and L.artamdErrorCount() == errors
    torch.cuda.synchronize()
    assert all(float(it.out_item.abs().max()) == 0.0 for it in items)
    # ... and the same contexts then make the call as if nothing had happened
    launches, got = call([items[0].batch, items[1].batch], [it.n_ins for it in items])
    for i, (it, (made, res)) in enumerate(zip(items, got)):
        it.check(made, res, f"item {i}")
    assert launches == 1


CHILD = r'''
import sys, json, hashlib, math
sys.path.insert(0, %(root)r)
import numpy as np, torch
import audio_resampler_amd as A
L = A.lib()
R = 48000 / 44100
N, K, STEP = 3, 8, 4
ratios = [[R * (1 + 100e-6 * math.sin(2 * math.pi * (i + 3 * s) / 64)) for i in range(1, K + 1)] for s in range(N)]
n_ins = [[480 + 16 * s] * K for s in range(N)]
caps = [[int(n * r) + 64 for n, r in zip(n_ins[s], ratios[s])] for s in range(N)]
rng = np.random.default_rng(5)
xs = [torch.from_numpy((rng.standard_normal((sum(n_ins[s]), 2)) * 0.25).astype(np.float32)).cuda() for s in range(N)]
rs = [A.Resampler(2, 380, 380, 0.0, A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE) for s in range(N)]
for r in rs:
    r.advance(190)
outs = [torch.zeros((sum(caps[s]), 2), device="cuda") for s in range(N)]
torch.cuda.synchronize()
log, k, pos, out_pos = [], 0, [0] * N, [0] * N
while k < K:
    before = [r.state() for r in rs]
    try:
        launches, got = A.process_schedule_batch_device(rs, [xs[s][pos[s]:] for s in range(N)], [n_ins[s][k:k + STEP] for s in range(N)],
                                                        [outs[s][out_pos[s]:] for s in range(N)], [caps[s][k:k + STEP] for s in range(N)],
                                                        [ratios[s][k:k + STEP] for s in range(N)])
    except RuntimeError:
        assert [r.state() for r in rs] == before, (before, [r.state() for r in rs])
        log.append(("failed", k, L.artamdErrorCount()))
        continue
    assert launches == 1 and all(made == STEP for made, _r in got), (launches, got)
    for s, (made, res) in enumerate(got):
        for u, g in res:
            pos[s] += u; out_pos[s] += g
    k += STEP
torch.cuda.synchronize()
h = hashlib.sha256()
for s in range(N):
    h.update(outs[s][:out_pos[s]].cpu().numpy().tobytes())
print(json.dumps({"sha256": h.hexdigest(), "frames": sum(out_pos), "errors": L.artamdErrorCount(), "log": log}))
'''


def _child(fail_at):
    env = dict(os.environ)
    env.pop("ARTAMD_TEST_FAIL_FIR", None)
    if fail_at:
        env["ARTAMD_TEST_FAIL_FIR"] = str(fail_at)
    p = subprocess.run([sys.executable, "-c", CHILD % dict(root=os.path.dirname(HERE))], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_a_failed_shared_launch_moves_nothing_and_is_counted():
    """ARTAMD_TEST_FAIL_FIR=k refuses the k-th FIR launch of the process on the host, before anything is enqueued: here the first and
    the second shared launch.  Every stream stands where it stood, the failure is counted once, and the retry ends with the clean run's samples"""
    clean, _ = _child(0)
    assert clean["errors"] == 0 and clean["log"] == []
    for fail_at in (1, 2):
        got, err = _child(fail_at)
        assert got["errors"] == 1 and got["log"] == [["failed", 4 * (fail_at - 1), 1]], got
        assert "schedule batch launch failed" in err
        assert got["frames"] == clean["frames"] and got["sha256"] == clean["sha256"], (fail_at, got, clean)
