"""GPU: resampleAdjointScheduleClipsPlanarDevice, resampleProcessScheduleClipsPlanarDevice and ClipWarper.  The yardstick is the CPU oracle
alone (tests/_warp_ref.py: the dense operator A of a clip made block by block, one unit impulse per input frame through the strict oracle),
never the library's own forward.

1. every tap of every row: a batch of unit-impulse gradients on ONE context gives the rows of A — exactly zero where A is zero, within one
   unit in the last place elsewhere (the weight is the same expression in both; the ulp is for a last-bit difference in frac);
2. accumulated sums against A^T gy in float64, per frame within (K_j + 4) 2^-24 (|A|^T |gy|)_j: K_j fused multiply-adds, two roundings of
   the weight, one of the result (derived, not measured: tests/test_gpu_clip_adjoint.py's bound);
3. one block: resampleAdjointClipsPlanarDevice's bits;
4. bit-for-bit invariance: batch or alone, planar or interleaved, odd pitches and bases (and nothing written outside), a cut
   numOutputFrames, channel groups;
5. the contexts are only read; 6. refusals; 7. the forward clips entry; 8. ClipWarper and its autograd."""
import numpy as np
import pytest

import audio_resampler_amd as A
import _warp_ref as W

pytestmark = pytest.mark.gpu
BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
SENTINEL = -777.25
# the clips of the sums, the invariance tests and ClipWarper: block 128, one ratio per block
LENGTHS, BLOCK, RATIOS, LOWPASS = [700, 1, 0, 350], 128, [1.0884, 0.75, 1.3333, 0.5, 2.0, 0.97], 0.5
OUTPUTS = [969, 208, 207, 614]


def np_of(width):
    return np.float64 if width == 64 else np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cut(lengths=LENGTHS):
    """[(frames of every block), ...], [(their ratios), ...]"""
    pairs = [W.clip_blocks(n, BLOCK, RATIOS) for n in lengths]
    return [p[0] for p in pairs], [p[1] for p in pairs]


def buffers(gys, n_ins, planar, gy_pad, gx_pad, base, width):
    """item i's gradient buffer — gys [i] is numpy [C, frames_i] — planar with pitch frames_i + gy_pad, or (planar False) interleaved; its
    result buffer likewise with n_ins [i] + gx_pad, both `base` samples into their allocations, the result's filled with a sentinel"""
    import torch
    dt = torch.float64 if width == 64 else torch.float32
    size = 8 if width == 64 else 4
    keep, gy_ptr, gx_ptr, gy_pitch, gx_pitch = [], [], [], [], []
    for g, nin in zip(gys, n_ins):
        Cn, fr = g.shape
        if planar:
            po, pi = fr + gy_pad, nin + gx_pad
            host = np.zeros((Cn, po), np_of(width)); host[:, :fr] = g
        else:
            po, pi = 0, 0
            host = np.ascontiguousarray(g.T)
        t = torch.zeros(base + host.size + 1, dtype=dt, device="cuda")
        t[base:base + host.size] = torch.from_numpy(host.reshape(-1)).cuda()
        x = torch.full((base + max(Cn * (pi if planar else nin), 1) + 5,), SENTINEL, dtype=dt, device="cuda")
        keep.append((t, x))
        gy_ptr.append(t.data_ptr() + base * size); gx_ptr.append(x.data_ptr() + base * size)
        gy_pitch.append(po if Cn > 1 else 0); gx_pitch.append(pi if Cn > 1 else 0)
    return keep, gy_ptr, gy_pitch, gx_ptr, gx_pitch


def results(keep, gys, n_ins, planar, gx_pad, base):
    """[gx_i [C, n_ins_i]]; the sentinel must have survived everywhere but in frames [0, n_ins [i]) of the planes"""
    out = []
    for g, nin, (_, x) in zip(gys, n_ins, keep):
        Cn = g.shape[0]
        h = x.cpu().numpy()
        body = h[base:base + Cn * ((nin + gx_pad) if planar else nin)]
        grid = body.reshape(Cn, nin + gx_pad) if planar else body.reshape(nin, Cn).T
        got = grid[:, :nin].copy()
        grid[:, :nin] = SENTINEL
        assert np.all(h == SENTINEL), "written outside frames [0, N_i) of the planes"
        out.append(got)
    return out


def adjoint(B, ctxs, gys, blocks, ratios, n_outs=None, planar=True, gy_pad=0, gx_pad=0, base=0, width=32):
    """one call of the blocks adjoint -> (launches, [gx_i [C, N_i]])"""
    import torch
    n_ins = [int(sum(b)) for b in blocks]
    n_outs = [g.shape[1] for g in gys] if n_outs is None else n_outs
    keep, gy_ptr, gy_pitch, gx_ptr, gx_pitch = buffers(gys, n_ins, planar, gy_pad, gx_pad, base, width)
    launches = B.adjoint_schedule_clips_planar_device(ctxs, gy_ptr, gy_pitch, n_outs, gx_ptr, gx_pitch, blocks, ratios)
    torch.cuda.synchronize()
    return launches, results(keep, gys, n_ins, planar, gx_pad, base)


def adjoint_two_phase(ctxs, gys, n_ins, ratios):
    """the same through resampleAdjointClipsPlanarDevice (one process call and the flush)"""
    import torch
    keep, gy_ptr, gy_pitch, gx_ptr, gx_pitch = buffers(gys, n_ins, True, 0, 0, 0, 32)
    launches = A.adjoint_clips_planar_device(ctxs, gy_ptr, gy_pitch, [g.shape[1] for g in gys], gx_ptr, gx_pitch, n_ins, ratios)
    torch.cuda.synchronize()
    return launches, results(keep, gys, n_ins, True, 0, 0)


# ---- 1. every tap of every row ------------------------------------------------------------------------------------------------
ROWS = [
    # an empty block, a one-output block, two tiles of input frames, a block across the tile boundary
    ("interpolating", 32, 16, 16, BH | IN | LP, (40, 0, 3, 33, 24, 300), (1.0884, 0.9, 0.25, 1.3, 0.75, 1.01), (416, 400), (44, 0, 1, 42, 18, 311)),
    ("8-byte", 64, 16, 16, BH | IN | LP, (40, 0, 3, 33, 24, 300), (1.0884, 0.9, 0.25, 1.3, 0.75, 1.01), (416, 400), (44, 0, 1, 42, 18, 311)),
    ("nearest-filter", 32, 32, 8, BH | LP, (30, 40), (1.5, 2 / 3), (83, 70), None),
    ("pass-through", 32, 32, 8, BH, (30, 40), (1.5, 2 / 3), (83, 70), None),
    # more phases on a tile than one group of the kernel's phase table holds
    ("100-blocks", 32, 16, 16, BH | IN | LP, (4,) * 100, (0.8, 1.25) * 50, (410, 400), None),
    # blocks without outputs
    ("one-frame-blocks", 32, 16, 16, BH | IN | LP, (1,) * 60, (0.5, 2.0, 1.0) * 20, (48, 60), None),
]


@pytest.mark.parametrize("name,width,taps,filters,flags,blocks,ratios,shape,per_block", ROWS, ids=[r[0] for r in ROWS])
def test_unit_impulses_give_the_rows_of_the_oracles_operator(name, width, taps, filters, flags, blocks, ratios, shape, per_block):
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    dense, made = W.dense_operator(taps, filters, flags, blocks, ratios, width=width)
    assert dense.shape == shape and (per_block is None or made == per_block)
    if name == "one-frame-blocks":
        assert sum(1 for m in made if m == 0) == 20
    M, frames = dense.shape
    ctx = B.Resampler(1, taps, filters, 0.0, flags)
    dt = torch.float64 if width == 64 else torch.float32
    gy = torch.eye(M, dtype=dt, device="cuda")
    gx = torch.full((M, frames), SENTINEL, dtype=dt, device="cuda")
    size = gy.element_size()
    launches = B.adjoint_schedule_clips_planar_device([ctx] * M, [gy.data_ptr() + n * M * size for n in range(M)], None, [M] * M,
                                                      [gx.data_ptr() + n * frames * size for n in range(M)], None, [list(blocks)] * M, [list(ratios)] * M)
    torch.cuda.synchronize()
    assert launches == 1
    got = gx.cpu().numpy().astype(np.float64)
    zero = dense == 0
    print(name, "outputs", M, "non-zero entries", int((~zero).sum()), "entries off by an ulp", int((got != dense).sum()))
    assert np.all(got[zero] == 0), "a weight where the operator has none"
    assert np.all(np.abs(got - dense) <= np.where(zero, 0.0, W.ulp_of(dense, width))), np.abs(got - dense).max()
    if name == "pass-through":                                    # (the copied sample: a row with a single 1)
        assert any(np.count_nonzero(row) == 1 and row.max() == 1.0 for row in dense)
    ctx.close()


# ---- 2. accumulated sums -------------------------------------------------------------------------------------------------------
def operators():
    blocks, ratios = cut()
    dense = [W.dense_operator(380, 380, BH | IN | LP, b, r, LOWPASS)[0] for b, r in zip(blocks, ratios)]
    assert [d.shape for d in dense] == list(zip(OUTPUTS, LENGTHS))
    return blocks, ratios, dense


def noise_gradients(counts, channels, seed):
    rng = np.random.default_rng(seed)
    return [(0.25 * rng.standard_normal((channels, m))).astype(np.float32) for m in counts]


def check_sums(got, dense, gy, where):
    for c in range(gy.shape[0]):
        want, scale, K = W.expected_gradient(dense, gy[c])
        bound = (K + 4) * 2.0 ** -24 * scale
        err = np.abs(got[c].astype(np.float64) - want)
        if len(err):
            print(where, "channel", c, "K up to", int(K.max()), "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (where, c, float(err.max()))


def test_sums_match_the_transposed_oracle_operator():
    pytest.importorskip("torch")
    blocks, ratios, dense = operators()
    gys = noise_gradients(OUTPUTS, 2, 21)
    ctx = A.Resampler(2, 380, 380, LOWPASS, BH | IN | LP)
    launches, got = adjoint(A, [ctx] * len(LENGTHS), gys, blocks, ratios)
    assert launches == 1
    for i, n in enumerate(LENGTHS):
        assert got[i].shape == (2, n)
        check_sums(got[i], dense[i], gys[i], ("clip", i, "frames", n))
    ctx.close()


# ---- 3. one block is the two-phase entry ---------------------------------------------------------------------------------------------
ONE_BLOCK = [
    ("44100-16000", 380, 380, BH | IN | LP, (44100.0, 16000.0, 0), None),
    ("16000-44100", 380, 380, BH | IN | LP, (16000.0, 44100.0, 0), None),
    ("any-ratio-1.1", 380, 380, BH | IN | LP, None, 1.1),
    # the kernels' other branch: a single row per output, and the pass-through's copied sample
    ("nearest-filter", 32, 8, BH | LP, (3.0, 2.0, 0), None),
    ("pass-through", 32, 8, BH, (2.0, 3.0, 0), None),
]


@pytest.mark.parametrize("name,taps,filters,flags,fixed,ratio", ONE_BLOCK, ids=[c[0] for c in ONE_BLOCK])
def test_one_block_gives_the_two_phase_entrys_bits(name, taps, filters, flags, fixed, ratio):
    pytest.importorskip("torch")
    lengths = [700, 1, 257, 189]
    ctx = A.Resampler(2, taps, filters, 0.0, flags, fixed)
    r = ratio if ratio is not None else 1.0                       # (a fixed-ratio context ignores it)
    Ms = [W.output_count(taps, filters, flags, (n,), (r,), fixed=fixed) for n in lengths]
    gys = noise_gradients(Ms, 2, 33)
    launches, got = adjoint(A, [ctx] * len(lengths), gys, [[n] for n in lengths], [[r]] * len(lengths))
    launches2, want = adjoint_two_phase([ctx] * len(lengths), gys, lengths, [r] * len(lengths))
    assert launches == launches2 == 1
    for i in range(len(lengths)):
        assert np.any(want[i] != 0) and np.array_equal(bits(got[i]), bits(want[i])), i
    ctx.close()


# ---- 4. invariance, bit for bit ------------------------------------------------------------------------------------------------
def test_batch_layout_pitch_and_cut_do_not_change_a_bit():
    pytest.importorskip("torch")
    blocks, ratios = cut()
    n = len(LENGTHS)
    ctx = A.Resampler(2, 380, 380, LOWPASS, BH | IN | LP)
    gys = noise_gradients(OUTPUTS, 2, 31)
    _, batch = adjoint(A, [ctx] * n, gys, blocks, ratios)
    assert all(np.any(batch[i] != 0) for i in range(n) if LENGTHS[i])
    for i in range(n):                                            # each clip alone (an empty clip: no launch)
        launches, alone = adjoint(A, [ctx], [gys[i]], [blocks[i]], [ratios[i]])
        assert launches == (1 if LENGTHS[i] else 0) and np.array_equal(bits(alone[0]), bits(batch[i])), i
    order = [3, 0, 2, 1]                                          # ... and at another place in the batch
    _, moved = adjoint(A, [ctx] * n, [gys[i] for i in order], [blocks[i] for i in order], [ratios[i] for i in order])
    _, inter = adjoint(A, [ctx] * n, gys, blocks, ratios, planar=False)
    _, odd = adjoint(A, [ctx] * n, gys, blocks, ratios, gy_pad=3, gx_pad=5, base=1)
    for i in range(n):
        assert np.array_equal(bits(moved[order.index(i)]), bits(batch[i])), ("place", i)
        assert np.array_equal(bits(inter[i]), bits(batch[i])), ("interleaved", i)
        assert np.array_equal(bits(odd[i]), bits(batch[i])), ("odd pitch and base", i)
    # numOutputFrames cut to half = the full call on a gradient zeroed past the cut
    short_counts = [m // 2 for m in OUTPUTS]
    zeroed = [g.copy() for g in gys]
    for g, c in zip(zeroed, short_counts):
        g[:, c:] = 0
    _, short = adjoint(A, [ctx] * n, gys, blocks, ratios, n_outs=short_counts)
    _, full = adjoint(A, [ctx] * n, zeroed, blocks, ratios)
    for i in range(n):
        assert np.array_equal(bits(short[i]), bits(full[i])), ("cut", i)
    ctx.close()


@pytest.mark.parametrize("channels", [3, 9])
@pytest.mark.parametrize("flags", [BH | IN | LP, BH | LP], ids=["interpolating", "nearest-filter"])
def test_channel_groups_equal_the_one_channel_result_per_plane(channels, flags):
    """3 channels: a partial group of 4; 9: a full group of 8 and a second, partial one.  600 frames: three tiles of input frames"""
    pytest.importorskip("torch")
    blocks, ratios = (200, 0, 150, 250), (0.9, 1.0, 1.5, 2 / 3)
    one = A.Resampler(1, 16, 16, 0.0, flags)
    many = A.Resampler(channels, 16, 16, 0.0, flags)
    M = W.output_count(16, 16, flags, blocks, ratios)
    gy = (0.25 * np.random.default_rng(32).standard_normal((channels, M))).astype(np.float32)
    _, planes = adjoint(A, [one] * channels, [gy[c:c + 1] for c in range(channels)], [blocks] * channels, [ratios] * channels)
    for planar in (True, False):
        launches, got = adjoint(A, [many], [gy], [blocks], [ratios], planar=planar, gy_pad=1, gx_pad=2)
        assert launches == 1
        for c in range(channels):
            assert np.any(got[0][c] != 0) and np.array_equal(bits(got[0][c]), bits(planes[c][0])), (planar, c)
    one.close(); many.close()


# ---- 5. contexts untouched ----------------------------------------------------------------------------------------------------
def test_a_context_in_mid_stream_is_only_read_and_serves_a_batch():
    torch = pytest.importorskip("torch")
    x = torch.from_numpy((0.25 * np.random.default_rng(41).standard_normal((2000, 2))).astype(np.float32)).cuda()
    pair = [A.Resampler(2, 64, 64, 0.0, BH | IN) for _ in range(2)]
    outs = [torch.zeros(4096, 2, device="cuda") for _ in range(2)]
    for r, y in zip(pair, outs):
        assert r.process_device(x, 1000, y, 2048, 1.1)[0] == 1000
    before = (pair[0].state(), pair[0].position(), pair[0].last_kernel(), pair[0].last_gathered())
    assert before == (pair[1].state(), pair[1].position(), pair[1].last_kernel(), pair[1].last_gathered())
    blocks, ratios = [(200, 100), (), (40,)], [(1.1, 0.9), (), (0.9,)]
    gy = (0.25 * np.random.default_rng(42).standard_normal((2, 100))).astype(np.float32)
    launches, got = adjoint(A, [pair[0]] * 3, [gy] * 3, blocks, ratios, n_outs=[100, 0, 50])
    assert launches == 1 and np.any(got[0] != 0) and np.any(got[2] != 0)
    # ... and what a fresh context of the same parameters gives
    fresh = A.Resampler(2, 64, 64, 0.0, BH | IN)
    _, same = adjoint(A, [fresh] * 3, [gy] * 3, blocks, ratios, n_outs=[100, 0, 50])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, same))
    assert before == (pair[0].state(), pair[0].position(), pair[0].last_kernel(), pair[0].last_gathered())
    nexts = []
    for r, y in zip(pair, outs):
        y.zero_()
        nexts.append(r.process_device(x[1000:], 1000, y, 2048, 1.1))
    torch.cuda.synchronize()
    assert nexts[0] == nexts[1] and torch.equal(outs[0], outs[1])
    assert pair[0].state() == pair[1].state() and pair[0].last_kernel() == pair[1].last_kernel() and pair[0].last_gathered() == pair[1].last_gathered()
    for r in pair + [fresh]:
        r.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_and_count_nothing():
    torch = pytest.importorskip("torch")
    errors = A.lib().artamdErrorCount()
    flags = BH | IN | LP
    plain = A.Resampler(1, 16, 16, 0.0, flags)
    ends = A.Resampler(1, 16, 16, 0.0, flags | A.EXTRAPOLATE_ENDPOINTS)
    blocks, ratios = [60, 37], [1.25, 0.8]
    M = W.output_count(16, 16, flags, tuple(blocks), tuple(ratios))
    gy = torch.ones(M + 8, device="cuda")
    gx = torch.full((97,), SENTINEL, device="cuda")
    call = A.adjoint_schedule_clips_planar_device
    for ctxs, n_out in (([ends], M), ([plain, ends], M), ([plain], M + 1)):
        k = len(ctxs)
        with pytest.raises(RuntimeError):
            call(ctxs, [gy] * k, None, [n_out] * k, [gx] * k, None, [blocks] * k, [ratios] * k)
    for bad_blocks, bad_ratios, n_out in (([60, -1], ratios, M), (blocks, [1.25, 0.0], M), (blocks, [-1.0, 0.8], M), (blocks, ratios, -1),
                                          ([2 ** 30, 2 ** 30], ratios, M)):
        with pytest.raises(RuntimeError):
            call([plain], [gy], None, [n_out], [gx], None, [bad_blocks], [bad_ratios])
    with pytest.raises(RuntimeError):                             # (a NULL buffer of a clip with frames)
        call([plain], [None], None, [M], [gx], None, [blocks], [ratios])
    torch.cuda.synchronize()
    assert bool((gx == SENTINEL).all()) and A.lib().artamdErrorCount() == errors
    assert call([plain], [gy], None, [M], [gx], None, [blocks], [ratios]) == 1      # (and M itself is taken)
    assert call([plain, plain, plain], [gy] * 3, None, [0, 0, 0], [gx] * 3, None, [[0, 0], [], [0]], [[1.0, 1.0], [], [1.0]]) == 0
    torch.cuda.synchronize()
    assert bool((gx != SENTINEL).all())
    plain.close(); ends.close()


# ---- 7. the forward clips entry ------------------------------------------------------------------------------------------------------
STREAMS = [([200, 0, 100, 37], [1.1, 0.9, 0.5, 1.7]), ([50], [0.75]), ([0], [1.3]), ([128, 128, 44], [0.97, 1.02, 1.01])]


def schedule(entry, ctxs, x, idx, **more):
    """the schedules of STREAMS [i], i in idx, on ctxs [i] and x [i] through `entry`, planar buffers -> (launches, per stream (blocks made,
    results), outputs [len (idx), 2, room]); the last stream is not flushed"""
    import torch
    streams = [STREAMS[i] for i in idx]
    caps = [[int((f + 34) * r) + 8 for f, r in zip(*s)] for s in streams]
    room = max(sum(c) for c in caps)
    y = torch.zeros(len(idx), 2, room, device="cuda")
    launches, got = entry([ctxs[i] for i in idx], [x[i] for i in idx], [x.stride(1)] * len(idx), [s[0] for s in streams], [y[k] for k in range(len(idx))],
                          [room] * len(idx), caps, [s[1] for s in streams], flush_last=[i != len(STREAMS) - 1 for i in idx], **more)
    torch.cuda.synchronize()
    return launches, got, y


def dirty(ctxs, x):
    import torch
    scratch = torch.zeros(2, 2048, device="cuda")
    for i, r in enumerate(ctxs):
        r.process_planar_device(x[i], x.stride(1), 300 + 7 * i, scratch, 2048, 2048, 1.05)
    torch.cuda.synchronize()


def test_forward_clips_entry_is_reset_plus_the_schedule_batch_entry():
    torch = pytest.importorskip("torch")
    n = len(STREAMS)
    x = torch.from_numpy((0.25 * np.random.default_rng(71).standard_normal((n, 2, 400))).astype(np.float32)).cuda()
    make = lambda: [A.Resampler(2, 64, 64, 0.0, BH | IN) for _ in range(n)]
    observe = lambda ctxs: [(r.state(), r.position(), r.last_kernel(), r.last_gathered()) for r in ctxs]
    new, old = make(), make()
    dirty(new, x); dirty(old, x)
    assert observe(new) == observe(old)
    for r in old:
        r.reset()
    launches_old, got_old, y_old = schedule(A.process_schedule_batch_planar_device, old, x, range(n))
    launches_new, got_new, y_new = schedule(A.process_schedule_clips_planar_device, new, x, range(n), from_start=True)
    assert got_new == got_old and torch.equal(y_new, y_old) and observe(new) == observe(old)
    assert all(made == len(s[0]) for (made, _), s in zip(got_new, STREAMS)) and bool(y_new.abs().sum() > 0)
    assert launches_new == launches_old + 1                       # (the zeroing launch)
    # from_start=False is the schedule batch entry itself: the streams go on where they stand (the last in mid-stream, the first flushed)
    launches_old, got_old, y_old = schedule(A.process_schedule_batch_planar_device, old, x, [3, 0])
    launches_new, got_new, y_new = schedule(A.process_schedule_clips_planar_device, new, x, [3, 0], from_start=False)
    assert got_new == got_old and torch.equal(y_new, y_old) and observe(new) == observe(old) and launches_new == launches_old
    for r in new + old:
        r.close()


# ---- 8. ClipWarper ------------------------------------------------------------------------------------------------------------------
def warp_input(seed=81):
    import torch
    return torch.from_numpy((0.25 * np.random.default_rng(seed).standard_normal((len(LENGTHS), 2, max(LENGTHS)))).astype(np.float32)).cuda()


def test_clip_warper_is_the_clips_entry_on_fresh_contexts():
    torch = pytest.importorskip("torch")
    blocks, ratios, dense = operators()
    n = len(LENGTHS)
    x = warp_input()
    warper = A.ClipWarper(2, lowpass_ratio=LOWPASS, block=BLOCK)
    y, out_lengths = warper(x, [RATIOS] * n, LENGTHS)
    assert y.grad_fn is None and out_lengths.tolist() == OUTPUTS == [d.shape[0] for d in dense] and y.shape == (n, 2, max(OUTPUTS))
    # the route before it: a reset per context, then the schedule batch entry
    ctxs = [A.Resampler(2, 380, 380, LOWPASS, BH | IN | LP) for _ in range(n)]
    caps = [[int((f + 192) * r) + 8 for f, r in zip(b, q)] for b, q in zip(blocks, ratios)]
    want = torch.zeros(n, 2, max(sum(c) for c in caps), device="cuda")
    for r in ctxs:
        r.reset()
    _, got = A.process_schedule_batch_planar_device(ctxs, [x[i] for i in range(n)], [x.stride(1)] * n, [list(b) for b in blocks], [want[i] for i in range(n)],
                                                    [want.stride(1)] * n, caps, [list(q) for q in ratios], flush_last=[True] * n)
    torch.cuda.synchronize()
    for i in range(n):
        assert got[i][0] == len(blocks[i]) and sum(g for _, g in got[i][1]) == OUTPUTS[i]
        assert torch.equal(y[i, :, :OUTPUTS[i]], want[i, :, :OUTPUTS[i]]) and bool((y[i, :, OUTPUTS[i]:] == 0).all()), i
    assert bool(y.abs().sum() > 0)
    # the same call twice (the pool is started afresh), with a scalar and a ratio per clip, and a [C, T] clip alone
    again, _ = warper(x, np.array([RATIOS] * n), torch.tensor(LENGTHS))
    assert torch.equal(again, y)
    flat, flat_lengths = warper(x, 1.0884, LENGTHS)
    per_clip, per_clip_lengths = warper(x, torch.full((n,), 1.0884, dtype=torch.float64), LENGTHS)
    assert torch.equal(flat, per_clip) and torch.equal(flat_lengths, per_clip_lengths)
    single, single_lengths = warper(x[3, :, :350], torch.tensor([RATIOS], dtype=torch.float64).cuda())
    assert single_lengths.tolist() == [OUTPUTS[3]] and torch.equal(single[0], y[3, :, :OUTPUTS[3]])
    for r in ctxs:
        r.close()
    warper.close()


def test_clip_warper_autograd_gradient_matches_the_oracle():
    torch = pytest.importorskip("torch")
    _, _, dense = operators()
    n = len(LENGTHS)
    warper = A.ClipWarper(2, lowpass_ratio=LOWPASS, block=BLOCK)
    rng = np.random.default_rng(61)
    x = warp_input().requires_grad_()
    y, out_lengths = warper(x, [RATIOS] * n, LENGTHS)
    assert y.requires_grad and y.grad_fn is not None and not out_lengths.requires_grad
    g = (0.25 * rng.standard_normal(tuple(y.shape))).astype(np.float32)
    (y * torch.from_numpy(g).cuda()).sum().backward()
    torch.cuda.synchronize()
    grad = x.grad.cpu().numpy()
    assert grad.shape == (n, 2, max(LENGTHS))
    for i, frames in enumerate(LENGTHS):
        check_sums(grad[i][:, :frames], dense[i], g[i][:, :OUTPUTS[i]], ("autograd clip", i))
        assert np.all(grad[i][:, frames:] == 0), i
    # the call without grad is the forward alone, and gives the attached call's samples
    plain, _ = warper(x.detach(), [RATIOS] * n, LENGTHS)
    with torch.no_grad():
        quiet, _ = warper(x, [RATIOS] * n, LENGTHS)
    assert plain.grad_fn is None and quiet.grad_fn is None and not quiet.requires_grad
    assert torch.equal(plain, y.detach()) and torch.equal(quiet, plain)
    with pytest.raises(RuntimeError):                             # (once differentiable)
        x2 = x.detach().clone().requires_grad_()
        y2, _ = warper(x2, [RATIOS] * n, LENGTHS)
        (gx2,) = torch.autograd.grad(y2.sum(), x2, create_graph=True)
        gx2.sum().backward()
    with pytest.raises(ValueError):                               # (the ratio curve has no gradient)
        warper(x, torch.tensor([RATIOS] * n, requires_grad=True), LENGTHS)
    # no clip at all: nothing to make, and a gradient of that shape (no context is ever needed)
    empty = A.ClipWarper(2, block=BLOCK)
    x0 = torch.zeros(0, 2, 10, device="cuda", requires_grad=True)
    y0, lengths0 = empty(x0, 1.0)
    y0.sum().backward()
    assert y0.shape[:2] == (0, 2) and lengths0.tolist() == [] and x0.grad.shape == (0, 2, 10) and empty.pool == []
    # backward after close () raises
    y3, _ = warper(x.detach().clone().requires_grad_(), [RATIOS] * n, LENGTHS)
    warper.close()
    with pytest.raises(RuntimeError):
        y3.sum().backward()


def test_clip_warper_gradcheck_on_the_8_byte_build():
    torch = pytest.importorskip("torch")
    B = A.binding(64)
    warper = B.ClipWarper(2, taps=16, filters=16, block=16)
    x = torch.from_numpy(0.25 * np.random.default_rng(81).standard_normal((2, 2, 24))).cuda().requires_grad_()
    ratios = [[1.1, 0.8], [0.7, 1.25]]
    assert warper(x, ratios, [24, 17])[1].tolist() == [W.output_count(16, 16, BH | IN | LP, *W.clip_blocks(n, 16, r)) for n, r in zip([24, 17], ratios)]
    assert torch.autograd.gradcheck(lambda t: warper(t, ratios, [24, 17])[0], (x,), eps=1e-6, atol=1e-7, rtol=1e-6)
    warper.close()
