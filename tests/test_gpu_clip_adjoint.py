"""GPU: resampleAdjointClipsPlanarDevice and ClipResampler's autograd.  The yardstick is the CPU oracle alone (tests/_adjoint_ref.py: the
dense operator A of a whole clip, one unit impulse per input frame through the strict oracle), never the library's own forward.

1. every tap of every row: a batch of unit-impulse gradients on ONE context gives the rows of A — exactly zero where A is zero, within one
   unit in the last place elsewhere (the weight is the same expression in both; the ulp is for a last-bit difference in frac);
2. accumulated sums against A^T gy in float64, per frame within (K_j + 4) 2^-24 (|A|^T |gy|)_j: K_j fused multiply-adds, two roundings of
   the weight, one of the result (derived, not measured);
3. bit-for-bit invariance: batch or alone, planar or interleaved, odd pitches and bases (and nothing written outside), channel groups,
   a cut numOutputFrames;
4. the contexts are only read; 5. refusals; 6.-8. autograd through ClipResampler."""
import numpy as np
import pytest

import audio_resampler_amd as A
import _adjoint_ref as R

pytestmark = pytest.mark.gpu
BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
DOWN, UP = (44100.0, 16000.0, 0), (16000.0, 44100.0, 0)
LENGTHS = [700, 1, 699, 0, 350, 189, 190, 191]
SENTINEL = -777.25


def np_of(width):
    return np.float64 if width == 64 else np.float32


def adjoint(B, ctxs, gys, n_ins, n_outs=None, ratios=None, planar=True, gy_pad=0, gx_pad=0, base=0, width=32):
    """One adjoint call.  gys [i]: numpy [C, frames_i] (channels first); item i's gradient buffer is planar with pitch frames_i + gy_pad, or
    (planar False) interleaved; its result buffer likewise with n_ins [i] + gx_pad, both `base` samples into their allocations, the result's
    filled with a sentinel that must survive everywhere but in frames [0, n_ins [i]) of the planes.  Returns (launches, [gx_i [C, n_ins_i]])."""
    import torch
    dt = torch.float64 if width == 64 else torch.float32
    size = 8 if width == 64 else 4
    n_outs = [g.shape[1] for g in gys] if n_outs is None else n_outs
    ratios = [1.0] * len(ctxs) if ratios is None else ratios
    d_gy, d_gx, gy_ptr, gx_ptr, gy_pitch, gx_pitch = [], [], [], [], [], []
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
        d_gy.append(t); d_gx.append(x)
        gy_ptr.append(t.data_ptr() + base * size); gx_ptr.append(x.data_ptr() + base * size)
        gy_pitch.append(po if Cn > 1 else 0); gx_pitch.append(pi if Cn > 1 else 0)
    launches = B.adjoint_clips_planar_device(ctxs, gy_ptr, gy_pitch, n_outs, gx_ptr, gx_pitch, n_ins, ratios)
    torch.cuda.synchronize()
    out = []
    for g, nin, x in zip(gys, n_ins, d_gx):
        Cn = g.shape[0]
        h = x.cpu().numpy()
        body = h[base:base + Cn * ((nin + gx_pad) if planar else nin)]
        grid = body.reshape(Cn, nin + gx_pad) if planar else body.reshape(nin, Cn).T
        got = grid[:, :nin].copy()
        grid[:, :nin] = SENTINEL
        assert np.all(h == SENTINEL), "written outside frames [0, numInputFrames) of the planes"
        out.append(got)
    return launches, out


# ---- 1. every tap of every row ------------------------------------------------------------------------------------------------
ROWS = [
    ("interpolating-down", 32, 16, 16, BH | IN | LP, (44100.0, 16000.0, 0), 97, 39),
    ("interpolating-up", 32, 16, 16, BH | IN | LP, (44100.0, 48000.0, 0), 97, 115),
    ("nearest-filter", 32, 32, 8, BH | LP, (3.0, 2.0, 0), 70, None),
    ("pass-through", 32, 32, 8, BH, (2.0, 3.0, 0), 70, None),
    ("8-byte", 64, 16, 16, BH | IN | LP, (44100.0, 16000.0, 0), 97, 39),
]


@pytest.mark.parametrize("name,width,taps,filters,flags,fixed,frames,outputs", ROWS, ids=[r[0] for r in ROWS])
def test_unit_impulses_give_the_rows_of_the_oracles_operator(name, width, taps, filters, flags, fixed, frames, outputs):
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    dense = R.dense_operator(taps, filters, flags, frames, fixed=fixed, width=width)
    M = dense.shape[0]
    assert outputs is None or M == outputs
    ctx = B.Resampler(1, taps, filters, 0.0, flags, fixed)
    dt = torch.float64 if width == 64 else torch.float32
    gy = torch.eye(M, dtype=dt, device="cuda")
    gx = torch.full((M, frames), SENTINEL, dtype=dt, device="cuda")
    size = gy.element_size()
    launches = B.adjoint_clips_planar_device([ctx] * M, [gy.data_ptr() + n * M * size for n in range(M)], None, [M] * M,
                                             [gx.data_ptr() + n * frames * size for n in range(M)], None, [frames] * M, [1.0] * M)
    torch.cuda.synchronize()
    assert launches == 1
    got = gx.cpu().numpy().astype(np.float64)
    zero = dense == 0
    print(name, "outputs", M, "non-zero entries", int((~zero).sum()), "entries off by an ulp", int((got != dense).sum()))
    assert np.all(got[zero] == 0), "a weight where the operator has none"
    assert np.all(np.abs(got - dense) <= np.where(zero, 0.0, R.ulp_of(dense, width))), np.abs(got - dense).max()
    if name == "pass-through":                                    # (the copied sample: a row with a single 1)
        assert any(np.count_nonzero(row) == 1 and row.max() == 1.0 for row in dense)
    ctx.close()


# ---- 2. accumulated sums -------------------------------------------------------------------------------------------------------
def noise_gradients(dense_list, channels, seed):
    rng = np.random.default_rng(seed)
    return [(0.25 * rng.standard_normal((channels, d.shape[0]))).astype(np.float32) for d in dense_list]


def check_sums(got, dense, gy, where):
    for c in range(gy.shape[0]):
        want, scale, K = R.expected_gradient(dense, gy[c])
        bound = (K + 4) * 2.0 ** -24 * scale
        err = np.abs(got[c].astype(np.float64) - want)
        if len(err):
            print(where, "channel", c, "K up to", int(K.max()), "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (where, c, float(err.max()))


@pytest.mark.parametrize("fixed", [DOWN, UP], ids=["44100-16000", "16000-44100"])
def test_sums_match_the_transposed_oracle_operator(fixed):
    pytest.importorskip("torch")
    flags = BH | IN | LP
    dense = [R.dense_operator(380, 380, flags, n, fixed=fixed) for n in LENGTHS]
    gys = noise_gradients(dense, 2, 21)
    ctx = A.Resampler(2, 380, 380, 0.0, flags, fixed)
    launches, got = adjoint(A, [ctx] * len(LENGTHS), gys, LENGTHS)
    assert launches == 1
    for i, n in enumerate(LENGTHS):
        assert got[i].shape == (2, n)
        check_sums(got[i], dense[i], gys[i], (fixed[:2], "clip", i, "frames", n))
    ctx.close()


def test_sums_of_an_any_ratio_context():
    pytest.importorskip("torch")
    lengths = [300, 31]
    dense = [R.dense_operator(64, 64, BH | IN, n, ratio=1.1) for n in lengths]
    gys = noise_gradients(dense, 2, 22)
    ctx = A.Resampler(2, 64, 64, 0.0, BH | IN)
    launches, got = adjoint(A, [ctx] * 2, gys, lengths, ratios=[1.1, 1.1])
    assert launches == 1
    for i in range(2):
        check_sums(got[i], dense[i], gys[i], ("ratio 1.1 clip", i))
    ctx.close()


# ---- 3. invariance, bit for bit ------------------------------------------------------------------------------------------------
def outputs_of(ctx, frames):
    """how many output frames a clip of `frames` frames makes on this fixed-ratio context (only to size the gradients: were it not the
    adjoint's own M, the calls below would be refused or read short)"""
    import torch
    cap = int((frames + ctx.c.numTaps) * ctx.c.fixedRatio) + 64
    x = torch.zeros(ctx.channels, max(frames, 1), device="cuda")
    y = torch.zeros(ctx.channels, cap, device="cuda")
    ctx.reset()
    used, made = ctx.process_and_flush_planar_device(x, max(frames, 1), frames, y, cap, cap, 0.0)
    ctx.reset()
    torch.cuda.synchronize()
    assert used == frames and made < cap
    return made


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("fixed", [DOWN, UP], ids=["44100-16000", "16000-44100"])
def test_batch_layout_pitch_and_cut_do_not_change_a_bit(fixed):
    pytest.importorskip("torch")
    ctx = A.Resampler(2, 380, 380, 0.0, BH | IN | LP, fixed)
    Ms = [outputs_of(ctx, n) for n in LENGTHS]
    rng = np.random.default_rng(31)
    gys = [(0.25 * rng.standard_normal((2, m))).astype(np.float32) for m in Ms]
    _, batch = adjoint(A, [ctx] * len(LENGTHS), gys, LENGTHS)
    for i, n in enumerate(LENGTHS):                               # each clip alone (an empty clip: no launch)
        launches, alone = adjoint(A, [ctx], [gys[i]], [n])
        assert launches == (1 if n else 0) and np.array_equal(bits(alone[0]), bits(batch[i])), i
    _, inter = adjoint(A, [ctx] * len(LENGTHS), gys, LENGTHS, planar=False)
    _, odd = adjoint(A, [ctx] * len(LENGTHS), gys, LENGTHS, gy_pad=3, gx_pad=5, base=1)
    for i in range(len(LENGTHS)):
        assert np.array_equal(bits(inter[i]), bits(batch[i])), ("interleaved", i)
        assert np.array_equal(bits(odd[i]), bits(batch[i])), ("odd pitch and base", i)
    # numOutputFrames cut to half = the full call on a gradient zeroed past the cut
    cut = [m // 2 for m in Ms]
    zeroed = [g.copy() for g in gys]
    for g, c in zip(zeroed, cut):
        g[:, c:] = 0
    _, short = adjoint(A, [ctx] * len(LENGTHS), gys, LENGTHS, n_outs=cut)
    _, full = adjoint(A, [ctx] * len(LENGTHS), zeroed, LENGTHS)
    for i in range(len(LENGTHS)):
        assert np.array_equal(bits(short[i]), bits(full[i])), ("cut", i)
    ctx.close()


@pytest.mark.parametrize("channels", [3, 9])
@pytest.mark.parametrize("fixed,flags", [((44100.0, 16000.0, 0), BH | IN | LP), ((3.0, 2.0, 0), BH | LP)], ids=["interpolating", "nearest-filter"])
def test_channel_groups_equal_the_one_channel_result_per_plane(channels, fixed, flags):
    """3 channels: a partial group of 4; 9: a full group of 8 and a second, partial one.  600 frames: three tiles of input frames"""
    pytest.importorskip("torch")
    frames = 600
    one = A.Resampler(1, 16, 16, 0.0, flags, fixed)
    many = A.Resampler(channels, 16, 16, 0.0, flags, fixed)
    M = outputs_of(one, frames)
    gy = (0.25 * np.random.default_rng(32).standard_normal((channels, M))).astype(np.float32)
    _, planes = adjoint(A, [one] * channels, [gy[c:c + 1] for c in range(channels)], [frames] * channels)
    for planar in (True, False):
        launches, got = adjoint(A, [many], [gy], [frames], planar=planar, gy_pad=1, gx_pad=2)
        assert launches == 1
        for c in range(channels):
            assert np.array_equal(bits(got[0][c]), bits(planes[c][0])), (planar, c)
    one.close(); many.close()


# ---- 4. contexts untouched ----------------------------------------------------------------------------------------------------
def test_a_context_in_mid_stream_is_only_read():
    torch = pytest.importorskip("torch")
    x = torch.from_numpy((0.25 * np.random.default_rng(41).standard_normal((2000, 2))).astype(np.float32)).cuda()
    pair = [A.Resampler(2, 64, 64, 0.0, BH | IN) for _ in range(2)]
    outs = [torch.zeros(4096, 2, device="cuda") for _ in range(2)]
    for r, y in zip(pair, outs):
        assert r.process_device(x, 1000, y, 2048, 1.1)[0] == 1000
    before = (pair[0].state(), pair[0].position(), pair[0].last_kernel(), pair[0].last_gathered())
    assert before == (pair[1].state(), pair[1].position(), pair[1].last_kernel(), pair[1].last_gathered())
    gy = (0.25 * np.random.default_rng(42).standard_normal((2, 100))).astype(np.float32)
    launches, _ = adjoint(A, [pair[0]] * 3, [gy] * 3, [300, 0, 40], n_outs=[100, 0, 50], ratios=[1.1, 1.1, 0.9])
    assert launches == 1
    assert before == (pair[0].state(), pair[0].position(), pair[0].last_kernel(), pair[0].last_gathered())
    nexts = []
    for r, y in zip(pair, outs):
        y.zero_()
        nexts.append(r.process_device(x[1000:], 1000, y, 2048, 1.1))
    torch.cuda.synchronize()
    assert nexts[0] == nexts[1] and torch.equal(outs[0], outs[1])
    assert pair[0].state() == pair[1].state() and pair[0].last_kernel() == pair[1].last_kernel() and pair[0].last_gathered() == pair[1].last_gathered()
    for r in pair:
        r.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_enqueue_and_count_nothing():
    torch = pytest.importorskip("torch")
    errors = A.lib().artamdErrorCount()
    plain = A.Resampler(1, 16, 16, 0.0, BH | IN | LP, (44100.0, 16000.0, 0))
    ends = A.Resampler(1, 16, 16, 0.0, BH | IN | LP | A.EXTRAPOLATE_ENDPOINTS, (44100.0, 16000.0, 0))
    M = R.dense_operator(16, 16, BH | IN | LP, 97, fixed=(44100.0, 16000.0, 0)).shape[0]
    gy = torch.ones(M + 8, device="cuda")
    gx = torch.full((97,), SENTINEL, device="cuda")
    for ctxs, n_out in (([ends], M), ([plain, ends], M), ([plain], M + 1)):
        k = len(ctxs)
        with pytest.raises(RuntimeError):
            A.adjoint_clips_planar_device(ctxs, [gy] * k, None, [n_out] * k, [gx] * k, None, [97] * k, [1.0] * k)
    with pytest.raises(RuntimeError):
        A.adjoint_clips_planar_device([plain], [gy], None, [-1], [gx], None, [97], [1.0])
    torch.cuda.synchronize()
    assert bool((gx == SENTINEL).all()) and A.lib().artamdErrorCount() == errors
    assert A.adjoint_clips_planar_device([plain], [gy], None, [M], [gx], None, [97], [1.0]) == 1      # (and M itself is taken)
    assert A.adjoint_clips_planar_device([plain, plain], [gy] * 2, None, [0, 0], [gx] * 2, None, [0, 0], [1.0] * 2) == 0
    torch.cuda.synchronize()
    assert bool((gx != SENTINEL).all())
    plain.close(); ends.close()


# ---- 6.-8. autograd ---------------------------------------------------------------------------------------------------------------
def test_autograd_gradient_matches_the_oracle():
    torch = pytest.importorskip("torch")
    flags, lengths = BH | IN | LP, [700, 350, 0]
    clips = A.ClipResampler(2, 44100, 16000)
    rng = np.random.default_rng(61)
    x = torch.from_numpy((0.25 * rng.standard_normal((3, 2, 700))).astype(np.float32)).cuda().requires_grad_()
    y, out_lengths = clips(x, lengths)
    assert y.requires_grad and y.grad_fn is not None and not out_lengths.requires_grad
    g = (0.25 * rng.standard_normal(tuple(y.shape))).astype(np.float32)
    (y * torch.from_numpy(g).cuda()).sum().backward()
    torch.cuda.synchronize()
    grad = x.grad.cpu().numpy()
    assert grad.shape == (3, 2, 700)
    for i, n in enumerate(lengths):
        dense = R.dense_operator(380, 380, flags, n, fixed=DOWN)
        assert int(out_lengths[i]) == dense.shape[0]
        check_sums(grad[i][:, :n], dense, g[i][:, :dense.shape[0]], ("autograd clip", i))
        assert np.all(grad[i][:, n:] == 0), i
    with pytest.raises(RuntimeError):                             # (once differentiable)
        x2 = x.detach().clone().requires_grad_()
        y2, _ = clips(x2, lengths)
        (gx2,) = torch.autograd.grad(y2.sum(), x2, create_graph=True)
        gx2.sum().backward()
    clips.close()


def test_autograd_leaves_the_call_without_grad_unchanged():
    torch = pytest.importorskip("torch")
    clips = A.ClipResampler(2, 44100, 16000)
    x = torch.from_numpy((0.25 * np.random.default_rng(71).standard_normal((3, 2, 700))).astype(np.float32)).cuda()
    plain, lengths = clips(x, [700, 350, 0])
    assert plain.grad_fn is None and not plain.requires_grad
    attached, lengths2 = clips(x.clone().requires_grad_(), [700, 350, 0])
    with torch.no_grad():
        quiet, _ = clips(x.clone().requires_grad_(), [700, 350, 0])
    torch.cuda.synchronize()
    assert attached.grad_fn is not None and quiet.grad_fn is None and not quiet.requires_grad
    assert torch.equal(lengths, lengths2) and torch.equal(plain, attached.detach()) and torch.equal(plain, quiet)
    # ... and what it returns is what a fresh context makes of each clip alone (today's contract)
    r = A.Resampler(2, 380, 380, 0.0, BH | IN | LP, (44100.0, 16000.0, 0))
    for i, n in enumerate([700, 350]):
        r.reset()
        y = torch.zeros(2, 1024, device="cuda")
        _, made = r.process_and_flush_planar_device(x[i].contiguous(), 700, n, y, 1024, 1024, 0.0)
        torch.cuda.synchronize()
        assert made == int(lengths[i]) and torch.equal(y[:, :made], plain[i, :, :made])
    r.close(); clips.close()


def test_autograd_gradcheck_on_the_8_byte_build():
    torch = pytest.importorskip("torch")
    B = A.binding(64)
    clips = B.ClipResampler(2, 44100, 16000, taps=16, filters=16)
    x = torch.from_numpy(0.25 * np.random.default_rng(81).standard_normal((2, 2, 24))).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda t: clips(t, [24, 17])[0], (x,), eps=1e-6, atol=1e-7, rtol=1e-6)
    clips.close()
