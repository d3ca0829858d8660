"""GPU: resampleRateGradientScheduleClipsPlanarDevice and ClipRateWarper.  The yardstick is tests/_rate_grad_ref.py (the strict CPU oracle's bank
and counts, restated in float64; tests/test_rate_grad_ref.py holds it to the oracle), never the library's own forward.

1. the entry against the helper, per block within (T + 8 + depth) 2^-53 sum |terms|.  T fused multiply-adds of a chain and eight single
   roundings (the bank rows' difference, F *, gy *, n *, n_k * behind, rho * rho, the division, the helper's own last bit), and depth,
   the additions between a term and the result, read off the kernels' reduction tree:
       C - 1 (the channels of an output) + 6 (the butterfly over a wave) + 3 (the four waves) + tiles of the phase (the finish's ascending
       sum, the first onto zero) + K (the S0 of the phases behind, one by one) + 1 (S1 + n * behind) + 1 (the flush onto the last block);
2. a unit gradient at one output of the first, a middle and the flush phase gives that output's own row: every sum but the chain is then
   exact or a single rounding, and the chain is replayed here in exact arithmetic, so the row is asked for within one rounding;
3. the bits of a clip's gradient do not depend on the batch, the place, the layout, the pitch, the stream or the contexts listed; a cut
   numOutputFrames is zeroed gy; NaN past the cut and past the clip does not get in;
4. refusals on the device; 5. ClipRateWarper and its autograd; 6. torch.autograd.gradcheck in x and the ratios together (8-byte build)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import audio_resampler_amd as A
from audio_resampler_amd import rate_grad
import _rate_grad_ref as R

pytestmark = pytest.mark.gpu
BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
TAPS, FILTERS, TILE = 16, 16, 256
SENTINEL = -777.25
SMOOTH = (1.3071, 0.8213, 1.1037)
# (blocks, ratios) of the clips that share the first test's call
CLIPS = [
    ((16, 16, 9), SMOOTH), ((16,), (0.8213,)), ((1,), (1.3071,)), ((0,), (1.1037,)), ((16, 16, 1), (0.8213, 1.3071, 1.1037)),     # lengths 41, 16, 1, 0, 33
    ((40, 40), (8.0, 8.0)),                    # a phase of more than one tile
    ((1,) * 64, (0.3,) * 64),                  # phases without outputs, and more phases than the finishing wave takes in one trip
    ((100, 60), (0.05, 0.05)),
    ((16, 16, 9), (1.1, 0.8, 1.3)), ((16, 16, 9), (0.6, 1.7, 0.9)),      # outputs on filter boundaries: the convention, on the device
]


def np_of(width):
    return np.float64 if width == 64 else np.float32


def flags_of(lowpass):
    return BH | IN | (LP if lowpass else 0)


def make(blocks, ratios, channels, lowpass, width, seed):
    """(x [C, N], gy [C, M]) of noise in the build's sample type, as float64"""
    rng = np.random.default_rng(seed)
    M = sum(R.replay(TAPS, FILTERS, lowpass, flags_of(lowpass), blocks, ratios, None, width)[0])
    return ((0.25 * rng.standard_normal((channels, int(sum(blocks))))).astype(np_of(width)).astype(np.float64),
            rng.standard_normal((channels, M)).astype(np_of(width)).astype(np.float64))


def depth_of(ref, channels):
    K = len(ref.counts) - 1
    return channels - 1 + 6 + 3 + max(1, max(-(-c // TILE) for c in ref.counts)) + K + 1 + 1


def plane(a, pitch, fill, width):
    """a [C, n] as planes `pitch` apart (pitch 0: interleaved), the gaps filled with `fill`"""
    Cn, n = a.shape
    if not pitch:
        return np.ascontiguousarray(a.T).reshape(-1).astype(np_of(width))
    host = np.full((Cn, pitch), fill, np_of(width))
    host[:, :n] = a
    return host.reshape(-1)


def entry(width, ctxs, clips, xs, gys, planar=True, x_pad=0, gy_pad=0, base=0, n_outs=None, fill=0.0, stream=None):
    """one call -> (launches, [grad_i float64 [K_i]]); every gradient buffer has two doubles more on either side, which must survive"""
    import torch
    dt, size = (torch.float64, 8) if width == 64 else (torch.float32, 4)
    keep, x_ptr, x_pitch, gy_ptr, gy_pitch, g_ptr = [], [], [], [], [], []
    for (blocks, _), x, gy in zip(clips, xs, gys):
        Cn = x.shape[0]
        px, pg = (x.shape[1] + x_pad, gy.shape[1] + gy_pad) if planar and Cn > 1 else (0, 0)
        if Cn == 1 and (x_pad or gy_pad):                         # (one channel: the frames past the clip are the padding)
            x, gy = np.concatenate([x, np.full((1, x_pad), fill)], 1), np.concatenate([gy, np.full((1, gy_pad), fill)], 1)
        tx = torch.from_numpy(np.concatenate([np.zeros(base, np_of(width)), plane(x, px, fill, width), np.zeros(1, np_of(width))])).cuda()
        tg = torch.from_numpy(np.concatenate([np.zeros(base, np_of(width)), plane(gy, pg, fill, width), np.zeros(1, np_of(width))])).cuda()
        out = torch.full((len(blocks) + 4,), SENTINEL, dtype=torch.float64, device="cuda")
        keep.append((tx, tg, out))
        x_ptr.append(tx.data_ptr() + base * size); gy_ptr.append(tg.data_ptr() + base * size); g_ptr.append(out.data_ptr() + 16)
        x_pitch.append(px); gy_pitch.append(pg)
    n_outs = [g.shape[1] for g in gys] if n_outs is None else n_outs
    call = rate_grad.binding(width).rate_gradient_schedule_clips_planar_device
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    launches = call(ctxs, x_ptr, x_pitch, gy_ptr, gy_pitch, n_outs, [list(c[0]) for c in clips], [list(c[1]) for c in clips], g_ptr)
    torch.cuda.synchronize()
    got = []
    for (blocks, _), (_, _, out) in zip(clips, keep):
        h = out.cpu().numpy()
        assert np.all(h[:2] == SENTINEL) and np.all(h[2 + len(blocks):] == SENTINEL), "written outside the clip's numBlocks doubles"
        got.append(h[2:2 + len(blocks)].copy())
    return launches, got


# ---- 1. the entry against the helper ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 2, 5])
@pytest.mark.parametrize("lowpass", [0.0, 0.45])
@pytest.mark.parametrize("width", [32, 64])
def test_entry_matches_the_helper(width, lowpass, channels):
    pytest.importorskip("torch")
    B = A.binding(width)
    flags = flags_of(lowpass)
    ctx = B.Resampler(channels, TAPS, FILTERS, lowpass, flags)
    data = [make(b, r, channels, lowpass, width, 100 + i) for i, (b, r) in enumerate(CLIPS)]
    refs = [R.clip(TAPS, FILTERS, lowpass, flags, b, r, x, gy, width) for (b, r), (x, gy) in zip(CLIPS, data)]
    assert max(refs[5].counts) > TILE and refs[6].counts.count(0) > 10 and len(refs[6].counts) > 64 and sum(refs[7].counts[:1]) <= 6
    launches, got = entry(width, [ctx] * len(CLIPS), CLIPS, [d[0] for d in data], [d[1] for d in data])
    assert launches == 2
    worst = 0.0
    for i, (ref, g) in enumerate(zip(refs, got)):
        bound = (TAPS + 8 + depth_of(ref, channels)) * 2.0 ** -53 * ref.terms
        err = np.abs(g - ref.grad)
        if ref.terms.max() > 0:
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (i, CLIPS[i], g, ref.grad, err, bound)
        assert np.all(np.isfinite(g)) and (sum(CLIPS[i][0]) == 0) == bool(np.all(g == 0)), (i, g)
    print("width", width, "lowpass", lowpass, "channels", channels, "worst error / bound", worst)
    ctx.close()


# ---- 2. unit gradients ------------------------------------------------------------------------------------------------------------------
def chain(bank, fi, window):
    """F * the device's chain in exact arithmetic, every step rounded once: fma ((double) b_hi - (double) b_lo, x, acc), t ascending"""
    acc = 0.0
    for t, x in window:
        d = float(bank[fi + 1][t]) - float(bank[fi][t])
        acc = float(Fraction(d) * Fraction(float(x)) + Fraction(acc))
    return FILTERS * acc


@pytest.mark.parametrize("width", [32, 64])
def test_a_unit_gradient_gives_the_outputs_own_row(width):
    pytest.importorskip("torch")
    import _oracle as O
    B = A.binding(width)
    flags = flags_of(0.45)
    blocks, ratios = (16, 16, 9), SMOOTH
    x, _ = make(blocks, ratios, 1, 0.45, width, 7)
    ref = R.clip(TAPS, FILTERS, 0.45, flags, blocks, ratios, x, None, width)
    bank = O.binding(width).OracleResampler(1, TAPS, FILTERS, 0.45, flags, kind="strict").bank()
    K, M = len(blocks), len(ref.n)
    rho = list(ratios) + [ratios[-1]]
    picks = [int(np.flatnonzero((ref.phase == k) & (ref.n > 0))[q]) for k, q in ((0, 2), (1, -1), (K, 0))]
    ctx = B.Resampler(1, TAPS, FILTERS, 0.45, flags)
    gys = []
    for m in picks:
        gy = np.zeros((1, M)); gy[0, m] = 1.0
        gys.append(gy)
    launches, got = entry(width, [ctx] * len(picks), [(blocks, ratios)] * len(picks), [x] * len(picks), gys)
    for m, g in zip(picks, got):
        k, n = int(ref.phase[m]), float(ref.n[m])
        end = int(np.cumsum(blocks)[k]) if k < K else int(sum(blocks))
        first = int(ref.ip[m])
        fi = int(ref.cell[m] % FILTERS)
        D = chain(bank, fi, [(t, x[0, first + t]) for t in range(TAPS) if 0 <= first + t < end])
        assert D != 0.0 and abs(D - ref.D[0, m]) <= TAPS * 2.0 ** -52 * abs(ref.D[0, m]) + 1e-300
        v = 1.0 * D
        per_phase = [0.0 - (n * v if q == k else ref.counts[q] * v if q < k else 0.0) / (rho[q] * rho[q]) for q in range(K + 1)]
        want = np.array(per_phase[:K - 1] + [per_phase[K - 1] + per_phase[K]])
        print("width", width, "output", m, "phase", k, "n", n, "row", g, "exact", bool(np.all(g == want)))
        assert np.all(np.abs(g - want) <= 2.0 ** -52 * np.abs(want)), (m, g, want)
        assert np.all(g[k + 1:] == 0)                              # (a later block does not move this output)
    ctx.close()


# ---- 3. reproducibility -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_bits_do_not_depend_on_batch_place_layout_pitch_stream_or_contexts(width):
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    flags, lowpass = flags_of(0.45), 0.45
    mine = ((16, 16, 9), SMOOTH)
    x, gy = make(*mine, 2, lowpass, width, 11)
    ctxs = [B.Resampler(2, TAPS, FILTERS, lowpass, flags) for _ in range(33)]
    bits = lambda a: a.view(np.uint64).tolist()
    launches, (alone,) = entry(width, ctxs[:1], [mine], [x], [gy])
    assert launches == 2 and np.all(alone != 0)
    others = [((16, 7), (0.9371, 1.2113)), ((40, 40), (8.0, 8.0)), ((1,) * 9, (0.3,) * 9), ((0,), (1.0,))]
    batch = [others[i % len(others)] for i in range(33)]
    batch[17] = mine
    data = [make(b, r, 2, lowpass, width, 200 + i) for i, (b, r) in enumerate(batch)]
    data[17] = (x, gy)
    for listed in (ctxs, [ctxs[5]] * 33):                          # (33 contexts, then one listed for all)
        _, got = entry(width, listed, batch, [d[0] for d in data], [d[1] for d in data])
        assert bits(got[17]) == bits(alone)
    _, (interleaved,) = entry(width, ctxs[:1], [mine], [x], [gy], planar=False)
    _, (odd,) = entry(width, ctxs[:1], [mine], [x], [gy], x_pad=3, gy_pad=5, base=1, fill=float("nan"))
    assert bits(interleaved) == bits(alone) and bits(odd) == bits(alone)
    side = torch.cuda.Stream()
    ctxs[2].set_stream(side.cuda_stream)
    _, (streamed,) = entry(width, [ctxs[2]], [mine], [x], [gy], stream=side)
    assert bits(streamed) == bits(alone)
    # a cut numOutputFrames is zeroed gy; NaN behind the cut (and behind the clip's frames, in the padding above) stays out
    cut = gy.shape[1] - 13
    zeroed, poisoned = gy.copy(), gy.copy()
    zeroed[:, cut:] = 0.0; poisoned[:, cut:] = np.nan
    _, (want,) = entry(width, ctxs[:1], [mine], [x], [zeroed])
    _, (got,) = entry(width, ctxs[:1], [mine], [x], [poisoned], n_outs=[cut])
    assert bits(got) == bits(want) and bits(want) != bits(alone)
    mono = B.Resampler(1, TAPS, FILTERS, lowpass, flags)           # (and in one channel, where the padding lies right behind the frames)
    _, (plain,) = entry(width, [mono], [mine], [x[:1]], [zeroed[:1]])
    _, (padded,) = entry(width, [mono], [mine], [x[:1]], [gy[:1, :cut]], x_pad=4, gy_pad=13, fill=float("nan"), n_outs=[cut])
    assert bits(padded) == bits(plain)
    for r in ctxs + [mono]:
        r.close()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
def test_refusals_on_the_device_enqueue_and_count_nothing(width):
    torch = pytest.importorskip("torch")
    B = A.binding(width)
    errors = B.lib().artamdErrorCount()
    flags = flags_of(0.45)
    mine = ((16, 16, 9), SMOOTH)
    x, gy = make(*mine, 1, 0.45, width, 13)
    plain = B.Resampler(1, TAPS, FILTERS, 0.45, flags)
    fixed = B.Resampler(1, TAPS, FILTERS, 0.0, flags, (44100.0, 48000.0, 0))
    nearest = B.Resampler(1, TAPS, FILTERS, 0.45, BH | LP)
    ends = B.Resampler(1, TAPS, FILTERS, 0.45, flags | A.EXTRAPOLATE_ENDPOINTS)
    elsewhere = B.Resampler(1, TAPS, FILTERS, 0.45, flags)
    side = torch.cuda.Stream()
    elsewhere.set_stream(side.cuda_stream)
    dt = torch.float64 if width == 64 else torch.float32
    tx, tg = torch.from_numpy(x[0].astype(np_of(width))).cuda(), torch.from_numpy(gy[0].astype(np_of(width))).cuda()
    out = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    call = rate_grad.binding(width).rate_gradient_schedule_clips_planar_device
    M = gy.shape[1]
    args = lambda ctxs, n_out=M, blocks=mine[0], ratios=mine[1], xs=tx, gs=tg, o=out: (
        ctxs, [xs] * len(ctxs), None, [gs] * len(ctxs), None, [n_out] * len(ctxs), [list(blocks)] * len(ctxs), [list(ratios)] * len(ctxs), [o] * len(ctxs))
    for ctxs in ([fixed], [nearest], [ends], [plain, elsewhere], [plain, nearest]):
        with pytest.raises(RuntimeError):
            call(*args(ctxs))
    for more in (dict(n_out=M + 1), dict(n_out=-1), dict(blocks=(16, -1, 9)), dict(ratios=(1.3, 0.0, 1.1)), dict(xs=None), dict(gs=None), dict(o=None)):
        with pytest.raises(RuntimeError):
            call(*args([plain], **more))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and B.lib().artamdErrorCount() == errors
    assert call(*args([plain])) == 2                              # (and the same call on the plain context is taken)
    assert call([plain, plain], [tx] * 2, None, [tg] * 2, None, [0, 0], [[], []], [[], []], [out, out]) == 0      # (no blocks: nothing written)
    torch.cuda.synchronize()
    h = out.cpu().numpy()
    assert np.all(h[:3] != SENTINEL) and np.all(h[3:] == SENTINEL) and B.lib().artamdErrorCount() == errors
    for r in (plain, fixed, nearest, ends, elsewhere):
        r.close()


# ---- 5. ClipRateWarper ------------------------------------------------------------------------------------------------------------------
LENGTHS, BLOCK = [41, 16, 33], 16
CURVE = [[1.3071, 0.8213, 1.1037], [0.9371, 1.2113, 0.8213], [0.8213, 1.3071, 1.2113]]


def warp_refs(width, x, g, curve, lowpass=0.45):
    """per clip the helper's result for ClipRateWarper's cut of x [B, C, T] (numpy) at curve [B][K], g [B, C, Tout]"""
    refs = []
    for i, n in enumerate(LENGTHS):
        k = max(1, -(-n // BLOCK))
        blocks = tuple(min(BLOCK, n - q * BLOCK) for q in range(k))
        M = sum(R.replay(TAPS, FILTERS, lowpass, flags_of(lowpass), blocks, curve[i][:k], None, width)[0])
        refs.append(R.clip(TAPS, FILTERS, lowpass, flags_of(lowpass), blocks, curve[i][:k], x[i][:, :n], g[i][:, :M], width))
    return refs


@pytest.mark.parametrize("width", [32, 64])
def test_clip_rate_warper_autograd(width):
    torch = pytest.importorskip("torch")
    B, RG = A.binding(width), rate_grad.binding(width)
    dt = torch.float64 if width == 64 else torch.float32
    rng = np.random.default_rng(23)
    xh = (0.25 * rng.standard_normal((3, 2, max(LENGTHS)))).astype(np_of(width))
    x = torch.from_numpy(xh).cuda()
    warper, plain = RG.ClipRateWarper(2, TAPS, FILTERS, flags_of(0.45), 0.45, block=BLOCK), B.ClipWarper(2, TAPS, FILTERS, flags_of(0.45), 0.45, block=BLOCK)
    y0, lengths0 = plain(x, CURVE, LENGTHS)
    gh = rng.standard_normal(tuple(y0.shape)).astype(np_of(width))
    g = torch.from_numpy(gh).cuda()
    xg = x.clone().requires_grad_()
    y1, _ = plain(xg, CURVE, LENGTHS)
    (y1 * g).sum().backward()
    refs = warp_refs(width, xh.astype(np.float64), gh.astype(np.float64), CURVE)
    bound = lambda ref: (TAPS + 8 + depth_of(ref, 2)) * 2.0 ** -53 * ref.terms

    # [B, K] ratios in float64 on the GPU: forward bits, both gradients, entries past a clip's blocks
    r = torch.tensor(CURVE, dtype=torch.float64, device="cuda", requires_grad=True)
    x2 = x.clone().requires_grad_()
    y, lengths = warper(x2, r, LENGTHS)
    assert y.grad_fn is not None and not lengths.requires_grad and torch.equal(y.detach(), y0) and torch.equal(lengths, lengths0)
    (y * g).sum().backward()
    assert torch.equal(x2.grad, xg.grad)                           # (the x gradient is ClipWarper's, bit for bit)
    assert r.grad.dtype == torch.float64 and r.grad.is_cuda and r.grad.shape == (3, 3)
    got = r.grad.cpu().numpy()
    for i, ref in enumerate(refs):
        k = len(ref.grad)
        assert np.all(np.abs(got[i, :k] - ref.grad) <= bound(ref)), (i, got[i], ref.grad)
        assert np.all(got[i, k:] == 0) and np.all(got[i, :k] != 0)
    full = got.copy()

    # the ratios alone (x without grad), in float32 on the GPU and float64 on the CPU: the same values, in the ratios' dtype and place
    for make_r in (lambda: torch.tensor(CURVE, dtype=torch.float64, requires_grad=True),
                   lambda: torch.tensor(CURVE, dtype=torch.float32, device="cuda", requires_grad=True)):
        r = make_r()
        curve = r.detach().cpu().numpy().astype(np.float64).tolist()
        y, _ = warper(x, r, LENGTHS)
        assert y.grad_fn is not None
        # (float32 ratios are other ratios: their own output counts, so their own gradient of the outputs)
        gs = g if r.dtype == torch.float64 else torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np_of(width))).cuda()
        (y * gs).sum().backward()
        assert r.grad.dtype == r.dtype and r.grad.device == r.device
        if r.dtype == torch.float64:
            assert np.array_equal(r.grad.numpy(), full)            # (the same call: the same bits)
        else:
            for i, ref in enumerate(warp_refs(width, xh.astype(np.float64), gs.cpu().numpy().astype(np.float64), curve)):
                k = len(ref.grad)
                err = np.abs(r.grad[i, :k].cpu().numpy().astype(np.float64) - ref.grad)
                assert np.all(err <= bound(ref) + 2.0 ** -24 * np.abs(ref.grad)), (i, err)
    # x alone: ClipWarper's bits again, and no ratio gradient is made
    x3 = x.clone().requires_grad_()
    y, _ = warper(x3, CURVE, LENGTHS)
    (y * g).sum().backward()
    assert torch.equal(x3.grad, xg.grad)

    # [B] and scalar ratios: autograd sums the blocks' gradients back to the caller's shape
    per_clip = [1.1037, 0.8213, 1.3071]
    for shape in ("clip", "scalar"):
        values = per_clip if shape == "clip" else [0.9371] * 3
        r = torch.tensor(values if shape == "clip" else values[0], dtype=torch.float64, device="cuda", requires_grad=True)
        y, lengths = warper(x, r, LENGTHS)
        gs = torch.from_numpy(rng.standard_normal(tuple(y.shape)).astype(np_of(width))).cuda()
        (y * gs).sum().backward()
        rs = warp_refs(width, xh.astype(np.float64), gs.cpu().numpy().astype(np.float64), [[v] * 3 for v in values])
        sums = np.array([ref.grad.sum() for ref in rs])
        # (the blocks' bounds add up; torch's own sum of K or B K entries rounds each partial sum once more)
        slack = np.array([bound(ref).sum() + len(ref.grad) * 2.0 ** -53 * np.abs(ref.grad).sum() for ref in rs])
        got = r.grad.cpu().numpy()
        if shape == "clip":
            assert got.shape == (3,) and np.all(np.abs(got - sums) <= slack), (got, sums, slack)
        else:
            assert got.shape == () and abs(float(got) - sums.sum()) <= slack.sum() + 9 * 2.0 ** -53 * np.abs(sums).sum(), (got, sums.sum())

    # without gradients: the forward alone
    r = torch.tensor(CURVE, dtype=torch.float64, device="cuda", requires_grad=True)
    with torch.no_grad():
        quiet, _ = warper(x, r, LENGTHS)
    detached, _ = warper(x, r.detach(), LENGTHS)
    assert quiet.grad_fn is None and not quiet.requires_grad and detached.grad_fn is None and torch.equal(quiet, y0) and torch.equal(detached, y0)
    with pytest.raises(RuntimeError):                             # (once differentiable)
        y, _ = warper(x, r, LENGTHS)
        (gr,) = torch.autograd.grad((y * g).sum(), r, create_graph=True)
        gr.sum().backward()
    with pytest.raises(RuntimeError):                             # (x is saved for backward: an edit in place is caught)
        x4 = x.clone()
        y, _ = warper(x4, r, LENGTHS)
        x4.add_(1.0)
        y.sum().backward()
    # no clip at all: nothing to make, gradients of the callers' shapes, no context ever needed
    empty = RG.ClipRateWarper(2, TAPS, FILTERS, block=BLOCK)
    x0, r0 = torch.zeros(0, 2, 10, dtype=dt, device="cuda", requires_grad=True), torch.tensor(1.25, dtype=torch.float64, requires_grad=True)
    y, lengths = empty(x0, r0)
    y.sum().backward()
    assert y.shape[:2] == (0, 2) and lengths.tolist() == [] and x0.grad.shape == (0, 2, 10) and float(r0.grad) == 0.0 and empty.pool == []
    # backward after close () raises
    y, _ = warper(x, r, LENGTHS)
    warper.close()
    with pytest.raises(RuntimeError):
        y.sum().backward()
    plain.close()


# ---- 6. gradcheck -----------------------------------------------------------------------------------------------------------------------
def test_gradcheck_in_the_samples_and_the_ratios_on_the_8_byte_build():
    torch = pytest.importorskip("torch")
    RG = rate_grad.binding(64)
    flags, lengths, eps = flags_of(0.0), [24, 17], 2.0 ** -20
    curve = [[1.1037, 0.8213], [0.9371, 1.2113]]
    xh = 0.25 * np.random.default_rng(81).standard_normal((2, 1, 24))
    # the condition of tests/test_rate_grad_ref.py (b): at r +- eps no count and no interpolation cell changes
    slopes = []
    for i, n in enumerate(lengths):
        blocks = (16, n - 16)
        mid = R.clip(TAPS, FILTERS, 0.0, flags, blocks, curve[i], xh[i][:, :n])
        slopes.append(np.abs(mid.D).max())
        for k in range(2):
            lo, hi = list(curve[i]), list(curve[i])
            lo[k] -= eps; hi[k] += eps
            a, b = R.clip(TAPS, FILTERS, 0.0, flags, blocks, lo, xh[i][:, :n]), R.clip(TAPS, FILTERS, 0.0, flags, blocks, hi, xh[i][:, :n])
            assert a.counts == b.counts == mid.counts and np.array_equal(a.cell, b.cell), (i, k)
    # what the oracle's own central differences leave at this step (there: at most 7.8e-10 of sum |g D| seen, 1e-7 allowed): 1e-7 of the
    # largest slope for an entry of the Jacobian, which is one output's D n / rho^2 or a filter weight
    tol = 1e-7 * max(slopes)
    warper = RG.ClipRateWarper(1, TAPS, FILTERS, flags, 0.0, block=16)
    x = torch.from_numpy(xh).cuda().requires_grad_()
    r = torch.tensor(curve, dtype=torch.float64, device="cuda", requires_grad=True)
    print("eps", eps, "atol", tol)
    assert torch.autograd.gradcheck(lambda t, q: warper(t, q, lengths)[0], (x, r), eps=eps, atol=tol, rtol=1e-7)
    warper.close()
