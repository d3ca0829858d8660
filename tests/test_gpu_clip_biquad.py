"""ClipBiquad: a whole-clip biquad cascade whose coefficients can be learnt.  The forward values are the existing out-of-place entry's,
bit for bit (against ClipFilter's tracked path and against the CPU oracle); the coefficient gradient is the lagged sums of the rows
the ORACLE makes — y_s (prefix 1..s forwards), g_s (suffix s+1..S reversed), u_s (g_s through section s's all-pole part, reversed) —
formed in exact arithmetic and compared within a derived bound; grad_x is the flipped oracle's, bit for bit.

The bound per coefficient: |got - want| <= c * |want| + N * 2^-52 * sum |terms|, N all terms over clips and channels.  c is the cast
of the fp64 result to the coefficients' dtype (2^-23 for float32; 2^-52 for the 8-byte build, where there is none); the second term is
twice the first-order bound of adding N doubles in any order (the kernel's tiles, then torch's sum over clips and channels), which
also covers the one rounding of each product in the 8-byte build."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import audio_resampler_amd as A
import test_gpu_biquad_batch as TB
import test_gpu_biquad_clips as TC
import test_gpu_biquad_planar as TP
import test_gpu_biquad_filter_clips as TF

pytestmark = pytest.mark.gpu

_bits, _signal, _dtype, _width = TB._bits, TP._signal, TP._dtype, TP._width
_oracle_forward, _oracle_reversed, _same_bits = TF._oracle_forward, TF._oracle_reversed, TF._same_bits
NAMES = ("a0", "a1", "a2", "a3", "a4", "b1", "b2", "b3", "b4")


def _np(M):
    return np.float64 if _width(M) == 64 else np.float32


# ---- coefficients ------------------------------------------------------------------------------------------------------------------
def _hand(M, channels=None):
    """the existing hand-made sections, orders 1-4 by channel and section: [4, 9], or [channels, 4, 9] with channels that differ"""
    row = lambda k: [TB.HAND[k].get(n, 0.0) for n in NAMES]
    if channels is None:
        return torch.tensor([row(1 + s % 4) for s in range(4)], dtype=_dtype(M))
    return torch.tensor([[row(1 + (c + s) % 4) for s in range(4)] for c in range(channels)], dtype=_dtype(M))


def _art(M, channels=None):
    """ART's -p: [2, 9]; per channel: the second channel's second section at the other cut-off"""
    co = M.ClipBiquad.design(TP.ART_P)
    if channels is None:
        return co
    other = M.ClipBiquad.design([("lowpass", TB.PRE), ("lowpass", TB.POST)])
    return torch.stack([co if c % 2 == 0 else other for c in range(channels)])


def _per_channel(co, channels):
    h = co.detach().cpu().numpy()
    return np.ascontiguousarray(np.broadcast_to(h, (channels,) + h.shape) if h.ndim == 2 else h)


def _secs(M, co, which, pole=False):
    """section records (channel-major) of the sections `which` of co [C, S, 9], as biquad_init with gain 1.0 makes them; pole: their
    all-pole parts"""
    Cn = co.shape[0]
    secs = (M.Biquad * (Cn * len(which)))()
    for c in range(Cn):
        for j, s in enumerate(which):
            v = [float(q) for q in co[c, s]]
            if pole:
                v[:5] = [1.0, 0.0, 0.0, 0.0, 0.0]
            M.lib().biquad_init(C.byref(secs[c * len(which) + j]), C.byref(M.BiquadCoefficients(*v)), 1.0)
    return secs


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _oracle_rows(M, co, x, gy):
    """x, gy: numpy [C, n] -> (y_0 .. y_S, g_0 .. g_S, u_1 .. u_S (index 0: None)), every row by the CPU oracle"""
    S = co.shape[1]
    y = [x] + [_oracle_forward(M, _secs(M, co, list(range(s))), s, x) for s in range(1, S + 1)]
    g = [_oracle_reversed(M, _secs(M, co, list(range(s, S))), S - s, gy) for s in range(S)] + [gy]
    u = [None] + [_oracle_reversed(M, _secs(M, co, [s - 1], pole=True), 1, g[s]) for s in range(1, S + 1)]
    return y, g, u


def _reference(M, co, x, lengths, gy):
    """co [C, S, 9], x and gy numpy [B, C, T] -> terms[c][s][j]: every product of coefficient j's sum over the clips (a-columns: u_s[t]
    y_{s-1}[t-k]; b-columns: u_s[t] y_s[t-k], to be negated), and grad_x by the oracle"""
    Cn, S, _ = co.shape
    terms = [[[[] for _ in range(9)] for _ in range(S)] for _ in range(Cn)]
    gx = gy.copy()
    for i, n in enumerate(lengths):
        y, g, u = _oracle_rows(M, co, np.ascontiguousarray(x[i][:, :n]), np.ascontiguousarray(gy[i][:, :n]))
        gx[i][:, :n] = g[0]
        for c in range(Cn):
            for s in range(1, S + 1):
                for j in range(9):
                    k, v = (j, y[s - 1][c]) if j < 5 else (j - 4, y[s][c])
                    if k < n:
                        terms[c][s - 1][j].append(u[s][c][k:n].astype(np.float64) * v[:n - k].astype(np.float64))
    return terms, gx


def _check_coefficient_gradient(M, got, terms, shared, what):
    """got: the gradient as numpy, [S, 9] (shared: the channels' terms together) or [C, S, 9]"""
    cast = 2.0 ** -52 if _width(M) == 64 else 2.0 ** -23
    Cn, S = len(terms), len(terms[0])
    groups = [[c for c in range(Cn)]] if shared else [[c] for c in range(Cn)]
    worst = 0.0
    for gi, group in enumerate(groups):
        for s in range(S):
            for j in range(9):
                parts = [t for c in group for t in terms[c][s][j]]
                flat = np.concatenate(parts) if parts else np.zeros(0)
                want = math.fsum(flat.tolist()) * (1.0 if j < 5 else -1.0)
                mass, N = math.fsum(np.abs(flat).tolist()), flat.size
                g = float(got[s, j] if shared else got[gi, s, j])
                bound = cast * abs(want) + N * 2.0 ** -52 * mass
                worst = max(worst, abs(g - want) / bound if bound else 0.0)
                assert abs(g - want) <= bound, (what, gi, s, NAMES[j], g, want, abs(g - want), bound)
    print(what, "largest error / bound:", worst)


def _long_length(M, co, channels):
    """a clip on the time-parallel route of the whole bank: max (513, 2 L + 1)"""
    full = _per_channel(co, channels)
    L = TC._chunk(M, _secs(M, full, list(range(full.shape[1]))), full.shape[1])
    assert L, "the test's filters forget"
    T = max(TB._serial_max(M) + 1, 2 * L + 1)
    assert 513 <= T <= 4000
    return T


# ---- 4. forward bits ---------------------------------------------------------------------------------------------------------------
def test_forward_is_clip_filters_tracked_path_bit_for_bit():
    """(on the parent commit this fails: there is no ClipBiquad)"""
    lengths = [700, 513, 40]
    cf = A.ClipFilter(2, TP.ART_P)
    x0 = _signal(3 * 2, 700, 77, torch.float32).view(3, 2, 700)
    want = cf(x0.clone().requires_grad_(), lengths).detach()
    for co in (A.ClipBiquad.design(TP.ART_P), A.ClipBiquad.design(TP.ART_P).cuda().requires_grad_()):
        cb = A.ClipBiquad(2, co)
        x = x0.clone()
        y = cb(x, lengths)
        torch.cuda.synchronize()
        assert y is not x and y.data_ptr() != x.data_ptr() and cb.launches > 0
        assert y.requires_grad == co.requires_grad
        assert torch.equal(_bits(y.detach()), _bits(want))               # the tails too: x copied through
        assert torch.equal(_bits(x), _bits(x0))                          # x keeps its bits
        for i, n in enumerate(lengths):
            assert torch.equal(_bits(y.detach()[i, :, n:]), _bits(x0[i, :, n:]))
        # a non-contiguous x, and one clip [C, T]
        xt = x0.transpose(1, 2).contiguous().transpose(1, 2)
        assert xt.stride(2) != 1 and torch.equal(_bits(cb(xt, lengths).detach()), _bits(want))
        assert torch.equal(_bits(cb(x0[1], None).detach()), _bits(cb(x0[1:2], [700]).detach()[0]))
        with pytest.raises(ValueError):
            cb(x0, [700, 701, 0])
        with pytest.raises(ValueError):
            cb(x0.double(), lengths)
        cb.close()
    cf.close()


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("make", [_art, _hand], ids=["art", "hand"])
def test_forward_with_per_channel_coefficients_is_the_oracles(width, make):
    M = A.binding(width)
    co = make(M, 2)
    assert not torch.equal(co[0], co[1])
    lengths = [700, 513, 40]
    x0 = _signal(3 * 2, 700, 79, _dtype(M)).view(3, 2, 700)
    for tracked in (False, True):
        cb = M.ClipBiquad(2, co.clone().requires_grad_(tracked))
        x = x0.clone()
        y = cb(x, lengths).detach().cpu().numpy()
        assert torch.equal(_bits(x), _bits(x0))
        h, secs = x0.cpu().numpy(), _secs(M, co.numpy(), list(range(co.shape[1])))
        for i, n in enumerate(lengths):
            assert _same_bits(y[i][:, :n], _oracle_forward(M, secs, co.shape[1], h[i][:, :n])), (tracked, i)
            assert _same_bits(y[i][:, n:], h[i][:, n:]), (tracked, i)
        cb.close()


# ---- 5. the coefficient gradient is the lag sums of the oracle's rows --------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per-channel"])
@pytest.mark.parametrize("make", [_art, _hand], ids=["art-S2", "hand-S4"])
def test_coefficient_gradient_is_the_lag_sums_of_the_oracles_rows(width, per_channel, make):
    M = A.binding(width)
    Cn = 2
    co0 = make(M, Cn if per_channel else None)
    full = _per_channel(co0, Cn)
    T = _long_length(M, co0, Cn)
    lengths = [T, 96, T - 37]                                            # the time-parallel route, the serial one, a clip with a tail
    x0 = _signal(3 * Cn, T, 201, _dtype(M)).view(3, Cn, T).mul_(0.25)
    gy = _signal(3 * Cn, T, 202, _dtype(M)).view(3, Cn, T)
    terms, want_gx = _reference(M, full, x0.cpu().numpy(), lengths, gy.cpu().numpy())

    grads = []
    for x_tracked in (True, False):
        co = co0.clone().requires_grad_()
        cb = M.ClipBiquad(Cn, co)
        x = x0.clone().requires_grad_(x_tracked)
        y = cb(x, lengths)
        (y * gy).sum().backward()
        torch.cuda.synchronize()
        assert co.grad.shape == co.shape and co.grad.dtype == co.dtype and not co.grad.is_cuda
        _check_coefficient_gradient(M, co.grad.numpy(), terms, not per_channel, (width, per_channel, make.__name__, x_tracked))
        grads.append(co.grad.clone())
        if x_tracked:
            assert _same_bits(x.grad.cpu().numpy(), want_gx)             # the flipped oracle's, the tails passed through
        else:
            assert x.grad is None
        assert torch.equal(_bits(x.detach()), _bits(x0))
        cb.close()
    assert torch.equal(_bits(grads[0]), _bits(grads[1]))                 # with or without grad_x: the same bits
    assert bool((grads[0] != 0).all())                                   # all nine columns, whatever order biquad_init derived


# ---- 6. gradcheck on the 8-byte build ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_channel", [False, True], ids=["shared", "per-channel"])
def test_gradcheck_in_x_and_the_coefficients_on_the_8_byte_build(per_channel):
    """the suite's settings and the shape the closed form was checked with on the CPU.  gradcheck perturbs its inputs through
    .data, which moves no _version: the function makes a ClipBiquad per evaluation, so every evaluation reads the values it is given"""
    B = A.binding(64)
    low = B.ClipBiquad.design([("lowpass", 0.2)])[0]
    hand = torch.tensor([TB.HAND[4][n] for n in NAMES], dtype=torch.float64)
    co = torch.stack([low, hand])
    if per_channel:
        co = torch.stack([co, co * torch.tensor([[0.9], [1.1]], dtype=torch.float64)])
    co = co.cuda().requires_grad_()
    x = torch.from_numpy(0.25 * np.random.default_rng(81).standard_normal((2, 2, 40))).cuda().requires_grad_()
    assert torch.autograd.gradcheck(lambda t, c: B.ClipBiquad(2, c)(t, [40, 23]), (x, co), eps=1e-6, atol=1e-7, rtol=1e-6)


# ---- 7. plumbing -------------------------------------------------------------------------------------------------------------------
def test_launch_counts_do_not_grow_with_the_batch():
    co = _hand(A).requires_grad_()
    T = _long_length(A, co, 2)
    counts = []
    for B in (1, 5):
        cb = A.ClipBiquad(2, co)
        x = _signal(B * 2, T, 300 + B, torch.float32).view(B, 2, T).requires_grad_()
        y = cb(x)
        y.sum().backward()
        torch.cuda.synchronize()
        counts.append((cb.launches, tuple(cb.backward_launches)))
        cb.close()
    assert counts[0] == counts[1], counts
    assert counts[0][0] > 0 and all(v > 0 for v in counts[0][1]) and counts[0][1][2] == 2


def test_cpu_and_gpu_resident_coefficients_give_the_same_bits():
    lengths = [700, 96]
    x0 = _signal(2 * 2, 700, 310, torch.float32).view(2, 2, 700)
    out = []
    for device in ("cpu", "cuda"):
        co = _art(A, 2).to(device).requires_grad_()
        cb = A.ClipBiquad(2, co)
        y = cb(x0.clone(), lengths)
        y.square().sum().backward()
        torch.cuda.synchronize()
        assert co.grad.device == co.device and co.grad.dtype == co.dtype
        out.append((y.detach().clone(), co.grad.cpu().clone()))
        cb.close()
    assert torch.equal(_bits(out[0][0]), _bits(out[1][0])) and torch.equal(_bits(out[0][1]), _bits(out[1][1]))


def test_the_cache_follows_the_tensors_version_and_a_backward_keeps_its_forwards_banks():
    lengths = [700, 96]
    x0 = _signal(2 * 2, 700, 320, torch.float32).view(2, 2, 700)
    co = _art(A).requires_grad_()
    cb = A.ClipBiquad(2, co)
    quiet = A.ClipBiquad(2, _art(A).requires_grad_())                    # the same values, never changed
    y1, yq = cb(x0, lengths), quiet(x0, lengths)
    first = y1.detach().clone()
    assert torch.equal(_bits(first), _bits(cb(x0, lengths).detach()))   # the same version: the same banks, the same bits
    with torch.no_grad():
        co[0, 0] *= 0.5                                                  # in place: _version moves
    y2 = cb(x0, lengths)
    torch.cuda.synchronize()
    assert not torch.equal(y2.detach(), first)
    # the backward of the first forward differentiates that forward, not the coefficients of now
    y1.sum().backward()
    yq.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(_bits(co.grad), _bits(quiet.coefficients.grad))
    with pytest.raises(RuntimeError):                                    # a second backward
        y1.sum().backward()
    cb.close()
    with pytest.raises(RuntimeError):                                    # backward after close()
        y2.sum().backward()
    y3 = cb(x0, lengths)                                                 # (the object serves again after close ())
    y3.sum().backward()
    quiet.close()
    cb.close()


def test_wrong_coefficients_raise():
    good = _art(A)
    for wrong in (torch.zeros(9), torch.zeros(2, 8), torch.zeros(5, 9), torch.zeros(0, 9), torch.zeros(3, 2, 9), torch.zeros(2, 2, 2, 9),
                  good.double(), good.numpy()):
        with pytest.raises(ValueError):
            A.ClipBiquad(2, wrong)
    with pytest.raises(ValueError):
        A.wide().ClipBiquad(2, good)


# ---- 8. a chain --------------------------------------------------------------------------------------------------------------------
def test_chain_into_clip_resampler():
    """ClipBiquad -> ClipResampler: the coefficient gradient is test 5's reference computed from the gradient that reached the
    filter's output (read with retain_grad), and grad_x the flipped oracle's of that gradient"""
    lengths = [600, 411]
    co = _art(A, 2).requires_grad_()
    cb, rs = A.ClipBiquad(2, co), A.ClipResampler(2, 44100, 16000)
    x = _signal(2 * 2, 600, 91, torch.float32).view(2, 2, 600).mul_(0.25).requires_grad_()
    mid = cb(x, lengths)
    mid.retain_grad()
    y, out_lengths = rs(mid, lengths)
    g = (0.25 * np.random.default_rng(92).standard_normal(tuple(y.shape))).astype(np.float32)
    (y * torch.from_numpy(g).cuda()).sum().backward()
    torch.cuda.synchronize()
    gmid = mid.grad.cpu().numpy()
    assert np.any(gmid != 0)
    terms, want_gx = _reference(A, co.detach().numpy(), x.detach().cpu().numpy(), lengths, gmid)
    _check_coefficient_gradient(A, co.grad.numpy(), terms, False, "chain")
    assert _same_bits(x.grad.cpu().numpy(), want_gx)
    cb.close(); rs.close()
