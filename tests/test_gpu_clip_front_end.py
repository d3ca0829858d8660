"""GPU: what the six clip classes' shared front end can get wrong — row addresses, pitches and the offsets of the max_batch chunks.
Every class at max_batch = 2 on three clips (the chunk loop runs twice, the second chunk from a clip that is not the first; ClipStretcher:
four clips of one pool) must give, bit for bit, what the same class gives on a plain contiguous tensor in one chunk, for a slice of a
wider tensor (the row pitch is not T), a [C, T] input against x[None], and one channel (pitch 0 in either layout); where the class is
differentiable the same for x.grad, with a grad_y that is broadcast (y.sum()), contiguous, and expanded along the batch."""
import numpy as np
import pytest

import audio_resampler_amd as A

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

T, PAD, LENGTHS = 257, 320, [257, 0, 100, 31]
CLASSES = ("ClipResampler", "ClipWarper", "ClipDecimator", "ClipFilter", "ClipBiquad", "ClipStretcher")
DIFFERENTIABLE = tuple(c for c in CLASSES if c != "ClipDecimator")
WARP = np.array([[1.0, 0.5, 1.7], [0.8, 0.8, 0.8], [2.0, 1.1, 0.6], [0.9, 1.0, 1.0]])      # a ratio per block of 100 frames
STRETCH = [1.25, 0.8, 1.5, 1.1]                                   # (all of the single-stage pool)
SECTIONS = [("lowpass", 0.1), ("highpass", 0.01)]
_cache = {}


def _batch(name):
    return 4 if name == "ClipStretcher" else 3


def _make(name, ch, max_batch):
    if name == "ClipResampler":
        return A.ClipResampler(ch, 44100, 16000, taps=32, filters=32, max_batch=max_batch)
    if name == "ClipWarper":
        return A.ClipWarper(ch, taps=32, filters=32, block=100, max_batch=max_batch)
    if name == "ClipDecimator":
        return A.ClipDecimator(ch, 16, 2, 1.0, 44100, A.DITHER_HIGHPASS | A.SHAPING_ATH_CURVE, max_batch=max_batch)
    if name == "ClipFilter":
        return A.ClipFilter(ch, SECTIONS, max_batch=max_batch)
    if name == "ClipBiquad":
        return A.ClipBiquad(ch, A.ClipBiquad.design(SECTIONS))       # (no pool of its own: one call whatever B)
    return A.ClipStretcher(ch, 11025, max_batch=max_batch)


def _run(name, obj, x, lengths, clips):
    """(the samples the call made, its second result as a list or None); clips: which rows of WARP / STRETCH the clips of x take"""
    clips = list(clips)
    if name == "ClipWarper":
        y, n = obj(x, WARP[clips], lengths)
    elif name == "ClipStretcher":
        y, n = obj(x, [STRETCH[i] for i in clips], lengths)
    elif name in ("ClipResampler", "ClipDecimator"):
        y, n = obj(x, lengths)
    else:
        return obj(x, lengths), None
    return y, n.tolist()


def _data(name, ch):
    g = torch.Generator().manual_seed(11 + ch)
    return ((torch.rand(_batch(name), ch, T, generator=g) * 2 - 1) * 1.05).cuda()      # (past full scale here and there: the decimator clips)


def _weights(shape):
    g = torch.Generator().manual_seed(5)
    return torch.randn(tuple(shape), generator=g).cuda()


def _backward(y, kind):
    if kind == "sum":
        y.sum().backward()                                        # (grad_y: one value broadcast, every stride 0)
    elif kind == "weighted":
        (y * _weights(y.shape)).sum().backward()                  # (grad_y contiguous: its rows are handed on as they lie)
    else:
        y.backward(_weights(y.shape)[:1].expand(y.shape))         # (grad_y with a batch stride of 0: taken through .contiguous())


def _reference(name, ch, kind=None):
    """the class on the plain contiguous tensor, every clip in one chunk: (y, second result, x.grad or None) — made once"""
    key = (name, ch, kind)
    if key not in _cache:
        B = _batch(name)
        obj = _make(name, ch, 1024)
        x = _data(name, ch).clone().requires_grad_(kind is not None)
        y, n = _run(name, obj, x, LENGTHS[:B], range(B))
        if kind == "expand":
            y.backward(_weights(y.shape)[:1].expand(y.shape).contiguous())      # (the same values, laid out plainly)
        elif kind is not None:
            _backward(y, kind)
        _cache[key] = (y.detach().clone(), n, None if kind is None else x.grad.clone())
        torch.cuda.synchronize()
        obj.close()
    return _cache[key]


def _padded(base):
    """base's values as the first T frames of a wider tensor (7.0 behind them): (the wide tensor, its slice)"""
    big = torch.full(tuple(base.shape[:-1]) + (PAD,), 7.0, dtype=base.dtype, device=base.device)
    big[..., :T] = base
    return big, big[..., :T]


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("name", CLASSES)
def test_chunks_and_row_pitch(name, ch):
    B = _batch(name)
    want_y, want_n, _ = _reference(name, ch)
    obj = _make(name, ch, 2)
    for form in ("contiguous", "slice"):
        base = _data(name, ch)
        big, x = _padded(base) if form == "slice" else (None, base.clone())
        y, n = _run(name, obj, x, LENGTHS[:B], range(B))
        assert n == want_n and y.shape == want_y.shape and torch.equal(y, want_y), (name, form)
        if form == "slice":
            assert bool((big[..., T:] == 7.0).all())              # (nothing is written past a row's frames)
            if name == "ClipFilter":
                assert y.data_ptr() == big.data_ptr()              # (in place: on the rows of the wide tensor themselves)
            else:
                assert torch.equal(x, base)
    obj.close()


@pytest.mark.parametrize("name", CLASSES)
def test_two_dimensional_input_is_one_clip(name):
    want_y, want_n, _ = _reference(name, 2)
    obj = _make(name, 2, 2)
    for i in (0, 2):
        base = _data(name, 2)
        y2, n2 = _run(name, obj, base[i].clone(), [LENGTHS[i]], [i])
        y3, n3 = _run(name, obj, base[i:i + 1].clone(), [LENGTHS[i]], [i])
        assert y3.dim() == 3 and y2.dim() == (2 if name in ("ClipFilter", "ClipBiquad") else 3)
        assert n2 == n3 and torch.equal(y2.reshape(y3.shape), y3)
        assert n3 is None or n3 == want_n[i:i + 1]
        wide = y3.shape[2]
        assert torch.equal(y3[0], want_y[i, :, :wide]) and not bool(want_y[i, :, wide:].any())
    obj.close()


@pytest.mark.parametrize("kind", ["sum", "weighted", "expand"])
@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("name", DIFFERENTIABLE)
def test_gradients_over_chunks_and_row_pitch(name, ch, kind):
    B = _batch(name)
    want_y, want_n, want_g = _reference(name, ch, kind)
    obj = _make(name, ch, 2)
    for form in ("contiguous", "slice"):
        base = _data(name, ch)
        if form == "slice":
            leaf = _padded(base)[0].requires_grad_()
            x = leaf[..., :T]
        else:
            leaf = x = base.clone().requires_grad_()
        y, n = _run(name, obj, x, LENGTHS[:B], range(B))
        assert n == want_n and torch.equal(y.detach(), want_y), (name, form)
        _backward(y, kind)
        assert torch.equal(leaf.grad[..., :T], want_g), (name, form)
        assert not bool(leaf.grad[..., T:].any())
        assert torch.equal(leaf.detach()[..., :T], base)          # (the tracked call writes nothing, ClipFilter's included)
    obj.close()


def test_gradient_of_a_two_dimensional_input():
    for name in DIFFERENTIABLE:
        _, _, want_g = _reference(name, 2, "weighted")
        want_y = _reference(name, 2, "weighted")[0]
        obj = _make(name, 2, 2)
        x = _data(name, 2)[2].clone().requires_grad_()
        y, _ = _run(name, obj, x, [LENGTHS[2]], [2])
        wide = y.shape[-1]
        (y.reshape(1, 2, wide) * _weights(want_y.shape)[2:3, :, :wide]).sum().backward()
        assert torch.equal(x.grad, want_g[2]), name
        obj.close()


def test_clip_biquad_coefficient_gradient_on_a_slice():
    grads = []
    for form in ("contiguous", "slice"):
        co = A.ClipBiquad.design(SECTIONS).requires_grad_()
        obj = A.ClipBiquad(2, co)
        base = _data("ClipBiquad", 2)
        leaf = (_padded(base)[0] if form == "slice" else base.clone()).requires_grad_()
        y = obj(leaf[..., :T], LENGTHS[:3])
        (y * _weights(y.shape)).sum().backward()
        grads.append((y.detach().clone(), leaf.grad[..., :T].clone(), co.grad.clone()))
        obj.close()
    assert torch.equal(grads[0][0], _reference("ClipBiquad", 2)[0])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
