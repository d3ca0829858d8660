"""GPU: ClipResampler — a batch of channels-first clips [B, C, T] plus lengths through one resampleProcessAndFlushBatchPlanarDevice call on
the tensor's own rows.  Every row equals, bit for bit, what a fresh fixed-ratio Resampler makes of that clip alone with
process_planar_device and a flush; the rest of each row is as allocated (zeros)."""
import numpy as np
import pytest

import audio_resampler_amd as A

pytestmark = pytest.mark.gpu
BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
SRC, DST, T = 44100.0, 16000.0, 380
LENGTHS = [3000, 1, 2999, 0, 1500]


def alone(x, frames, flags):
    """clip x [C, frames] on a context of its own: the process call, then the flush behind it in every plane"""
    import torch
    ch = x.shape[0]
    r = A.Resampler(ch, T, T, 0.0, flags, (SRC, DST, 0))
    cap = int(frames * DST / SRC) + T + 64
    y = torch.zeros(ch, cap, device="cuda")
    xc = x.contiguous()
    u, g = r.process_planar_device(xc if frames else None, max(frames, 1), frames, y, cap, cap, 0.0)
    assert u == frames
    _, more = r.process_planar_device(None, 0, -1, y[:, g:], cap, cap - g, 0.0)
    r.synchronize()
    return y[:, :g + more].cpu().numpy()


@pytest.mark.parametrize("max_batch", [1024, 2])
def test_rows_equal_fresh_contexts_on_each_clip_alone(max_batch):
    torch = pytest.importorskip("torch")
    flags = BH | IN | LP
    x = torch.from_numpy((0.25 * np.random.default_rng(11).standard_normal((5, 2, 3000))).astype(np.float32)).cuda()
    clips = A.ClipResampler(2, SRC, DST, T, T, flags, max_batch=max_batch)
    for rnd in range(2):                               # (the second call: the pool's contexts are reset)
        y, out_lengths = clips(x, LENGTHS)
        torch.cuda.synchronize()
        assert y.shape[:2] == (5, 2) and y.shape[2] == int(out_lengths.max()) and out_lengths.tolist()[3] > 0
        for i, n in enumerate(LENGTHS):
            want = alone(x[i, :, :n], n, flags)
            g = int(out_lengths[i])
            assert g == want.shape[1], (rnd, i, g, want.shape)
            assert np.array_equal(y[i, :, :g].cpu().numpy().view(np.uint32), want.view(np.uint32)), (rnd, i)
            assert bool((y[i, :, g:] == 0).all()), (rnd, i)
    assert len(clips.pool) == min(5, max_batch)
    clips.close()


def test_one_clip_without_lengths_and_a_padded_view():
    """[C, T] is a batch of one; a view into a wider tensor is taken as it is (its row pitch, no copy)"""
    torch = pytest.importorskip("torch")
    flags = BH | IN | LP
    wide = torch.from_numpy((0.25 * np.random.default_rng(12).standard_normal((2, 2005))).astype(np.float32)).cuda()
    x = wide[:, 3:1503]
    clips = A.ClipResampler(2, SRC, DST, T, T, flags, max_batch=4)
    y, out_lengths = clips(x)
    torch.cuda.synchronize()
    want = alone(x, 1500, flags)
    assert y.shape == (1, 2, want.shape[1]) and out_lengths.tolist() == [want.shape[1]]
    assert np.array_equal(y[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        clips(x.double())
    clips.close()
