"""The cases of tests/golden/clip_adjoint_parent_bits.npz — resampleAdjointClipsPlanarDevice's results at the commit the file names, kept
so that any later merging of the two adjoint kernels (fir_adjoint.hip: the two-phase kernel and the blocks kernel) has bits to reproduce —
shared by the generator (tests/golden/make_golden_clip_adjoint.py) and the test that holds both adjoint entries to those bits
(tests/test_gpu_clip_adjoint_bits.py).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import audio_resampler_amd as A
import _warp_ref as W

BH, IN, LP = A.BLACKMAN_HARRIS, A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS
DOWN = (44100.0, 16000.0, 0)
SEED = 33
# (name, sample width, channels, taps, filters, flags, fixed rates or None, ratio or None, clip lengths)
CASES = [
    # tests/test_gpu_clip_warp.py's ONE_BLOCK rows
    ("44100-16000", 32, 2, 380, 380, BH | IN | LP, DOWN, None, (700, 1, 257, 189)),
    ("16000-44100", 32, 2, 380, 380, BH | IN | LP, (16000.0, 44100.0, 0), None, (700, 1, 257, 189)),
    ("any-ratio-1.1", 32, 2, 380, 380, BH | IN | LP, None, 1.1, (700, 1, 257, 189)),
    ("nearest-filter", 32, 2, 32, 8, BH | LP, (3.0, 2.0, 0), None, (700, 1, 257, 189)),
    ("pass-through", 32, 2, 32, 8, BH, (2.0, 3.0, 0), None, (700, 1, 257, 189)),
    # every channel-group width (1, 2 above, 4, 8) and a partial group (3 of 4; 9: a full group of 8 and 1 of the next)
    ("44100-16000-1ch", 32, 1, 380, 380, BH | IN | LP, DOWN, None, (600, 1)),
    ("44100-16000-3ch", 32, 3, 380, 380, BH | IN | LP, DOWN, None, (600, 1)),
    ("44100-16000-9ch", 32, 9, 380, 380, BH | IN | LP, DOWN, None, (600, 1)),
    ("44100-16000-8-byte", 64, 2, 380, 380, BH | IN | LP, DOWN, None, (700, 1, 257, 189)),
]


def gradients(case):
    """(the ratio to pass, output frames of every clip, gy_i [channels, M_i] in the build's sample type): normal noise, seed 33"""
    _, width, channels, taps, filters, flags, fixed, ratio, lengths = case
    r = ratio if ratio is not None else 1.0                       # (a fixed-ratio context ignores it)
    Ms = [W.output_count(taps, filters, flags, (n,), (r,), fixed=fixed) for n in lengths]
    rng = np.random.default_rng(SEED)
    smp = np.float64 if width == 64 else np.float32
    return r, Ms, [(0.25 * rng.standard_normal((channels, m))).astype(np.float32).astype(smp) for m in Ms]


def run(case, blocks):
    """the case's clips in one call — blocks False: resampleAdjointClipsPlanarDevice on the clips as given; True:
    resampleAdjointScheduleClipsPlanarDevice on each as one block -> (launches, [gx_i [channels, N_i]])"""
    import torch
    _, width, channels, taps, filters, flags, fixed, _, lengths = case
    B = A.binding(width)
    r, Ms, gys = gradients(case)
    ctx = B.Resampler(channels, taps, filters, 0.0, flags, fixed)
    d_gy = [torch.from_numpy(g).cuda() for g in gys]
    d_gx = [torch.full((channels, n), -777.25, dtype=d_gy[0].dtype, device="cuda") for n in lengths]
    pitch = lambda frames: [v if channels > 1 else 0 for v in frames]
    k = len(lengths)
    if blocks:
        launches = B.adjoint_schedule_clips_planar_device([ctx] * k, d_gy, pitch(Ms), Ms, d_gx, pitch(lengths), [[n] for n in lengths], [[r]] * k)
    else:
        launches = B.adjoint_clips_planar_device([ctx] * k, d_gy, pitch(Ms), Ms, d_gx, pitch(lengths), list(lengths), [r] * k)
    torch.cuda.synchronize()
    ctx.close()
    return launches, [x.cpu().numpy() for x in d_gx]
