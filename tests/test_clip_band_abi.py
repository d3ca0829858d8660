"""CPU: the three banded sampling entries — exported by both libraries, declared in art_hip.h with their prototypes, listed in
EXPORTED_SYMBOLS of both widths and wrapped (audio_resampler_amd.band); n <= 0 and the refusals that need no device; the wrappers' list
checks; the three kernels are in both libraries without scratch or spills; the new module adds no name to the binding or to the sampler's
namespace; ClipBandSampler's host-side refusals on CPU tensors, before any GPU is asked for; levels_of on CPU tensors against the numpy
restatement of tests/_band_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audio_resampler_amd as A
from audio_resampler_amd import band, sampler
import _band_ref as BR
from test_matrix_batch_abi import _kernel_notes
from test_clip_sampler_abi import rows_against_the_parents

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
PROTOTYPES = {
    "resampleSampleBandClipsPlanarDevice": (
        "Resample *const *cxts, int n, int numRungs, "
        "const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames, "
        "const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames, "
        "artsample_t *const *d_outputs, const long *outputPitches", 8),
    "resampleSampleBandAdjointClipsPlanarDevice": (
        "Resample *const *cxts, int n, int numRungs, "
        "const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames, "
        "const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, "
        "artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames", 8),
    "resampleSampleBandGradientsClipsPlanarDevice": (
        "Resample *const *cxts, int n, int numRungs, "
        "const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames, "
        "const double *const *d_positions, const double *const *d_levels, const int *numOutputFrames, "
        "const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, "
        "double *const *d_gradPositions, double *const *d_gradLevels", 10),
}
WRAPPERS = ("sample_band_clips_planar_device", "sample_band_adjoint_clips_planar_device", "sample_band_gradients_clips_planar_device")
KERNELS = ("fir_band_kernel", "fir_band_adjoint_kernel", "fir_band_slope_kernel")
DEFAULT = (1.0, 2 ** -0.5, 0.5, 2 ** -1.5, 0.25)


@pytest.mark.parametrize("width", [32, 64])
def test_symbols_are_exported_declared_listed_and_wrapped(width):
    B, S = A.binding(width), band.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    for name, (prototype, pointers) in PROTOTYPES.items():
        assert name in B.EXPORTED_SYMBOLS and hasattr(B.lib(), name)
        decl = re.search(r"int " + name + r" \(([^;]*)\);", header)
        assert decl, name + " is not declared"
        assert " ".join(decl.group(1).split()) == prototype
        res, argtypes = B.EXPORTED_SYMBOLS[name]
        assert res is C.c_int and argtypes == [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * pointers
    assert "ArtBandItem" not in header and "arthip_fir_band" not in header
    assert all(callable(getattr(S, w)) for w in WRAPPERS) and isinstance(S.ClipBandSampler, type) and S.width == width
    if width == 32:
        assert band.ClipBandSampler is S.ClipBandSampler and all(getattr(band, w) is getattr(S, w) for w in WRAPPERS)


@pytest.mark.parametrize("width", [32, 64])
def test_the_module_adds_no_name_to_the_binding_or_to_the_sampler(width):
    before = sorted(k for k in vars(A.binding(width)) if not k.startswith("_"))
    before_sampler = sorted(vars(sampler.binding(width)))
    band.binding(width)
    B = A.binding(width)
    assert sorted(k for k in vars(B) if not k.startswith("_")) == before and sorted(vars(sampler.binding(width))) == before_sampler
    assert not hasattr(B, "ClipBandSampler") and not any(hasattr(B, w) or hasattr(sampler.binding(width), w) for w in WRAPPERS)
    assert [k for k in vars(B) if k.startswith("_")] == ["_private"]
    assert sorted(k for k in vars(band.binding(width)) if not k.startswith("_")) == sorted(("ClipBandSampler", "width") + WRAPPERS)


@pytest.mark.parametrize("width", [32, 64])
def test_nothing_to_do_and_refusals_need_no_device(width):
    L = A.binding(width).lib()
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 8)(*[None] * 8)
    ints, longs = (C.c_int * 1)(5), (C.c_long * 1)(0)
    for name, (_, pointers) in PROTOTYPES.items():
        fn = getattr(L, name)
        for rungs in (0, 1, 5, 9):
            assert fn(None, 0, rungs, *[None] * pointers) == 0
            assert fn(none, -3, rungs, *[none] * pointers) == 0
        assert fn(none, 1, 1, *[None] * pointers) == -1           # (no lists)
        assert fn(None, 1, 1, *[none] * pointers) == -1           # (no contexts)
        for rungs in (-1, 0, 9, 2 ** 31 - 1):                     # (the ladder's size comes first: no context is looked at)
            assert fn(none, 1, rungs, *[none] * pointers) == -1
        for rungs in (1, 2, 8):                                   # (a NULL context among the rungs, every list there)
            assert fn(none, 1, rungs, *[none] * pointers) == -1
    assert L.resampleSampleBandClipsPlanarDevice(none, 1, 2, none, longs, ints, none, none, ints, none, longs) == -1
    assert L.resampleSampleBandAdjointClipsPlanarDevice(none, 1, 2, none, none, ints, none, longs, none, longs, ints) == -1
    assert L.resampleSampleBandGradientsClipsPlanarDevice(none, 1, 2, none, longs, ints, none, none, ints, none, longs, none, none) == -1
    assert L.resampleSampleBandGradientsClipsPlanarDevice(none, 1, 2, none, longs, ints, none, none, ints, none, longs, None, None) == -1
    assert L.artamdErrorCount() == errors
    S = band.binding(width)
    assert S.sample_band_clips_planar_device([], 3, [], None, [], [], [], [], [], None) == 0
    assert S.sample_band_adjoint_clips_planar_device([], 3, [], [], [], [], [], [], [], []) == 0
    assert S.sample_band_gradients_clips_planar_device([], 3, [], None, [], [], [], [], [], None, [], None) == 0
    assert L.artamdErrorCount() == errors


class _Ctx:
    """stands for a context in a call that is refused before its address is read"""
    p = None


@pytest.mark.parametrize("width", [32, 64])
def test_wrappers_check_their_lists(width):
    S = band.binding(width)
    per_clip = "one entry per clip in every list"
    two = [_Ctx(), _Ctx()]
    for call, args in ((S.sample_band_clips_planar_device, (two, 2, [0], [0], [5], [0], [0], [5, 5], [0], [0])),
                       (S.sample_band_clips_planar_device, (two, 2, [0], None, [5], [0], [0, 0], [5], [0], None)),
                       (S.sample_band_clips_planar_device, (two, 1, [0], None, [5], [0], [0], [5], [0], None)),     # (two clips of one rung: one entry each)
                       (S.sample_band_adjoint_clips_planar_device, (two, 2, [0], [0], [5], [0], [0], [0], [0], [])),
                       (S.sample_band_gradients_clips_planar_device, (two, 2, [0], [0], [5], [0], [0], [5], [0], [0], [0, 0], None)),
                       (S.sample_band_gradients_clips_planar_device, (two, 2, [0], [0], [5], [0], [0], [5], [0], [0], None, []))):
        with pytest.raises(ValueError) as e:
            call(*args)
        assert str(e.value) == per_clip
    for rungs in (0, -1, 3):                                      # (a ladder that does not divide the contexts)
        with pytest.raises(ValueError) as e:
            S.sample_band_clips_planar_device(two, rungs, [0], None, [5], [0], [0], [5], [0], None)
        assert str(e.value) == "resamplers: rungs contexts per clip"
    for call, args, name in ((S.sample_band_clips_planar_device, (two, 2, [0], None, [5], [0], [0], [5], [0], None), "resampleSampleBandClipsPlanarDevice"),
                             (S.sample_band_adjoint_clips_planar_device, (two, 2, [0], [0], [5], [0], [0], [0], [0], [5]),
                              "resampleSampleBandAdjointClipsPlanarDevice"),
                             (S.sample_band_gradients_clips_planar_device, (two, 2, [0], [0], [5], [0], [0], [5], [0], [0], [0], [0]),
                              "resampleSampleBandGradientsClipsPlanarDevice"),
                             (S.sample_band_gradients_clips_planar_device, (two, 2, [0], [0], [5], [0], [0], [5], [0], [0], None, None),
                              "resampleSampleBandGradientsClipsPlanarDevice")):
        with pytest.raises(RuntimeError) as e:                    # (a NULL context: the entry's own refusal, raised)
            call(*args)
        assert str(e.value) == name + " failed"


def test_kernels_are_in_both_libraries():
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for name in KERNELS:
            assert name.encode() in blob, (path, name)


@pytest.mark.parametrize("lib", [LIB32, LIB64], ids=["4-byte", "8-byte"])
def test_kernels_use_no_scratch_no_spills_and_a_constant_lds(tmp_path, monkeypatch, lib):
    import test_matrix_batch_abi
    monkeypatch.setattr(test_matrix_batch_abi, "LIB32", lib)      # (the helper reads the library its module names)
    notes = {s: f for s, f in _kernel_notes(tmp_path).items() if "fir_band" in s}
    assert len(notes) == len(KERNELS) and all(any(k + "E" in s for s in notes) for k in KERNELS), sorted(notes)
    for s, f in sorted(notes.items()):
        print(s, {k: f.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)
        # (the maps hold nothing in the LDS; the adjoint's chunk of 256 outputs: three ints and three doubles each — the sampler's rows with
        # the rung in the pass-through's place, and the blend — gy for four channels, the range)
        sample_bytes = 8 if lib == LIB64 else 4
        assert int(f["group_segment_fixed_size"]) == (256 * (3 * 4 + 3 * 8 + 4 * sample_bytes) + 8 if "adjoint" in s else 0), (s, f)
        assert int(f["vgpr_count"]) <= 128, (s, f)               # (room for four waves per SIMD at least)


@pytest.mark.parametrize("width", [32, 64])
def test_kernels_keep_the_parent_commits_rows(tmp_path, monkeypatch, width):
    """(the banded maps' 128 VGPRs at most are held by the test above)"""
    rows_against_the_parents(tmp_path, monkeypatch, width, KERNELS)


@pytest.mark.parametrize("width", [32, 64])
def test_clip_band_sampler_refuses_on_the_host_before_any_gpu_is_asked_for(width):
    torch = pytest.importorskip("torch")
    S = band.binding(width)
    dtype = torch.float64 if width == 64 else torch.float32
    other = torch.float32 if width == 64 else torch.float64
    expected = f"expected a CUDA {'float64' if width == 64 else 'float32'} tensor [B, 2, T]"
    s = S.ClipBandSampler(2, (1.0, 0.5), taps=16, filters=16)
    x, p = torch.zeros(2, 2, 25, dtype=dtype), torch.zeros(2, 7, dtype=torch.float64)
    for bad in (torch.zeros(25, dtype=dtype), torch.zeros(2, 3, 25, dtype=dtype), torch.zeros(2, 2, 25, dtype=other)):
        with pytest.raises(ValueError) as e:
            s(bad, p)
        assert str(e.value) == expected
    for bad in ([25], [25, 26], [-1, 25]):
        with pytest.raises(ValueError) as e:
            s(x, p, lengths=bad)
        assert str(e.value) == "lengths: one entry per clip, 0 .. T"
    for bad in (torch.zeros(2, 7, 1, dtype=torch.float64), torch.zeros((), dtype=torch.float64), torch.zeros(3, 7, dtype=torch.float64),
                torch.zeros(2, 7, dtype=torch.float16), torch.zeros(2, 7, dtype=torch.int64), [[0.0] * 7] * 2):
        with pytest.raises(ValueError) as e:
            s(x, bad)
        assert str(e.value) == "positions: a float32 or float64 tensor [B, M] or [M]"
        if not torch.is_tensor(bad) or bad.shape != (3, 7):       # (three rows are as good a curve as any, on their own)
            with pytest.raises(ValueError):
                s.levels_of(bad)
    for bad in ([7], [7, 8], [-1, 7]):
        with pytest.raises(ValueError) as e:
            s(x, p, out_lengths=bad)
        assert str(e.value) == "out_lengths: one entry per clip, 0 .. M"
    for bad in (torch.zeros(2, 6, dtype=torch.float64), torch.zeros(6, dtype=torch.float64), torch.zeros(3, 7, dtype=torch.float64),
                torch.zeros(2, 7, 1, dtype=torch.float64), torch.zeros(2, 7, dtype=torch.int32), [0.0] * 7, 1.5):
        with pytest.raises(ValueError) as e:
            s(x, p, bad)
        assert str(e.value) == "levels: a float32 or float64 tensor [B, M] or [M], or None"
    for good in (None, p.clone(), torch.zeros(7, dtype=torch.float32), p.clone().requires_grad_()):
        with pytest.raises(ValueError) as e:                      # (everything in order: the samples live on the GPU)
            s(x, p, good, lengths=[25, 0], out_lengths=[7, 0])
        assert str(e.value) == expected
    assert s.pool == []                                           # (no context was made on the way to a refusal)

    IN, LP, BH = A.SUBSAMPLE_INTERPOLATE, A.INCLUDE_LOWPASS, A.BLACKMAN_HARRIS
    for M in (band, band.binding(64)):
        with pytest.raises(ValueError) as e:
            M.ClipBandSampler(2, flags=BH | IN | A.EXTRAPOLATE_ENDPOINTS)
        assert "EXTRAPOLATE_ENDPOINTS" in str(e.value)
        with pytest.raises(ValueError) as e:
            M.ClipBandSampler(2, flags=BH | LP)
        assert "SUBSAMPLE_INTERPOLATE" in str(e.value)
        for bad in ((), (1.0,) * 2, (0.5, 1.0), (1.0, 0.5, 0.5), (1.5, 1.0), (1.0, 0.0), (1.0, -0.5), (1.0, float("nan")),
                    tuple(2.0 ** -k for k in range(9)), 0.5):
            with pytest.raises(ValueError) as e:
                M.ClipBandSampler(2, bad)
            assert str(e.value) == "cutoffs: 1 to 8 cut-offs in (0, 1], strictly decreasing"
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError) as e:
                M.ClipBandSampler(2, guard=bad)
            assert str(e.value).startswith("guard")
        ok = M.ClipBandSampler(2, tuple(2.0 ** -k for k in range(8)))
        assert len(ok.cutoffs) == 8 and ok.pool == [] and M.ClipBandSampler(2).cutoffs == DEFAULT and M.ClipBandSampler(3, [0.7]).cutoffs == (0.7,)


# a log is good to an ulp or two of a value below ln 8: a term of the sum to 2^-49 or so over ln c_k - ln c_{k+1} >= 0.34 of these ladders;
# seven terms stay far inside 2^-44
LEVEL_TOLERANCE = 2.0 ** -44


def test_levels_of_on_cpu_tensors_is_the_numpy_restatement():
    torch = pytest.importorskip("torch")
    s = band.ClipBandSampler(2)
    want = {0.5: 0.0, 1.0: 0.0, 1.5: 2 * np.log2(1.5), 2.0: 2.0, 3.0: 2 * np.log2(3.0), 5.0: 4.0}
    for step, level in want.items():
        got = s.levels_of(torch.arange(9, dtype=torch.float64) * step + 0.25)
        assert got.shape == (1, 9) and got.dtype == torch.float64 and not got.requires_grad
        assert np.all(np.abs(got.numpy() - level) <= LEVEL_TOLERANCE), (step, got)
        assert np.all(np.abs(BR.auto_levels(np.arange(9) * step + 0.25, 9, DEFAULT) - level) <= LEVEL_TOLERANCE)
    assert abs(want[1.5] - 1.1699250014423124) < 1e-15 and abs(want[3.0] - 3.1699250014423126) < 1e-15
    rng = np.random.default_rng(12)
    M = 40
    ph = np.stack([np.cumsum(rng.uniform(0.2, 6.0, M)), 80.0 - np.cumsum(rng.uniform(0.2, 3.0, M)), 1.7 * np.arange(M)])
    ph[2, 11], ph[2, 30] = np.nan, np.inf                       # (their neighbours' steps are not finite: NaN levels; their own are)
    outs = [M, 1, 33]
    for guard, cutoffs in ((1.0, DEFAULT), (0.8, DEFAULT), (1.0, (1.0, 0.3)), (1.0, (0.9,)), (2.0, (0.5, 0.4, 0.1))):
        t = band.ClipBandSampler(2, cutoffs, guard=guard)
        p = torch.from_numpy(ph).requires_grad_()
        got = t.levels_of(p, outs)
        assert got.shape == (3, M) and not got.requires_grad
        for i, n in enumerate(outs):
            ref = BR.auto_levels(ph[i], n, cutoffs, guard)
            assert np.array_equal(np.isnan(got[i].numpy()), np.isnan(ref)) and not np.any(got[i, n:].numpy())
            assert np.all(np.abs(np.nan_to_num(got[i].numpy()) - np.nan_to_num(ref)) <= LEVEL_TOLERANCE), (guard, cutoffs, i)
        assert np.isnan(got[2].numpy()).tolist() == [m in (10, 12, 29, 31) for m in range(M)]
        # a single output: a step of 1, whose level is 0 unless the guard asks for less than the full band
        assert abs(float(got[1, 0]) - BR.auto_levels(np.array([5.0]), 1, cutoffs, guard)[0]) <= LEVEL_TOLERANCE and (guard < 1.0 or float(got[1, 0]) == 0.0)
        # the two ends are one-sided
        one_sided = BR.auto_levels(ph[0, :2], 2, cutoffs, guard)
        assert abs(float(got[0, 0]) - one_sided[0]) <= LEVEL_TOLERANCE
    # a curve for every clip, float32, out_lengths giving B
    shared = s.levels_of(torch.from_numpy(ph[0].astype(np.float32)), [M, 7])
    assert shared.shape == (2, M) and torch.equal(shared[0, :6], shared[1, :6]) and not bool(shared[1, 7:].any())
    assert np.all(np.abs(shared[0].numpy() - BR.auto_levels(ph[0].astype(np.float32).astype(np.float64), M, DEFAULT)) <= LEVEL_TOLERANCE)
    assert s.levels_of(torch.zeros(0, dtype=torch.float64)).shape == (1, 0) and s.pool == []
