"""CPU: the three sampling entries — exported by both libraries, declared in art_hip.h with their prototypes, listed in EXPORTED_SYMBOLS of
both widths and wrapped (audio_resampler_amd.sampler); n <= 0 and the refusals that need no device; the wrappers' list checks; the three
kernels are in both libraries without scratch or spills; the new module adds no name to the binding; ClipSampler's host-side refusals on
CPU tensors, before any GPU is asked for."""
import ctypes as C
import json
import os
import re

import pytest

import audio_resampler_amd as A
from audio_resampler_amd import sampler
from test_matrix_batch_abi import _kernel_notes

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
PROTOTYPES = {
    "resampleSampleClipsPlanarDevice": (
        "Resample *const *cxts, int n, "
        "const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames, "
        "const double *const *d_positions, const int *numOutputFrames, "
        "artsample_t *const *d_outputs, const long *outputPitches", 7),
    "resampleSampleAdjointClipsPlanarDevice": (
        "Resample *const *cxts, int n, "
        "const double *const *d_positions, const int *numOutputFrames, "
        "const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, "
        "artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames", 7),
    "resampleSamplePositionGradientClipsPlanarDevice": (
        "Resample *const *cxts, int n, "
        "const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames, "
        "const double *const *d_positions, const int *numOutputFrames, "
        "const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, "
        "double *const *d_gradPositions", 8),
}
WRAPPERS = ("sample_clips_planar_device", "sample_adjoint_clips_planar_device", "sample_position_gradient_clips_planar_device")
KERNELS = ("fir_sample_kernel", "fir_sample_adjoint_kernel", "fir_sample_slope_kernel")


@pytest.mark.parametrize("width", [32, 64])
def test_symbols_are_exported_declared_listed_and_wrapped(width):
    B, S = A.binding(width), sampler.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    for name, (prototype, pointers) in PROTOTYPES.items():
        assert name in B.EXPORTED_SYMBOLS and hasattr(B.lib(), name)
        decl = re.search(r"int " + name + r" \(([^;]*)\);", header)
        assert decl, name + " is not declared"
        assert " ".join(decl.group(1).split()) == prototype
        res, argtypes = B.EXPORTED_SYMBOLS[name]
        assert res is C.c_int and argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * pointers
    assert "ArtSampleItem" not in header and "arthip_fir_sample" not in header
    assert all(callable(getattr(S, w)) for w in WRAPPERS) and isinstance(S.ClipSampler, type) and S.width == width
    if width == 32:
        assert sampler.ClipSampler is S.ClipSampler and all(getattr(sampler, w) is getattr(S, w) for w in WRAPPERS)


@pytest.mark.parametrize("width", [32, 64])
def test_the_module_adds_no_name_to_the_binding(width):
    before = sorted(k for k in vars(A.binding(width)) if not k.startswith("_"))
    sampler.binding(width)
    B = A.binding(width)
    assert sorted(k for k in vars(B) if not k.startswith("_")) == before
    assert not hasattr(B, "ClipSampler") and not any(hasattr(B, w) for w in WRAPPERS)
    assert [k for k in vars(B) if k.startswith("_")] == ["_private"]
    assert sorted(k for k in vars(sampler.binding(width)) if not k.startswith("_")) == sorted(("ClipSampler", "width") + WRAPPERS)


@pytest.mark.parametrize("width", [32, 64])
def test_nothing_to_do_and_refusals_need_no_device(width):
    L = A.binding(width).lib()
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    ints, longs = (C.c_int * 1)(5), (C.c_long * 1)(0)
    for name, (_, pointers) in PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn(None, 0, *[None] * pointers) == 0
        assert fn(none, 0, *[None] * pointers) == 0
        assert fn(none, 1, *[None] * pointers) == -1              # (no lists)
        assert fn(None, 1, *[none] * pointers) == -1              # (no contexts)
    # a NULL context, every list there
    assert L.resampleSampleClipsPlanarDevice(none, -2, none, longs, ints, none, ints, none, longs) == 0
    assert L.resampleSampleClipsPlanarDevice(none, 1, none, longs, ints, none, ints, none, longs) == -1
    assert L.resampleSampleAdjointClipsPlanarDevice(none, 1, none, ints, none, longs, none, longs, ints) == -1
    assert L.resampleSamplePositionGradientClipsPlanarDevice(none, 1, none, longs, ints, none, ints, none, longs, none) == -1
    assert L.artamdErrorCount() == errors
    S = sampler.binding(width)
    assert S.sample_clips_planar_device([], [], None, [], [], [], [], None) == 0
    assert S.sample_adjoint_clips_planar_device([], [], [], [], [], [], [], []) == 0
    assert S.sample_position_gradient_clips_planar_device([], [], None, [], [], [], [], None, []) == 0
    assert L.artamdErrorCount() == errors


class _Ctx:
    """stands for a context in a call that is refused before its address is read"""
    p = None


@pytest.mark.parametrize("width", [32, 64])
def test_wrappers_check_their_lists(width):
    S = sampler.binding(width)
    per_clip = "one entry per clip in every list"
    for call, args in ((S.sample_clips_planar_device, ([_Ctx()], [0], [0], [5], [0], [5, 5], [0], [0])),
                       (S.sample_clips_planar_device, ([_Ctx()], [0, 0], None, [5], [0], [5], [0], None)),
                       (S.sample_adjoint_clips_planar_device, ([_Ctx()], [0], [5], [0], [0], [0], [0], [])),
                       (S.sample_position_gradient_clips_planar_device, ([_Ctx()], [0], [0], [5], [0], [5], [0], [0], [0, 0]))):
        with pytest.raises(ValueError) as e:
            call(*args)
        assert str(e.value) == per_clip
    for call, args, name in ((S.sample_clips_planar_device, ([_Ctx()], [0], None, [5], [0], [5], [0], None), "resampleSampleClipsPlanarDevice"),
                             (S.sample_adjoint_clips_planar_device, ([_Ctx()], [0], [5], [0], [0], [0], [0], [5]), "resampleSampleAdjointClipsPlanarDevice"),
                             (S.sample_position_gradient_clips_planar_device, ([_Ctx()], [0], [0], [5], [0], [5], [0], [0], [0]),
                              "resampleSamplePositionGradientClipsPlanarDevice")):
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
    notes = {s: f for s, f in _kernel_notes(tmp_path).items() if "fir_sample" in s}
    assert len(notes) == len(KERNELS), sorted(notes)
    for s, f in sorted(notes.items()):
        print(s, {k: f.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)
        # (the maps hold nothing in the LDS; the adjoint's chunk of 256 outputs: three ints and two doubles each, gy for four channels, the range)
        sample_bytes = 8 if lib == LIB64 else 4
        assert int(f["group_segment_fixed_size"]) == (256 * (3 * 4 + 2 * 8 + 4 * sample_bytes) + 8 if "adjoint" in s else 0), (s, f)
        assert int(f["vgpr_count"]) <= 128, (s, f)               # (room for four waves per SIMD at least)


ROW_FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def rows_against_the_parents(tmp_path, monkeypatch, width, kernels):
    """the rows of `kernels` in the library of that width against tests/golden/clip_curve_kernel_rows_parent.json (read at the parent commit with
    this same helper): every row is the parent's — registers, LDS bytes, no scratch, no spills"""
    import test_matrix_batch_abi
    monkeypatch.setattr(test_matrix_batch_abi, "LIB32", LIB64 if width == 64 else LIB32)
    notes = _kernel_notes(tmp_path)
    stored = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_curve_kernel_rows_parent.json")))
    assert len(stored["parent_commit"]) == 40 and sorted(stored[str(width)]) == sorted(("fir_sample_kernel", "fir_sample_adjoint_kernel", "fir_sample_slope_kernel",
                                                                                       "fir_band_kernel", "fir_band_adjoint_kernel", "fir_band_slope_kernel"))
    for kernel in kernels:
        (symbol, f), = [(s, f) for s, f in notes.items() if kernel + "E" in s]
        parent = stored[str(width)][kernel]
        got = {k: int(f.get(k, 0)) for k in ROW_FIELDS}
        print(width, kernel, got)
        for k in ("group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            assert got[k] == parent[k] and (k == "group_segment_fixed_size" or got[k] == 0), (symbol, k)
        assert got == parent, symbol


@pytest.mark.parametrize("width", [32, 64])
def test_kernels_keep_the_parent_commits_rows(tmp_path, monkeypatch, width):
    rows_against_the_parents(tmp_path, monkeypatch, width, KERNELS)


@pytest.mark.parametrize("width", [32, 64])
def test_clip_sampler_refuses_on_the_host_before_any_gpu_is_asked_for(width):
    torch = pytest.importorskip("torch")
    S = sampler.binding(width)
    dtype = torch.float64 if width == 64 else torch.float32
    other = torch.float32 if width == 64 else torch.float64
    expected = f"expected a CUDA {'float64' if width == 64 else 'float32'} tensor [B, 2, T]"
    curve = "positions: a float32 or float64 tensor [B, M] or [M]"
    s = S.ClipSampler(2, taps=16, filters=16)
    x, p = torch.zeros(2, 2, 25, dtype=dtype), torch.zeros(2, 7, dtype=torch.float64)
    for bad in (torch.zeros(25, dtype=dtype), torch.zeros(2, 3, 25, dtype=dtype), torch.zeros(2, 2, 25, dtype=other)):
        with pytest.raises(ValueError) as e:                      # (wrong rank, wrong channel count, wrong dtype)
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
        assert str(e.value) == curve
    for bad in ([7], [7, 8], [-1, 7]):
        with pytest.raises(ValueError) as e:
            s(x, p, out_lengths=bad)
        assert str(e.value) == "out_lengths: one entry per clip, 0 .. M"
    for good in (p, torch.zeros(7, dtype=torch.float32), p.clone().requires_grad_()):
        with pytest.raises(ValueError) as e:                      # (everything in order: the samples live on the GPU)
            s(x, good, lengths=[25, 0], out_lengths=[7, 0])
        assert str(e.value) == expected
    assert s.pool == []                                           # (no context was made on the way to a refusal)

    for M in (sampler, sampler.binding(64)):
        with pytest.raises(ValueError) as e:
            M.ClipSampler(2, flags=A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.EXTRAPOLATE_ENDPOINTS)
        assert "EXTRAPOLATE_ENDPOINTS" in str(e.value)
    nearest = S.ClipSampler(2, taps=16, filters=16, flags=A.BLACKMAN_HARRIS | A.INCLUDE_LOWPASS)
    with pytest.raises(ValueError) as e:
        nearest(x, p.clone().requires_grad_())
    assert "SUBSAMPLE_INTERPOLATE" in str(e.value)
    with torch.no_grad():                                         # (without grad mode the tensor is only its values)
        with pytest.raises(ValueError) as e:
            nearest(x, p.clone().requires_grad_())
        assert str(e.value) == expected
    with pytest.raises(ValueError) as e:                          # (a curve that asks for no gradient is the nearest filter's to take)
        nearest(x, p)
    assert str(e.value) == expected
    assert (s.channels, s.taps, nearest.pool) == (2, 16, [])
