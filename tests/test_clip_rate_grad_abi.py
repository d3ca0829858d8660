"""CPU: resampleRateGradientScheduleClipsPlanarDevice — exported by both libraries, declared in art_hip.h with its prototype, listed in
EXPORTED_SYMBOLS of both widths and wrapped (audio_resampler_amd.rate_grad); n <= 0 and the refusals that need no device; the wrapper's
list checks; its two kernels are in both libraries without scratch or spills and with an LDS that is a constant; the new module adds no
name to the binding; ClipRateWarper keeps ClipWarper's front-end refusals on CPU tensors, in their order, and refuses a context that does
not interpolate."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audio_resampler_amd as A
from audio_resampler_amd import rate_grad
from test_matrix_batch_abi import _kernel_notes

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
NAME = "resampleRateGradientScheduleClipsPlanarDevice"
PROTOTYPE = ("Resample *const *cxts, int n, const int *numBlocks, "
             "const artsample_t *const *d_inputs, const long *inputPitches, "
             "const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames, "
             "const int *const *numInputFrames, const double *const *ratios, "
             "double *const *d_gradRatios")
KERNELS = ("fir_rate_grad_tile_kernel", "fir_rate_grad_finish_kernel")


@pytest.mark.parametrize("width", [32, 64])
def test_symbol_is_exported_declared_listed_and_wrapped(width):
    B, R = A.binding(width), rate_grad.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    assert NAME in B.EXPORTED_SYMBOLS and hasattr(B.lib(), NAME)
    decl = re.search(r"int " + NAME + r" \(([^;]*)\);", header)
    assert decl, NAME + " is not declared"
    assert " ".join(decl.group(1).split()) == PROTOTYPE
    res, argtypes = B.EXPORTED_SYMBOLS[NAME]
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 9
    assert "ArtRateItem" not in header and "arthip_fir_rate_grad" not in header
    assert "The ratios get no gradient here: " + NAME in header
    assert callable(R.rate_gradient_schedule_clips_planar_device) and issubclass(R.ClipRateWarper, B.ClipWarper)
    assert R.width == width
    if width == 32:
        assert rate_grad.ClipRateWarper is R.ClipRateWarper
        assert rate_grad.rate_gradient_schedule_clips_planar_device is R.rate_gradient_schedule_clips_planar_device


@pytest.mark.parametrize("width", [32, 64])
def test_the_module_adds_no_name_to_the_binding(width):
    before = sorted(k for k in vars(A.binding(width)) if not k.startswith("_"))
    rate_grad.binding(width)
    B = A.binding(width)
    assert sorted(k for k in vars(B) if not k.startswith("_")) == before
    assert not hasattr(B, "ClipRateWarper") and not hasattr(B, "rate_gradient_schedule_clips_planar_device")
    assert [k for k in vars(B) if k.startswith("_")] == ["_private"]             # (the helpers, under one attribute)
    for helper in ("_clip_input", "_clip_ptrs", "_pool_ready", "_grad_function", "_clip_backward", "_rows_readable"):
        assert callable(getattr(B._private, helper))
    assert sorted(k for k in vars(rate_grad.binding(width)) if not k.startswith("_")) == ["ClipRateWarper", "rate_gradient_schedule_clips_planar_device", "width"]


@pytest.mark.parametrize("width", [32, 64])
def test_nothing_to_do_and_refusals_need_no_device(width):
    L = A.binding(width).lib()
    fn = getattr(L, NAME)
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    ints, longs = (C.c_int * 1)(1), (C.c_long * 1)(0)
    frames, rates = (C.c_int * 1)(5), (C.c_double * 1)(1.0)
    rows = lambda a: (C.c_void_p * 1)(C.cast(a, C.c_void_p))
    assert fn(None, 0, None, None, None, None, None, None, None, None, None) == 0
    assert fn(none, 0, None, None, None, None, None, None, None, None, None) == 0
    assert fn(none, -2, ints, none, longs, none, longs, ints, rows(frames), rows(rates), none) == 0
    assert fn(none, 1, None, None, None, None, None, None, None, None, None) == -1
    assert fn(none, 1, ints, none, longs, none, longs, ints, rows(frames), rows(rates), none) == -1      # (a NULL context)
    assert fn(None, 1, ints, none, longs, none, longs, ints, rows(frames), rows(rates), none) == -1
    assert L.artamdErrorCount() == errors
    R = rate_grad.binding(width)
    assert R.rate_gradient_schedule_clips_planar_device([], [], [], [], [], [], [], [], []) == 0
    assert R.rate_gradient_schedule_clips_planar_device([], [], None, [], None, [], [], [], []) == 0
    assert L.artamdErrorCount() == errors


class _Ctx:
    """stands for a context in a call that is refused before its address is read"""
    p = None


@pytest.mark.parametrize("width", [32, 64])
def test_wrapper_checks_its_lists(width):
    call = rate_grad.binding(width).rate_gradient_schedule_clips_planar_device
    per_clip, per_block = "one entry per clip in every list", "n_ins[i] and ratios[i] must have one entry per block"
    for args, message in ((([_Ctx()], [0], [0], [0], [0], [5, 5], [[1]], [[1.0]], [0]), per_clip),
                          (([_Ctx()], [0, 0], [0], [0], [0], [5], [[1]], [[1.0]], [0]), per_clip),
                          (([_Ctx()], [0], [0], [0], [0], [5], [[1]], [[1.0]], []), per_clip),
                          (([_Ctx()], [0], [0], [0], [0], [5], [[1]], [], [0]), per_clip),
                          (([_Ctx()], [0], [0], [0], [0], [5], [[1, 1]], [[1.0]], [0]), per_block),
                          (([_Ctx()], [0], [0], [0], [0], [5], [[]], [[1.0]], [0]), per_block)):
        with pytest.raises(ValueError) as e:
            call(*args)
        assert str(e.value) == message
    with pytest.raises(RuntimeError) as e:                      # (a NULL context: the entry's own refusal, raised)
        call([_Ctx()], [0], [0], [0], [0], [5], [[1]], [[1.0]], [0])
    assert str(e.value) == NAME + " failed"


def test_kernels_are_in_both_libraries():
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for name in KERNELS:
            assert name.encode() in blob, (path, name)


@pytest.mark.parametrize("lib", [LIB32, LIB64], ids=["4-byte", "8-byte"])
def test_kernels_use_no_scratch_no_spills_and_a_constant_lds(tmp_path, monkeypatch, lib):
    import test_matrix_batch_abi
    monkeypatch.setattr(test_matrix_batch_abi, "LIB32", lib)      # (the helper reads the library its module names)
    notes = {s: f for s, f in _kernel_notes(tmp_path).items() if "fir_rate_grad" in s}
    assert len(notes) == len(KERNELS), sorted(notes)
    for s, f in sorted(notes.items()):
        print(s, {k: f.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)
        # (the wave sums of a pair; 64 phases' S0 and gradient: nothing that grows with the ratio, the block count or the clip)
        assert int(f["group_segment_fixed_size"]) == (64 if "tile" in s else 1024), (s, f)
        assert int(f["vgpr_count"]) <= 128, (s, f)               # (room for four waves per SIMD at least)


@pytest.mark.parametrize("width", [32, 64])
def test_clip_rate_warper_keeps_the_front_end_refusals_in_their_order(width):
    torch = pytest.importorskip("torch")
    R = rate_grad.binding(width)
    dtype = torch.float64 if width == 64 else torch.float32
    other = torch.float32 if width == 64 else torch.float64
    expected = f"expected a CUDA {'float64' if width == 64 else 'float32'} tensor [B, 2, T]"
    shape = "ratios: a scalar, [B] or [B, K] with K >= ceil(max(lengths) / block)"
    lengths_message = "lengths: one entry per clip, 0 .. T"
    w = R.ClipRateWarper(2, taps=16, filters=16, block=10)
    grad = lambda *s: torch.ones(*s, dtype=torch.float64, requires_grad=True)
    x = torch.zeros(2, 2, 25, dtype=dtype)
    for ratios in (1.0, np.ones((2, 3)), torch.ones(2, 3), grad(2, 3), grad(2), grad(())):
        # the shape and dtype of x first, then the lengths, then the ratios, then the GPU
        for bad in (torch.zeros(25, dtype=dtype), torch.zeros(2, 3, 25, dtype=dtype), torch.zeros(2, 2, 25, dtype=other)):
            with pytest.raises(ValueError) as e:
                w(bad, ratios)
            assert str(e.value) == expected
        for bad in ([25], [25, 26], [-1, 25]):
            with pytest.raises(ValueError) as e:
                w(x, ratios, lengths=bad)
            assert str(e.value) == lengths_message
        with pytest.raises(ValueError) as e:                      # (good lengths, good ratios: the samples live on the GPU)
            w(x, ratios, lengths=[25, 0])
        assert str(e.value) == expected
    for ratios, lengths, message in ((grad(2, 2), None, shape), (grad(3, 3), None, shape), (grad(3), None, shape), (grad(2, 2), [20, 3], expected),
                                     (grad(2, 3), [25, 26], lengths_message),
                                     (torch.tensor([1.0, 0.0], dtype=torch.float64, requires_grad=True), None, "ratios must be finite and > 0"),
                                     (torch.tensor(float("nan"), requires_grad=True), None, "ratios must be finite and > 0"),
                                     (torch.ones(2, 3, dtype=torch.float16, requires_grad=True), None, "ratios that require grad: a float32 or float64 tensor")):
        with pytest.raises(ValueError) as e:
            w(x, ratios, lengths=lengths)
        assert str(e.value) == message, (tuple(ratios.shape), lengths)
    for ratios in (1.0, grad(())):                                # (no clip: still a CPU tensor)
        with pytest.raises(ValueError) as e:
            w(torch.zeros(0, 2, 25, dtype=dtype), ratios)
        assert str(e.value) == expected
    with torch.no_grad():                                         # (without grad mode the tensor is only its values)
        with pytest.raises(ValueError) as e:
            w(x, grad(2, 3))
        assert str(e.value) == expected
    assert w.pool == []                                           # (no context was made on the way to a refusal)


def test_clip_rate_warper_checks_its_construction():
    for M in (rate_grad, rate_grad.binding(64)):
        with pytest.raises(ValueError) as e:
            M.ClipRateWarper(2, flags=A.BLACKMAN_HARRIS | A.INCLUDE_LOWPASS)
        assert "SUBSAMPLE_INTERPOLATE" in str(e.value)
        with pytest.raises(ValueError):
            M.ClipRateWarper(2, flags=A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.EXTRAPOLATE_ENDPOINTS)
        with pytest.raises(ValueError):
            M.ClipRateWarper(2, block=0)
        w = M.ClipRateWarper(2, taps=16, filters=16, block=10, max_batch=3)
        assert (w.channels, w.taps, w.block, w.max_batch, w.pool) == (2, 16, 10, 3, [])
        assert w.blocks([25, 0, 10], [[1.0, 2.0, 3.0], [0.5, -1.0, -1.0], [0.25, float("nan"), 0.0]]) == ([[10, 10, 5], [0], [10]], [[1.0, 2.0, 3.0], [0.5], [0.25]])
