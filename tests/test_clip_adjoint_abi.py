"""CPU: resampleAdjointClipsPlanarDevice — exported by both libraries, declared in art_hip.h with its prototype, listed in
EXPORTED_SYMBOLS and wrapped; n <= 0 and a NULL context are answered without a device and without a count in artamdErrorCount, alike
by this entry and by resampleAdjointScheduleClipsPlanarDevice (the same clips as one block each); the
adjoint kernel's eight instantiations (channel-group widths 1, 2, 4, 8 x interpolating or not) are in both libraries and use no
scratch and no spills; ClipResampler.__call__ still makes its forward call where tests/test_clips_from_start_abi.py looks for it."""
import ctypes as C
import os
import re

import pytest

import audio_resampler_amd as A
from test_matrix_batch_abi import _kernel_notes

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
ADJ = "resampleAdjointClipsPlanarDevice"
BLOCKS = "resampleAdjointScheduleClipsPlanarDevice"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
VARIANTS = [f"fir_adjoint_kernelILi{cg}ELb{interp}EE" for cg in (1, 2, 4, 8) for interp in (0, 1)]


@pytest.mark.parametrize("width", [32, 64])
def test_symbol_is_exported_declared_listed_and_wrapped(width):
    B = A.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    assert ADJ in B.EXPORTED_SYMBOLS and hasattr(B.lib(), ADJ)
    decl = re.search(r"int " + ADJ + r" \(([^;]*)\);", header)
    assert decl, ADJ + " is not declared"
    assert " ".join(decl.group(1).split()) == (
        "Resample *const *cxts, int n, const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames, "
        "artsample_t *const *d_gradInputs, const long *gradInputPitches, const int *numInputFrames, const double *ratios")
    res, argtypes = B.EXPORTED_SYMBOLS[ADJ]
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    assert "ArtAdjItem" not in header and "arthip_fir_adjoint" not in header       # (the record type and the launch stay private)
    for M in (A, B):
        assert callable(M.adjoint_clips_planar_device)


@pytest.mark.parametrize("width", [32, 64])
def test_refusals_need_no_device(width):
    L = A.binding(width).lib()
    adj = getattr(L, ADJ)
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    ints, longs, ratios = (C.c_int * 1)(5), (C.c_long * 1)(0), (C.c_double * 1)(1.0)
    assert adj(None, 0, None, None, None, None, None, None, None) == 0
    assert adj(none, 0, None, None, None, None, None, None, None) == 0
    assert adj(none, -2, none, longs, ints, none, longs, ints, ratios) == 0
    assert adj(none, 1, None, None, None, None, None, None, None) == -1
    assert adj(none, 1, none, longs, ints, none, longs, ints, ratios) == -1
    assert L.artamdErrorCount() == errors


def test_both_entries_answer_nothing_to_do_and_a_null_context_alike():
    """n <= 0 is 0, a NULL context among n is -1 — wherever it stands, with every other argument in order — and neither entry needs a device
    or counts"""
    for width in (32, 64):
        L = A.binding(width).lib()
        errors = L.artamdErrorCount()
        for n in (1, 3):
            none = (C.c_void_p * n)(*[None] * n)
            ints, longs, ratios = (C.c_int * n)(*[5] * n), (C.c_long * n)(*[0] * n), (C.c_double * n)(*[1.0] * n)
            ones = (C.c_int * n)(*[1] * n)
            frames = (C.c_void_p * n)(*[C.addressof(ints) + 4 * i for i in range(n)])
            rates = (C.c_void_p * n)(*[C.addressof(ratios) + 8 * i for i in range(n)])
            for count, want in ((0, 0), (-1, 0), (n, -1)):
                assert getattr(L, ADJ)(none, count, none, longs, ints, none, longs, ints, ratios) == want
                assert getattr(L, BLOCKS)(none, count, ones, none, longs, ints, none, longs, frames, rates) == want
        assert L.artamdErrorCount() == errors


def test_kernel_instantiations_are_in_both_libraries():
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for name in VARIANTS:
            assert name.encode() in blob, (path, name)


@pytest.mark.parametrize("lib", [LIB32, LIB64], ids=["4-byte", "8-byte"])
def test_kernels_use_no_scratch_and_no_spills(tmp_path, monkeypatch, lib):
    import test_matrix_batch_abi
    monkeypatch.setattr(test_matrix_batch_abi, "LIB32", lib)      # (the helper reads the library its module names)
    notes = _kernel_notes(tmp_path)
    adjoint = {s: f for s, f in notes.items() if "fir_adjoint_kernel" in s}
    assert len(adjoint) == len(VARIANTS), sorted(adjoint)
    for s, f in sorted(adjoint.items()):
        print(s, {k: f.get(k) for k in FIELDS})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)


def test_clip_resampler_keeps_its_forward_call_and_gains_the_adjoint():
    code = A.ClipResampler.__call__.__code__
    names = code.co_names + code.co_freevars
    assert "process_and_flush_clips_planar_device" in names and "process_and_flush_batch_planar_device" not in names
    assert "_clip_resample_grad" in names and "requires_grad" in names and "is_grad_enabled" in names
