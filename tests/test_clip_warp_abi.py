"""CPU: resampleProcessScheduleClipsPlanarDevice and resampleAdjointScheduleClipsPlanarDevice — exported by both libraries, declared in
art_hip.h with their prototypes, listed in EXPORTED_SYMBOLS and wrapped; their refusals are answered without a device and without a
count in artamdErrorCount; the blocks adjoint kernel's eight instantiations (channel-group widths 1, 2, 4, 8 x interpolating or not) are
in both libraries and use no scratch and no spills; ClipWarper checks its arguments before it needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audio_resampler_amd as A
from test_matrix_batch_abi import _kernel_notes

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
FWD, ADJ = "resampleProcessScheduleClipsPlanarDevice", "resampleAdjointScheduleClipsPlanarDevice"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
VARIANTS = [f"fir_adjoint_blocks_kernelILi{cg}ELb{interp}EE" for cg in (1, 2, 4, 8) for interp in (0, 1)]
PROTOTYPES = {
    FWD: "Resample *const *cxts, int n, const int *numBlocks, "
         "const artsample_t *const *d_inputs, const long *inputPitches, const int *const *numInputFrames, "
         "artsample_t *const *d_outputs, const long *outputPitches, const int *const *numOutputFrames, "
         "const double *const *ratios, const int *flushLast, int fromStart, "
         "ResampleResult *const *results, int *blocksMade",
    ADJ: "Resample *const *cxts, int n, const int *numBlocks, "
         "const artsample_t *const *d_gradOutputs, const long *gradOutputPitches, const int *numOutputFrames, "
         "artsample_t *const *d_gradInputs, const long *gradInputPitches, "
         "const int *const *numInputFrames, const double *const *ratios",
}


@pytest.mark.parametrize("width", [32, 64])
def test_symbols_are_exported_declared_listed_and_wrapped(width):
    B = A.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    for name, want in PROTOTYPES.items():
        assert name in B.EXPORTED_SYMBOLS and hasattr(B.lib(), name)
        decl = re.search(r"int " + name + r" \(([^;]*)\);", header)
        assert decl, name + " is not declared"
        assert " ".join(decl.group(1).split()) == want
    res, argtypes = B.EXPORTED_SYMBOLS[FWD]
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 9 + [C.c_int] + [C.c_void_p] * 2
    res, argtypes = B.EXPORTED_SYMBOLS[ADJ]
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 8
    assert "ArtAdjBlocksItem" not in header and "ArtAdjPhase" not in header and "arthip_fir_adjoint_blocks" not in header
    for M in (A, B):
        assert callable(M.process_schedule_clips_planar_device) and callable(M.adjoint_schedule_clips_planar_device)
        assert isinstance(M.ClipWarper, type)


@pytest.mark.parametrize("width", [32, 64])
def test_refusals_need_no_device(width):
    L = A.binding(width).lib()
    fwd, adj = getattr(L, FWD), getattr(L, ADJ)
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    ints, longs = (C.c_int * 1)(1), (C.c_long * 1)(0)
    frames, rates = (C.c_int * 1)(5), (C.c_double * 1)(1.0)
    rows = lambda a: (C.c_void_p * 1)(C.cast(a, C.c_void_p))
    res, made = (C.c_uint * 2)(), (C.c_int * 1)(7)
    # the adjoint: nothing to do, then a NULL context (with and without the other arrays)
    assert adj(None, 0, None, None, None, None, None, None, None, None) == 0
    assert adj(none, 0, None, None, None, None, None, None, None, None) == 0
    assert adj(none, -2, ints, none, longs, ints, none, longs, rows(frames), rows(rates)) == 0
    assert adj(none, 1, None, None, None, None, None, None, None, None) == -1
    assert adj(none, 1, ints, none, longs, ints, none, longs, rows(frames), rows(rates)) == -1
    # the forward entry: nothing to do, then a NULL context, from a fresh start or not (refused before any reset)
    for from_start in (0, 1):
        assert fwd(none, 0, ints, none, longs, rows(frames), none, longs, rows(frames), rows(rates), None, from_start, rows(res), made) == 0
        assert fwd(none, 1, ints, none, longs, rows(frames), none, longs, rows(frames), rows(rates), None, from_start, rows(res), made) == -1
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
    blocks = {s: f for s, f in notes.items() if "fir_adjoint_blocks_kernel" in s}
    assert len(blocks) == len(VARIANTS), sorted(blocks)
    for s, f in sorted(blocks.items()):
        print(s, {k: f.get(k) for k in FIELDS})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)
        assert int(f["group_segment_fixed_size"]) <= 24 * 1024, (s, f)      # (independent of the block count: a fixed phase table)


def test_clip_warper_checks_its_arguments_without_a_gpu():
    torch = pytest.importorskip("torch")
    with pytest.raises(ValueError):
        A.ClipWarper(2, flags=A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE | A.EXTRAPOLATE_ENDPOINTS)
    with pytest.raises(ValueError):
        A.ClipWarper(2, block=0)
    w = A.ClipWarper(2, taps=16, filters=16, block=10)
    assert w.pool == []                                           # (no context before the first call)
    x = torch.zeros(2, 2, 25)
    for bad in (0.0, -1.0, float("nan"), float("inf"), [1.0, 0.0], [[1.0, 1.0, -2.0], [1.0, 1.0, 1.0]]):
        with pytest.raises(ValueError):
            w(x, bad)
    with pytest.raises(ValueError):                               # (K < ceil (25 / 10))
        w(x, np.ones((2, 2)))
    with pytest.raises(ValueError):                               # (one row per clip)
        w(x, np.ones((3, 3)))
    with pytest.raises(ValueError):                               # (no silent zero gradient for the ratio curve)
        w(x, torch.ones(2, 3, requires_grad=True))
    with pytest.raises(ValueError):
        w(x, 1.0, lengths=[25, 26])
    with pytest.raises(ValueError):                               # (the samples live on the GPU)
        w(x, 1.0)
    assert w.pool == []
    # the cut into blocks: whole blocks, the rest, and an empty clip as one block of no frames; ratios past a clip's blocks are not read
    frames, rates = w.blocks([25, 0, 10], [[1.0, 2.0, 3.0], [0.5, -1.0, -1.0], [0.25, float("nan"), 0.0]])
    assert frames == [[10, 10, 5], [0], [10]] and rates == [[1.0, 2.0, 3.0], [0.5], [0.25]]
    assert w.blocks([25, 3], 1.5) == ([[10, 10, 5], [3]], [[1.5] * 3, [1.5]])
    assert w.blocks([25, 3], torch.tensor([1.5, 0.5])) == ([[10, 10, 5], [3]], [[1.5] * 3, [0.5]])
