"""CPU: decimateProcessClipsPlanarLEDevice and resampleProcessAndFlushClipsPlanarDevice — exported by both libraries, declared in
art_hip.h with the build's sample type, listed in EXPORTED_SYMBOLS with the batch entries' argument types plus the new ones, and
wrapped; their refusals need no device; the grouped zeroing kernel and the decimator's clips kernels (the batch kernels' bodies
over the clips entry's record types) are in both libraries and use no scratch; the batch entry's own kernels still use none."""
import ctypes as C
import os
import re

import pytest

import audio_resampler_amd as A
from test_matrix_batch_abi import _kernel_notes

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
DEC, RES = "decimateProcessClipsPlanarLEDevice", "resampleProcessAndFlushClipsPlanarDevice"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def _declared(header, name):
    decl = re.search(r"int " + name + r" \(([^;]*)\);", header)
    assert decl, name + " is not declared"
    return " ".join(decl.group(1).split())


@pytest.mark.parametrize("width", [32, 64])
def test_symbols_are_exported_declared_and_listed(width):
    B = A.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    for name in (DEC, RES):
        assert name in B.EXPORTED_SYMBOLS and hasattr(B.lib(), name), name
    # declared with the build's sample type (artsample_t is float or double by PATH_WIDTH) and the batch entries' arguments
    assert _declared(header, DEC) == (
        "Decimate *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames, "
        "unsigned char *const *d_outputs, const long *outputPitches, int fromStart, unsigned long long *d_clipCounts")
    assert _declared(header, RES) == (
        "Resample *const *cxts, int n, const artsample_t *const *d_inputs, const long *inputPitches, const int *numInputFrames, "
        "artsample_t *const *d_outputs, const long *outputPitches, const int *numOutputFrames, const double *ratios, int fromStart, "
        "ResampleResult *results")
    res, argtypes = B.EXPORTED_SYMBOLS[DEC]
    assert res is C.c_int and argtypes == B.EXPORTED_SYMBOLS["decimateProcessBatchPlanarLEDevice"][1] + [C.c_int, C.c_void_p]
    res, argtypes = B.EXPORTED_SYMBOLS[RES]
    batch = B.EXPORTED_SYMBOLS["resampleProcessAndFlushBatchPlanarDevice"][1]
    assert res is C.c_int and argtypes == batch[:-1] + [C.c_int] + batch[-1:]
    # the record types and the private form stay out of the public header
    assert "ArtDecClip" not in header and "ArtZeroRun" not in header and "artamd_decimate_clips_planar" not in header
    for M in (A, B):
        assert callable(M.decimate_clips_planar_device) and callable(M.process_and_flush_clips_planar_device)
    assert "launches" in A.ClipDecimator.__call__.__code__.co_names
    for cls in (A.ClipDecimator, A.ClipResampler):              # from a fresh start by the call itself, no loop of resets
        code = cls.__call__.__code__
        names = code.co_names + code.co_freevars
        assert ("decimate_clips_planar_device" in names) or ("process_and_flush_clips_planar_device" in names), cls
        assert "clipped" not in names and "decimate_batch_planar_device" not in names, cls
        assert "process_and_flush_batch_planar_device" not in names, cls


@pytest.mark.parametrize("width", [32, 64])
def test_refusals_need_no_device(width):
    """n <= 0 returns 0 with NULL arrays, and a NULL context -1, before anything of the device is touched"""
    L = A.binding(width).lib()
    dec, res = getattr(L, DEC), getattr(L, RES)
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    for from_start in (0, 1):
        assert dec(None, 0, None, None, None, None, None, from_start, None) == 0
        assert dec(none, 0, None, None, None, None, None, from_start, None) == 0
        assert dec(none, -3, None, None, None, None, None, from_start, None) == 0
        assert dec(none, 1, None, None, None, None, None, from_start, None) == -1
        assert dec(none, 1, None, (C.c_long * 1)(5), (C.c_int * 1)(7), None, None, from_start, None) == -1
        assert res(None, 0, None, None, None, None, None, None, None, from_start, None) == 0
        assert res(none, -1, None, None, None, None, None, None, None, from_start, None) == 0
        assert res(none, 1, None, None, None, None, None, None, None, from_start, None) == -1
    assert L.artamdErrorCount() == errors


def test_new_kernels_are_in_both_libraries():
    """the serial wave over ArtDecClipLane: five orders x dither off / on; the time-parallel form over ArtDecClipTask: dither off / on;
    the grouped zeroing kernel"""
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for dither in (0, 1):
            for order in range(5):
                assert f"decimate_clips_pipe_kernelILi{order}ELb{dither}EE".encode() in blob, (path, order, dither)
            assert f"decimate_clips_parallel_kernelILb{dither}EE".encode() in blob, (path, dither)
        assert b"zero_runs_group_kernel" in blob, path


def test_new_kernels_use_no_scratch_and_the_batch_kernels_still_use_none(tmp_path):
    notes = _kernel_notes(tmp_path)
    new = {s: f for s, f in notes.items() if "decimate_clips_" in s or "zero_runs_group_kernel" in s}
    assert len(new) == 10 + 2 + 1, sorted(new)
    old = {s: f for s, f in notes.items() if "decimate_batch_pipe_kernel" in s or "decimate_batch_parallel_kernel" in s}
    assert len(old) == 5 * 2 * 2 + 2 * 2, sorted(old)                  # (orders x dither x pitched) + (dither x pitched)
    for s, f in sorted(new.items()) + sorted(old.items()):
        print(s, {k: f.get(k) for k in FIELDS})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)
