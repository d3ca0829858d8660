"""CPU: biquadBankApplyClipsPlanarDevice — exported by both libraries, declared in art_hip.h with the build's sample type, listed in
EXPORTED_SYMBOLS and wrapped (biquad_clips_planar_device, ClipFilter.launches); its refusals need no device; the gathered
time-parallel kernels are in both libraries, one instantiation per section count and layout, and use no scratch."""
import ctypes as C
import os
import re

import pytest

import audio_resampler_amd as A
from test_matrix_batch_abi import _kernel_notes

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
NAME = "biquadBankApplyClipsPlanarDevice"


@pytest.mark.parametrize("width", [32, 64])
def test_symbol_is_exported_declared_and_listed(width):
    B = A.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    assert NAME in B.EXPORTED_SYMBOLS
    assert hasattr(B.lib(), NAME)
    # declared with the build's sample type (artsample_t is float or double by PATH_WIDTH, biquad.h) and the batch entry's arguments
    decl = re.search(r"int " + NAME + r" \(([^;]*)\);", header)
    assert decl, "not declared"
    args = " ".join(decl.group(1).split())
    assert args == ("BiquadBank *const *banks, int n, artsample_t *const *d_buffers, const long *pitches, const int *numFrames, "
                    "int fromStart")
    res, argtypes = B.EXPORTED_SYMBOLS[NAME]
    assert res is C.c_int and argtypes == B.EXPORTED_SYMBOLS["biquadBankApplyBatchPlanarDevice"][1] + [C.c_int]
    # the private form (its own byte bound per round) is exported for the tests and stays out of the public header
    assert hasattr(B.lib(), "artamd_biquad_clips_planar") and "artamd_biquad_clips_planar" not in header
    assert "ArtBqClip" not in header
    for M in (A, B):
        assert callable(M.biquad_clips_planar_device)
    assert "launches" in A.ClipFilter.__call__.__code__.co_names


@pytest.mark.parametrize("width", [32, 64])
def test_refusals_need_no_device(width):
    """n <= 0 returns 0 with NULL arrays, and a NULL bank -1, before anything of the device is touched"""
    L = A.binding(width).lib()
    fn = getattr(L, NAME)
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    for from_start in (0, 1):
        assert fn(None, 0, None, None, None, from_start) == 0
        assert fn(none, 0, None, None, None, from_start) == 0
        assert fn(none, -3, None, None, None, from_start) == 0
        assert fn(none, 1, None, None, None, from_start) == -1
        assert fn(none, 1, None, (C.c_long * 1)(5), None, from_start) == -1
    assert L.artamdErrorCount() == errors


def test_gathered_kernels_are_in_both_libraries():
    """spec and commit: one instantiation per section count and layout (Lb0 interleaved, Lb1 planes); check: per section count"""
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for s in range(1, 5):
            for planar in (0, 1):
                for k in ("bq_clips_spec_kernel", "bq_clips_commit_kernel"):
                    assert f"{k}ILi{s}ELb{planar}EE".encode() in blob, (path, k, s, planar)
            assert f"bq_clips_check_kernelILi{s}EE".encode() in blob, (path, s)
        assert b"copy_rows_group_kernel" in blob, path


def test_gathered_kernels_use_no_scratch(tmp_path):
    kernels = {s: f for s, f in _kernel_notes(tmp_path).items() if "bq_clips_" in s or "copy_rows_group_kernel" in s}
    assert len(kernels) == 4 * 2 + 4 + 4 * 2 + 1, sorted(kernels)
    for s, f in sorted(kernels.items()):
        print(s, {k: f.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0, (s, f)
