"""CPU: the planar decimator entries — decimateProcessPlanarLEDevice, decimateProcessBatchPlanarLEDevice and decimateHipReset are
exported by both libraries, declared in art_hip.h and listed in EXPORTED_SYMBOLS; the batch entry's refusals need no device; every
decimator kernel that moves samples has its planar (PITCHED) instantiation beside the interleaved one in both libraries, and none of
them uses scratch."""
import ctypes as C
import os

import pytest

import audio_resampler_amd as A
from test_matrix_batch_abi import _code_objects, _kernel_notes      # noqa: F401  (the 4-byte library's notes)

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
NEW = ("decimateProcessPlanarLEDevice", "decimateProcessBatchPlanarLEDevice", "decimateHipReset")
KERNELS = ("decimate_parallel_kernel", "decimate_batch_parallel_kernel", "decimate_lds_kernel", "decimate_pipe_kernel",
           "decimate_batch_pipe_kernel")


@pytest.mark.parametrize("width", [32, 64])
def test_symbols_are_exported_declared_and_listed(width):
    B = A.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    for name in NEW:
        assert name in B.EXPORTED_SYMBOLS, name
        assert hasattr(B.lib(), name), name
        assert f"{name} (" in header, name
    # a pitch per side more than the interleaved entries
    assert len(B.EXPORTED_SYMBOLS["decimateProcessPlanarLEDevice"][1]) == len(B.EXPORTED_SYMBOLS["decimateProcessInterleavedLEDevice"][1]) + 2
    assert len(B.EXPORTED_SYMBOLS["decimateProcessBatchPlanarLEDevice"][1]) == len(B.EXPORTED_SYMBOLS["decimateProcessBatchInterleavedLEDevice"][1]) + 2
    assert B.EXPORTED_SYMBOLS["decimateProcessPlanarLEDevice"][1][2] is C.c_long and B.EXPORTED_SYMBOLS["decimateProcessPlanarLEDevice"][1][5] is C.c_long
    # the private forms (a lane count per workgroup) are exported for the tests and stay out of the public header
    for name in ("artamd_decimate_batch", "artamd_decimate_batch_planar"):
        assert hasattr(B.lib(), name), name
        assert name not in header, name
    assert "arthip_decimate_pitched" not in header and "ArtDecLane" not in header
    for name in ("decimate_batch_planar_device", "ClipDecimator"):
        assert callable(getattr(B, name)), name
        assert callable(getattr(A, name)), name
    for name in ("process_planar_device", "reset"):
        assert callable(getattr(B.Decimator, name)), name
    assert callable(B.ClipDecimator.as_int)


@pytest.mark.parametrize("width", [32, 64])
def test_batch_refusals_need_no_device(width):
    """n <= 0 returns 0 and a NULL context -1 before anything of the device is touched"""
    L = A.binding(width).lib()
    fn = L.decimateProcessBatchPlanarLEDevice
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    assert fn(none, 0, None, None, None, None, None) == 0
    assert fn(None, 0, None, None, None, None, None) == 0
    assert fn(none, -3, None, None, None, None, None) == 0
    assert fn(none, 1, None, None, None, None, None) == -1
    assert L.artamdErrorCount() == errors


def test_planar_instantiations_are_in_both_libraries():
    """the third template argument of the serial kernels, the second of the time-parallel ones: Lb0 interleaved, Lb1 with pitches"""
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for k in KERNELS:
            assert k.encode() in blob, (path, k)
        for k in ("decimate_parallel_kernelILb0ELb1E", "decimate_parallel_kernelILb1ELb1E", "decimate_batch_parallel_kernelILb1ELb1E",
                  "decimate_pipe_kernelILi4ELb1ELb1E", "decimate_lds_kernelILi4ELb1ELb1E", "decimate_batch_pipe_kernelILi4ELb1ELb1E",
                  "decimate_batch_pipe_kernelILi0ELb0ELb1E", "decimate_pipe_kernelILi1ELb0ELb0E"):
            assert k.encode() in blob, (path, k)


def test_decimator_kernels_use_no_scratch(tmp_path):
    kernels = {s: f for s, f in _kernel_notes(tmp_path).items() if any(k in s for k in KERNELS)}
    assert len(kernels) == 2 * (2 + 2 + 10 + 8 + 10), sorted(kernels)
    for s, f in sorted(kernels.items()):
        print(s, {k: f.get(k) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0, (s, f)      # (scalar registers parked in vector lanes use no memory)
