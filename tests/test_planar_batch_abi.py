"""CPU: the planar batch entries — resampleProcessAndFlushPlanarDevice, resampleProcessBatchPlanarDevice and
resampleProcessAndFlushBatchPlanarDevice are exported by both libraries, declared in art_hip.h and listed in EXPORTED_SYMBOLS; the batch
entries' refusals need no device; transpose_group_kernel, the one launch that moves every staged buffer of a batch, is in both libraries
(planes -> frames and frames -> planes) and uses no scratch."""
import ctypes as C
import os

import pytest

import audio_resampler_amd as A
from test_matrix_batch_abi import _code_objects, _kernel_notes      # noqa: F401  (the 4-byte library's notes)

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
NEW = ("resampleProcessAndFlushPlanarDevice", "resampleProcessBatchPlanarDevice", "resampleProcessAndFlushBatchPlanarDevice")


@pytest.mark.parametrize("width", [32, 64])
def test_symbols_are_exported_declared_and_listed(width):
    B = A.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    for name in NEW:
        assert name in B.EXPORTED_SYMBOLS, name
        assert hasattr(B.lib(), name), name
        assert f"{name} (" in header, name
    assert B.EXPORTED_SYMBOLS["resampleProcessBatchPlanarDevice"] == B.EXPORTED_SYMBOLS["resampleProcessAndFlushBatchPlanarDevice"]
    assert B.EXPORTED_SYMBOLS["resampleProcessAndFlushPlanarDevice"] == B.EXPORTED_SYMBOLS["resampleProcessPlanarDevice"]
    # a pitch list more than the interleaved entries: two
    assert len(B.EXPORTED_SYMBOLS["resampleProcessBatchPlanarDevice"][1]) == len(B.EXPORTED_SYMBOLS["resampleProcessBatchInterleavedDevice"][1]) + 2
    # the internal C ABI stays out of the public header
    assert "arthip_transpose_group" not in header and "ArtLayoutItem" not in header
    for name in ("process_batch_planar_device", "process_and_flush_batch_planar_device", "ClipResampler"):
        assert callable(getattr(B, name)), name
        assert callable(getattr(A, name)), name
    assert callable(B.Resampler.process_and_flush_planar_device)


@pytest.mark.parametrize("width", [32, 64])
@pytest.mark.parametrize("name", NEW[1:])
def test_refusals_need_no_device(width, name):
    """n <= 0 returns 0 and a NULL context -1 before anything of the device is touched"""
    L = A.binding(width).lib()
    fn = getattr(L, name)
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    assert fn(none, 0, None, None, None, None, None, None, None, None) == 0
    assert fn(none, -3, None, None, None, None, None, None, None, None) == 0
    assert fn(none, 1, None, None, None, None, None, None, None, None) == -1
    assert L.artamdErrorCount() == errors


def test_transpose_kernel_is_in_both_libraries():
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        assert b"transpose_group_kernelILb0" in blob and b"transpose_group_kernelILb1" in blob, path


def test_transpose_kernel_uses_no_scratch(tmp_path):
    kernels = {s: f for s, f in _kernel_notes(tmp_path).items() if "transpose_group_kernel" in s}
    assert len(kernels) == 2, sorted(kernels)
    for s, f in kernels.items():
        print(s, {k: f.get(k) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count")})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)
        assert int(f["group_segment_fixed_size"]) == 32768, (s, f)
