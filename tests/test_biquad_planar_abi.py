"""CPU: the planar biquad bank entries — biquadBankApplyPlanarDevice, biquadBankApplyBatchPlanarDevice and biquadBankReset are
exported by both libraries, declared in art_hip.h and listed in EXPORTED_SYMBOLS; the batch entry's refusals need no device; the
time-parallel kernels have their planar instantiations beside the interleaved ones in both libraries; and the biquad kernels use no
scratch."""
import ctypes as C
import os

import pytest

import audio_resampler_amd as A
from test_matrix_batch_abi import _code_objects, _kernel_notes      # noqa: F401  (the 4-byte library's notes)

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
NEW = ("biquadBankApplyPlanarDevice", "biquadBankApplyBatchPlanarDevice", "biquadBankReset")
# the kernels the planar entries add (spec, commit: planar instantiations) or change (the batch kernel's helper loop), and the check
# kernel that runs between the two
TOUCHED = ("biquad_spec_kernel", "biquad_check_kernel", "biquad_commit_kernel", "biquad_batch_pipe_kernel")


@pytest.mark.parametrize("width", [32, 64])
def test_symbols_are_exported_declared_and_listed(width):
    B = A.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    for name in NEW:
        assert name in B.EXPORTED_SYMBOLS, name
        assert hasattr(B.lib(), name), name
        assert f"{name} (" in header, name
    single, twin = B.EXPORTED_SYMBOLS["biquadBankApplyPlanarDevice"][1], B.EXPORTED_SYMBOLS["biquadBankApplyInterleavedDevice"][1]
    assert len(single) == len(twin) + 1 and single[2] is C.c_long            # the pitch, in samples
    assert [a for i, a in enumerate(single) if i != 2] == twin
    assert len(B.EXPORTED_SYMBOLS["biquadBankApplyBatchPlanarDevice"][1]) == len(B.EXPORTED_SYMBOLS["biquadBankApplyBatchInterleavedDevice"][1]) + 1
    # the private form (a lane count per workgroup) is exported for the tests and stays out of the public header
    assert hasattr(B.lib(), "artamd_biquad_batch_planar") and "artamd_biquad_batch_planar" not in header
    assert "arthip_biquad_spec_planar" not in header and "ArtBqLane" not in header
    for name in ("biquad_batch_planar_device", "ClipFilter"):
        assert callable(getattr(B, name)), name
        assert callable(getattr(A, name)), name
    for name in ("apply_planar_device", "reset"):
        assert callable(getattr(B.BiquadBank, name)), name


@pytest.mark.parametrize("width", [32, 64])
def test_batch_refusals_need_no_device(width):
    """n <= 0 returns 0 and a NULL bank -1 before anything of the device is touched"""
    L = A.binding(width).lib()
    fn = L.biquadBankApplyBatchPlanarDevice
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    assert fn(none, 0, None, None, None) == 0
    assert fn(None, 0, None, None, None) == 0
    assert fn(none, -3, None, None, None) == 0
    assert fn(none, 1, None, None, None) == -1
    assert fn(none, 1, None, (C.c_long * 1)(5), None) == -1
    assert L.artamdErrorCount() == errors


def test_clip_filter_refuses_bad_sections_without_a_device():
    for bad in ([], [("lowpass", 0.1)] * 5, [("bandpass", 0.1)]):
        with pytest.raises(ValueError):
            A.ClipFilter(2, bad)


def test_planar_instantiations_are_in_both_libraries():
    """the second template argument of the time-parallel kernels: Lb0 interleaved (channel fastest), Lb1 planes (chunk fastest)"""
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for s in range(1, 5):
            for k in ("biquad_spec_kernel", "biquad_commit_kernel"):
                for planar in (0, 1):
                    name = f"{k}ILi{s}ELb{planar}EE"
                    assert name.encode() in blob, (path, name)
            assert f"biquad_batch_pipe_kernelILi{s}EE".encode() in blob, (path, s)


def _report(kernels):
    for s, f in sorted(kernels.items()):
        print(s, {k: f.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})


def test_new_and_changed_biquad_kernels_use_no_scratch(tmp_path):
    """the planar instantiations, their interleaved twins (same template) and the batch kernel whose helper loop moves planes 16
    bytes at a time"""
    kernels = {s: f for s, f in _kernel_notes(tmp_path).items() if any(k in s for k in TOUCHED)}
    assert len(kernels) == 4 * 2 + 4 + 4 * 2 + 4, sorted(kernels)
    _report(kernels)
    for s, f in sorted(kernels.items()):
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0, (s, f)      # (scalar registers parked in vector lanes use no memory)


def test_every_biquad_kernel_uses_no_scratch(tmp_path):
    """Every biquad_* kernel of the 4-byte library, the serial single-call kernels included: biquad_order2_ff_kernel kept its helper
    waves' runs of frames in 416 bytes of scratch while its loops over a run ended in a break (a run-time trip count: the arrays
    were indexed by a register); with a guard per group of four frames the trip counts are constants and the runs live in registers."""
    kernels = {s: f for s, f in _kernel_notes(tmp_path).items() if "biquad_" in s}
    assert len(kernels) == 2 + 4 * 2 + 4 + 4 * 2 + 2 + 4, sorted(kernels)
    _report(kernels)
    for s, f in sorted(kernels.items()):
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0, (s, f)


def test_order2_kernel_uses_no_scratch_in_the_wide_build(tmp_path, monkeypatch):
    """the same kernel with 8-byte samples holds twice the registers per frame: no scratch and no spill there either"""
    import test_matrix_batch_abi as T
    monkeypatch.setattr(T, "LIB32", LIB64)
    kernels = {s: f for s, f in _kernel_notes(tmp_path).items() if "biquad_order2_ff_kernel" in s}
    assert len(kernels) == 2, sorted(kernels)
    _report(kernels)
    for s, f in sorted(kernels.items()):
        assert int(f["private_segment_fixed_size"]) == 0 and int(f.get("vgpr_spill_count", 0)) == 0, (s, f)
