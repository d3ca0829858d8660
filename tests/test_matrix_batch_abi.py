"""CPU: the grouped matrix-core launch of the batch entries (fir_mfma_group_kernel, mfma_head_group_kernel) is compiled into the 4-byte
library only — libartamd64.so has no streaming kernel and keeps making those calls one by one — behind an unchanged public ABI (no new
entry point: resampleProcessBatchInterleavedDevice and resampleProcessAndFlushBatchInterleavedDevice keep their signatures), and within
the register budget of the single launch's kernel: no scratch, no more VGPRs than fir_mfma_stream_kernel (three workgroups per CU)."""
import os
import re
import struct
import subprocess

import pytest

import audio_resampler_amd as A

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
NEW_KERNELS = (b"fir_mfma_group_kernel", b"mfma_head_group_kernel")


def test_new_kernels_are_in_the_4_byte_library_only():
    blob32, blob64 = open(LIB32, "rb").read(), open(LIB64, "rb").read()
    for name in NEW_KERNELS:
        assert name in blob32, name
        assert name not in blob64, name
    assert b"fir_mfma_stream_kernel" in blob32 and b"fir_mfma_stream_kernel" not in blob64


def test_no_new_entry_point():
    B, W = A.binding(32), A.binding(64)
    assert set(B.EXPORTED_SYMBOLS) == set(W.EXPORTED_SYMBOLS)
    assert not [n for n in B.EXPORTED_SYMBOLS if "Group" in n or "group" in n]
    for L in (B, W):
        for name in ("resampleProcessBatchInterleavedDevice", "resampleProcessAndFlushBatchInterleavedDevice", "resampleHipLastGathered"):
            assert hasattr(L.lib(), name), name
    assert B.EXPORTED_SYMBOLS["resampleProcessAndFlushBatchInterleavedDevice"] == B.EXPORTED_SYMBOLS["resampleProcessBatchInterleavedDevice"]
    # the internal C ABI stays out of the public header
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    assert "arthip_fir_group" not in header


def _code_objects(blob):
    """the gfx code objects embedded in a library: ELF images of machine EM_AMDGPU (224), sized by their section header table"""
    at = 0
    while True:
        at = blob.find(b"\x7fELF\x02\x01\x01", at)
        if at < 0:
            return
        machine = struct.unpack_from("<H", blob, at + 18)[0]
        shoff, = struct.unpack_from("<Q", blob, at + 40)
        shentsize, shnum = struct.unpack_from("<HH", blob, at + 58)
        if machine == 224 and shoff and at + shoff + shentsize * shnum <= len(blob):
            yield blob[at:at + shoff + shentsize * shnum]
        at += 4


def _kernel_notes(tmp_path):
    readelf = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        pytest.skip("no llvm-readelf under the ROCm install")
    kernels = {}
    for k, co in enumerate(_code_objects(open(LIB32, "rb").read())):
        path = tmp_path / f"co{k}.elf"
        path.write_bytes(co)
        text = subprocess.run([readelf, "--notes", str(path)], capture_output=True, text=True, timeout=300).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", text)[1:]:
            f = dict(re.findall(r"\.(\w+):\s+'?([\w.$@]+)'?", ".agpr_count:" + block))
            if "symbol" in f:
                kernels[f["symbol"]] = f
    return kernels


def test_group_kernel_register_budget(tmp_path):
    kernels = _kernel_notes(tmp_path)
    group = {s: f for s, f in kernels.items() if "fir_mfma_group_kernel" in s}
    stream = {s: f for s, f in kernels.items() if "fir_mfma_stream_kernel" in s and s.endswith("Lb0EEEv10ArtFirArgs8MfmaGeomi.kd")}      # (the plain instantiations)
    assert len(group) == 12 and len(stream) == 12, (sorted(group), sorted(stream))
    budget = max(int(f["vgpr_count"]) for f in stream.values())
    for s, f in group.items():
        print(s, {k: f.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)
        assert int(f["vgpr_count"]) + int(f.get("agpr_count", 0)) <= budget, (s, f, budget)
    heads = [f for s, f in kernels.items() if "mfma_head_group_kernel" in s]
    assert len(heads) == 1 and int(heads[0]["private_segment_fixed_size"]) == 0
