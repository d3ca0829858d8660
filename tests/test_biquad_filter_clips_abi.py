"""CPU: biquadBankFilterClipsPlanarDevice — exported by both libraries, declared in art_hip.h with the build's sample type, listed in
EXPORTED_SYMBOLS and wrapped (biquad_filter_clips_planar_device; ClipFilter's autograd path calls it); its refusals need no device;
its kernels (out-of-place gathered passes and serial pipe, each with a compile-time direction) are in both libraries under names
that no existing count of `biquad_` or `bq_clips_` kernels sees, and use no scratch; and the kernels that were there before have the
resource rows recorded from the parent commit (tests/golden/biquad_kernel_rows_parent.json), in both builds."""
import ctypes as C
import json
import os
import re

import pytest

import audio_resampler_amd as A
import test_matrix_batch_abi as T
from test_matrix_batch_abi import _kernel_notes

PKG = os.path.dirname(os.path.abspath(A.__file__))
HERE = os.path.dirname(os.path.abspath(__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
NAME = "biquadBankFilterClipsPlanarDevice"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")
NEW = ("bq_filter_spec_kernel", "bq_filter_commit_kernel", "bq_filter_pipe_kernel")


@pytest.mark.parametrize("width", [32, 64])
def test_symbol_is_exported_declared_and_listed(width):
    B = A.binding(width)
    header = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    assert NAME in B.EXPORTED_SYMBOLS and NAME in A.EXPORTED_SYMBOLS
    assert hasattr(B.lib(), NAME)
    decl = re.search(r"int " + NAME + r" \(([^;]*)\);", header)
    assert decl, "not declared"
    assert " ".join(decl.group(1).split()) == (
        "BiquadBank *const *banks, int n, const artsample_t *const *d_ins, const long *in_pitches, artsample_t *const *d_outs, "
        "const long *out_pitches, const int *numFrames, int reversed")
    res, argtypes = B.EXPORTED_SYMBOLS[NAME]
    assert res is C.c_int and argtypes == [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int]
    # the private form (its own byte bound per round) is exported for the tests and stays out of the public header
    assert hasattr(B.lib(), "artamd_biquad_filter_clips_planar") and "artamd_biquad_filter_clips_planar" not in header
    assert "ArtBqFilterLane" not in header
    for M in (A, B):
        assert callable(M.biquad_filter_clips_planar_device)
    assert "requires_grad" in A.ClipFilter.__call__.__code__.co_names and "launches" in A.ClipFilter.__call__.__code__.co_names


@pytest.mark.parametrize("width", [32, 64])
def test_refusals_need_no_device(width):
    """n <= 0 returns 0 with NULL arrays; a NULL bank, buffer or list -1, before anything of the device is touched and uncounted"""
    L = A.binding(width).lib()
    fn = getattr(L, NAME)
    errors = L.artamdErrorCount()
    none = (C.c_void_p * 1)(None)
    for reverse in (0, 1):
        assert fn(None, 0, None, None, None, None, None, reverse) == 0
        assert fn(none, 0, None, None, None, None, None, reverse) == 0
        assert fn(none, -3, None, None, None, None, None, reverse) == 0
        assert fn(none, 1, None, None, None, None, None, reverse) == -1
        assert fn(none, 1, none, (C.c_long * 1)(5), none, (C.c_long * 1)(5), (C.c_int * 1)(7), reverse) == -1
    assert L.artamdErrorCount() == errors


def test_new_kernels_are_in_both_libraries_under_names_of_their_own():
    """spec and commit: section count x layout x direction; the serial pipe: section count x direction.  No name has `biquad_` or
    `bq_clips_` in it: the existing tests' counts of those stay what they were."""
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for s in range(1, 5):
            for rev in (0, 1):
                for planar in (0, 1):
                    for k in ("bq_filter_spec_kernel", "bq_filter_commit_kernel"):
                        assert f"{k}ILi{s}ELb{planar}ELb{rev}EE".encode() in blob, (path, k, s, planar, rev)
                assert f"bq_filter_pipe_kernelILi{s}ELb{rev}EE".encode() in blob, (path, s, rev)


@pytest.mark.parametrize("width", [32, 64])
def test_new_kernels_use_no_scratch_and_the_old_ones_keep_their_rows(tmp_path, monkeypatch, width):
    if width == 64:
        monkeypatch.setattr(T, "LIB32", LIB64)
    notes = _kernel_notes(tmp_path)
    new = {s: f for s, f in notes.items() if any(k in s for k in NEW)}
    assert len(new) == 2 * (4 * 2 * 2) + 4 * 2, sorted(new)
    for s, f in sorted(new.items()):
        print(s, {k: f.get(k) for k in FIELDS})
        assert not s.startswith("biquad_") and "biquad_" not in s and "bq_clips_" not in s, s
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0, (s, f)          # (scalar registers parked in vector lanes use no memory)
    parent = json.load(open(os.path.join(HERE, "golden", "biquad_kernel_rows_parent.json")))[str(width)]
    assert len(parent) == 49
    for s, want in sorted(parent.items()):
        assert s in notes, s
        assert {k: int(notes[s].get(k, 0)) for k in FIELDS} == want, s
    # nothing else of that family appeared
    assert {s for s in notes if "biquad_" in s or "bq_clips_" in s or "copy_rows_group_kernel" in s} == set(parent)
