"""resampleProcessAndFlushBatchInterleavedDevice on the host side: exported by both builds, declared in art_hip.h with the documented
prototype, bound in the Python mirror for both widths, callable from a C translation unit that sees only include/, and the refusals
that are settled before anything touches a device."""
import os
import re
import subprocess

import pytest

import audio_resampler_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "resampleProcessAndFlushBatchInterleavedDevice"
PARAMS = ["Resample *const *cxts", "int n", "const artsample_t *const *d_inputs", "const int *numInputFrames",
          "artsample_t *const *d_outputs", "const int *numOutputFrames", "const double *ratios", "ResampleResult *results"]


@pytest.mark.parametrize("width", [32, 64])
def test_exported_by_both_libraries_and_bound(width):
    B = A.binding(width)
    assert hasattr(B.lib(), NAME)
    assert NAME in B.EXPORTED_SYMBOLS
    # the same shape as the existing batch entry's binding
    assert B.EXPORTED_SYMBOLS[NAME] == B.EXPORTED_SYMBOLS["resampleProcessBatchInterleavedDevice"]
    assert callable(B.process_and_flush_batch_device)
    assert callable(A.process_and_flush_batch_device)


def test_declared_in_art_hip_h_with_the_documented_prototype():
    text = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{}]*)\)\s*;", text)
    assert m, "prototype not found"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == PARAMS


@pytest.mark.parametrize("width,ctype", [(32, "float"), (64, "double")])
def test_client_compile_takes_the_builds_sample_type(width, ctype):
    src = ('#include "resampler.h"\n#include "biquad.h"\n#include "decimator.h"\n#include "art_hip.h"\n'
           f"int call (Resample *const *cxts, int n, const {ctype} *const *in, const int *nin, {ctype} *const *out, const int *cap,\n"
           "          const double *ratios, ResampleResult *res)\n"
           f"{{ return {NAME} (cxts, n, in, nin, out, cap, ratios, res); }}\n")
    defs = ["-DPATH_WIDTH=64"] if width == 64 else []
    # (an undeclared call would otherwise be a warning only, and a mismatched sample type too)
    p = subprocess.run(["gcc", "-std=c99", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
                        "-I", os.path.join(ROOT, "include"), "-fsyntax-only", "-x", "c", "-"] + defs,
                       input=src, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


@pytest.mark.parametrize("width", [32, 64])
def test_nothing_to_do_and_a_null_context_are_settled_before_any_device_work(width):
    """these calls never reach a device, so they answer the same with or without one"""
    import ctypes as C
    L = A.binding(width).lib()
    before = L.artamdErrorCount()
    assert L.resampleProcessAndFlushBatchInterleavedDevice(None, 0, None, None, None, None, None, None) == 0
    assert L.resampleProcessAndFlushBatchInterleavedDevice(None, -2, None, None, None, None, None, None) == 0
    ctx = (C.c_void_p * 2)(None, None)
    res = (A.binding(width).ResampleResult * 2)()
    assert L.resampleProcessAndFlushBatchInterleavedDevice(ctx, 2, None, None, None, None, None, res) == -1
    assert L.artamdErrorCount() == before
