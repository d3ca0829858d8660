"""artamdExtrapolateBatchDevice and resampleHipLastGathered on the host side: exported by both builds, declared in art_hip.h with the
build's sample type, bound in Python, and the argument checks that run before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import audio_resampler_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "artamdExtrapolateBatchDevice"


def _header():
    text = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("width", [32, 64])
def test_exported_by_both_libraries_and_bound(width):
    B = A.binding(width)
    for name in (NAME, "resampleHipLastGathered"):
        assert hasattr(B.lib(), name)
        assert name in B.EXPORTED_SYMBOLS
    assert callable(B.extrapolate_batch_device)
    assert callable(B.Resampler.last_gathered)


def test_declared_in_art_hip_h():
    text = _header()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{}]*)\)\s*;", text)
    assert m, "prototype not found"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 8
    assert params[0].startswith("const artsample_t *const *") and params[4].startswith("artsample_t *const *")
    assert re.search(r"\bint\s+resampleHipLastGathered\s*\(\s*Resample\s*\*\s*\w*\s*\)\s*;", text)
    m = re.search(r"#define\s+ARTAMD_EXTRAPOLATE_MAX_KNOWN\s+(\d+)", text)
    assert m and int(m.group(1)) >= 1023


@pytest.mark.parametrize("width,ctype", [(32, "float"), (64, "double")])
def test_client_compile_takes_the_builds_sample_type(width, ctype):
    src = ('#include "resampler.h"\n#include "biquad.h"\n#include "decimator.h"\n#include "art_hip.h"\n'
           f"int call (const {ctype} *const *k, const int *n, {ctype} *const *out, Resample *r)\n"
           f"{{ return {NAME} (k, n, n, n, out, n, 1, 0) + resampleHipLastGathered (r); }}\n")
    defs = ["-DPATH_WIDTH=64"] if width == 64 else []
    p = subprocess.run(["gcc", "-std=c99", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
                        "-I", os.path.join(ROOT, "include"), "-fsyntax-only", "-x", "c", "-"] + defs,
                       input=src, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


def _call(L, runs):
    """runs: (known, count, stride, backward, out, extras)"""
    n = len(runs)
    col = lambda j, t: (t * max(n, 1))(*[r[j] for r in runs])
    return L.artamdExtrapolateBatchDevice(col(0, C.c_void_p), col(1, C.c_int), col(2, C.c_int), col(3, C.c_int), col(4, C.c_void_p),
                                          col(5, C.c_int), n, None)


@pytest.mark.parametrize("width", [32, 64])
def test_bad_arguments_are_refused_before_any_device_work(width):
    """these calls never reach a device, so they answer the same with or without one"""
    L = A.binding(width).lib()
    before = L.artamdErrorCount()
    assert L.artamdExtrapolateBatchDevice(None, None, None, None, None, None, 0, None) == 0
    assert L.artamdExtrapolateBatchDevice(None, None, None, None, None, None, -2, None) == 0
    fake = 0x1000
    good = (fake, 64, 1, 0, fake + 4096, 0)                      # (extras 0: a run that writes nothing)
    assert _call(L, [good, good]) == 0
    for bad in ((fake, 7, 1, 0, fake, 5), (fake, 1024, 1, 1, fake, 5), (fake, 64, 1, 0, fake, -1), (fake, 64, 0, 0, fake, 5),
                (fake, 64, -3, 1, fake, 5), (None, 64, 1, 0, fake, 5), (fake, 64, 1, 0, None, 5)):
        assert _call(L, [good, bad]) == -1, bad
    assert L.artamdExtrapolateBatchDevice(None, None, None, None, None, None, 1, None) == -1
    assert L.artamdErrorCount() == before


def test_no_host_fit_remains_in_the_library():
    """one implementation of the fit: the device's.  No C file of the library fits a predictor, and the resampler's extrapolation
    makes no host round trip"""
    csrc = os.path.join(ROOT, "audio_resampler_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith(".c"):
            text = open(os.path.join(csrc, f)).read()
            assert not re.search(r"fit_predictor|reflection_from_predictor|art_extrapolate_(forward|backward)", text), f
    host = open(os.path.join(csrc, "resampler_host.c")).read()
    section = host[host.index("End-point extrapolation"):host.index("static ResampleResult enqueue_call_layouts (Resample *cxt")]
    assert "arthip_d2h" not in section and "arthip_sync" not in section
