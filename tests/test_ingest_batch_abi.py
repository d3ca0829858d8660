"""floatIntegersBatchLEDevice on the host side: exported by both builds, declared in art_hip.h with the build's sample type, and the
argument checks that run before anything touches a device."""
import ctypes as C
import os
import re
import subprocess

import pytest

import audio_resampler_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "floatIntegersBatchLEDevice"


@pytest.mark.parametrize("width", [32, 64])
def test_exported_by_both_libraries_and_bound(width):
    B = A.binding(width)
    assert hasattr(B.lib(), NAME)
    assert NAME in B.EXPORTED_SYMBOLS
    assert callable(B.ingest_batch_device)


def test_declared_in_art_hip_h():
    text = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{}]*)\)\s*;", text)
    assert m, "prototype not found"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 9
    assert params[5].startswith("artsample_t *const *")


@pytest.mark.parametrize("width,ctype", [(32, "float"), (64, "double")])
def test_client_compile_takes_the_builds_sample_type(width, ctype):
    src = ('#include "resampler.h"\n#include "biquad.h"\n#include "decimator.h"\n#include "art_hip.h"\n'
           f"int call (const unsigned char *const *in, const double *g, const int *b, {ctype} *const *out, const int *n)\n"
           f"{{ return {NAME} (in, g, b, b, b, out, n, 1, 0); }}\n")
    defs = ["-DPATH_WIDTH=64"] if width == 64 else []
    # (an undeclared call would otherwise be a warning only, and a mismatched sample type too)
    p = subprocess.run(["gcc", "-std=c99", "-Werror=implicit-function-declaration", "-Werror=incompatible-pointer-types",
                        "-I", os.path.join(ROOT, "include"), "-fsyntax-only", "-x", "c", "-"] + defs,
                       input=src, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr


@pytest.mark.parametrize("width", [32, 64])
def test_every_whole_run_of_a_sample_aligned_output_is_16_byte_aligned(width):
    """run k of an item starts at sample k * R - head (R = 16 bytes of samples): at byte address - head * size + 16 k"""
    fn = A.binding(width).lib().artamd_ingest_head          # library-private
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p]
    size = width // 8
    for base in (0x10000, 0x7F0000001000):
        for off in range(32):
            addr = base + off
            head = fn(addr)
            if off % size:
                assert head == 0, (off, head)            # not sample-aligned: every store is a scalar one
            else:
                assert 0 <= head < 16 // size and (addr - head * size) % 16 == 0, (off, head)


def _arrays(items):
    n = len(items)
    return ((C.c_void_p * n)(*[it[0] for it in items]), (C.c_double * n)(*([0.5] * n)), (C.c_int * n)(*[it[2] for it in items]),
            (C.c_int * n)(*([2] * n)), (C.c_int * n)(*([1] * n)), (C.c_void_p * n)(*[it[1] for it in items]),
            (C.c_int * n)(*[it[3] for it in items]))


@pytest.mark.parametrize("width", [32, 64])
def test_nothing_to_do_and_null_pointers_are_settled_before_any_device_work(width):
    """(input, output, bits, count): these calls never reach a device, so they answer the same with or without one"""
    L = A.binding(width).lib()
    before = L.artamdErrorCount()
    assert L.floatIntegersBatchLEDevice(None, None, None, None, None, None, None, 0, None) == 0
    assert L.floatIntegersBatchLEDevice(None, None, None, None, None, None, None, -3, None) == 0
    fake = 0x1000
    # every item skipped (count <= 0, bits > 24), NULL pointers included: nothing to do
    skipped = [(fake, fake, 16, 0), (None, None, 16, -1), (fake, fake, 25, 10), (None, fake, 32, 10)]
    assert L.floatIntegersBatchLEDevice(*_arrays(skipped), len(skipped), None) == 0
    # a live item with a NULL input or output: refused, not counted as a launch failure
    for bad in ((None, fake, 16, 10), (fake, None, 24, 1)):
        items = skipped + [bad]
        assert L.floatIntegersBatchLEDevice(*_arrays(items), len(items), None) == -1
    assert L.artamdErrorCount() == before
