"""The schedule entries for planes and for many streams (art_hip.h): resampleProcessSchedulePlanarDevice,
resampleProcessScheduleBatchInterleavedDevice, resampleProcessScheduleBatchPlanarDevice — declared, exported by both libraries and
bound with the right argument counts; the refusals that need no device."""
import ctypes as C
import os
import re

import pytest

import audio_resampler_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"resampleProcessSchedulePlanarDevice": 11,
         "resampleProcessScheduleBatchInterleavedDevice": 11,
         "resampleProcessScheduleBatchPlanarDevice": 13}
WIDTHS = [32, 64]


def _declared():
    text = open(os.path.join(ROOT, "include", "art_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {name: args for name, args in re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(([^;{}]*)\)\s*;", text)}


@pytest.mark.parametrize("width", WIDTHS)
def test_declared_exported_and_bound(width):
    B = A.binding(width)
    L = B.lib()
    declared = _declared()
    for name, nargs in NAMES.items():
        assert name in declared, f"{name} is not declared in art_hip.h"
        assert len(declared[name].split(",")) == nargs, (name, declared[name])
        assert hasattr(L, name), f"{name} is not exported"
        res, args = B.EXPORTED_SYMBOLS[name]
        assert res is C.c_int and len(args) == nargs, (name, res, args)
    for name in ("process_schedule_batch_device", "process_schedule_batch_planar_device"):
        assert callable(getattr(B, name)) and callable(getattr(A, name))
    assert callable(B.Resampler.process_schedule_planar_device)


def _lists(n):
    """well-formed arguments for max(n, 1) streams of two blocks each, every context NULL"""
    m = max(n, 1)
    keep = []

    def rows(ctype, *values):
        keep.extend((ctype * 2)(*values) for _ in range(m))
        return (C.c_void_p * m)(*[C.addressof(r) for r in keep[-m:]])

    return dict(cxts=(C.c_void_p * m)(), blocks=(C.c_int * m)(*([2] * m)), bufs=(C.c_void_p * m)(), frames=rows(C.c_int, 480, 480),
                caps=rows(C.c_int, 600, 600), ratios=rows(C.c_double, 1.0, 1.0), results=rows(A.ResampleResult),
                made=(C.c_int * m)(*([7] * m)), pitches=(C.c_long * m)(*([1000] * m)), keep=keep)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("n", [0, -3])
def test_nothing_to_do_returns_zero(width, n):
    L = A.binding(width).lib()
    a = _lists(n)
    errors = L.artamdErrorCount()
    assert L.resampleProcessScheduleBatchInterleavedDevice(a["cxts"], n, a["blocks"], a["bufs"], a["frames"], a["bufs"], a["caps"], a["ratios"],
                                                           None, a["results"], a["made"]) == 0
    assert L.resampleProcessScheduleBatchPlanarDevice(a["cxts"], n, a["blocks"], a["bufs"], a["pitches"], a["frames"], a["bufs"], a["pitches"],
                                                      a["caps"], a["ratios"], None, a["results"], a["made"]) == 0
    assert L.resampleProcessSchedulePlanarDevice(None, n, None, 1000, None, None, 1000, None, None, 0, None) == 0
    assert L.artamdErrorCount() == errors


@pytest.mark.parametrize("width", WIDTHS)
def test_a_null_context_is_refused_and_not_counted(width):
    L = A.binding(width).lib()
    a = _lists(3)                                    # (every context NULL)
    errors = L.artamdErrorCount()
    assert L.resampleProcessScheduleBatchInterleavedDevice(a["cxts"], 3, a["blocks"], a["bufs"], a["frames"], a["bufs"], a["caps"], a["ratios"],
                                                           None, a["results"], a["made"]) == -1
    assert L.resampleProcessScheduleBatchPlanarDevice(a["cxts"], 3, a["blocks"], a["bufs"], a["pitches"], a["frames"], a["bufs"], a["pitches"],
                                                      a["caps"], a["ratios"], None, a["results"], a["made"]) == -1
    assert L.artamdErrorCount() == errors
    assert list(a["made"]) == [7, 7, 7]              # nothing was touched
