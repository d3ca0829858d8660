"""CPU: artamdLagProductsBatchDevice — exported by both libraries, declared in art_hip.h as the issue's prototype, listed in
EXPORTED_SYMBOLS and wrapped (lag_products_batch_device; ClipBiquad's backward calls it); its refusals need no device; its kernels
are in both libraries under names of their own, use no scratch and spill nothing; and ClipBiquad.design gives biquad_lowpass /
biquad_highpass's values without a GPU, in both widths."""
import ctypes as C
import os
import re

import pytest

import audio_resampler_amd as A
import test_matrix_batch_abi as T
from test_matrix_batch_abi import _kernel_notes

PKG = os.path.dirname(os.path.abspath(A.__file__))
LIB32, LIB64 = os.path.join(PKG, "libartamd.so"), os.path.join(PKG, "libartamd64.so")
NAME = "artamdLagProductsBatchDevice"
KERNELS = ("lag_products_tile_kernel", "lag_products_finish_kernel")
PINNED = ("biquad_", "bq_clips_", "bq_filter_", "copy_rows_group_kernel", "fir_", "ingest_", "decimate_", "stretch_", "extrap")


def _header():
    text = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("width", [32, 64])
def test_symbol_is_exported_listed_and_wrapped(width):
    B = A.binding(width)
    assert hasattr(B.lib(), NAME)
    assert NAME in B.EXPORTED_SYMBOLS and NAME in A.EXPORTED_SYMBOLS
    res, argtypes = B.EXPORTED_SYMBOLS[NAME]
    assert res is C.c_int and argtypes == [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    for M in (A, B):
        assert callable(M.lag_products_batch_device) and isinstance(M.ClipBiquad, type)
    # the tile length the determinism contract speaks of is readable (the GPU tests build their frame counts from it)
    tile = B.lib().artamd_lag_products_tile
    tile.restype, tile.argtypes = C.c_int, []
    assert tile() >= 256 and "artamd_lag_products_tile" not in _header()


def test_declaration_is_the_contracts():
    text = _header()
    m = re.search(r"#define\s+ARTAMD_LAG_PRODUCTS_MAX\s+(\d+)", text)
    assert m and int(m.group(1)) == 8
    decl = re.search(r"\bint\s+" + NAME + r"\s*\(([^;{}]*)\)\s*;", text)
    assert decl, "not declared"
    assert " ".join(decl.group(1).split()) == (
        "const artsample_t *const *d_u, const artsample_t *const *d_v, const int *numFrames, const int *firstLags, "
        "const int *numLags, double *const *d_sums, int n, void *hipStream")
    raw = open(os.path.join(os.path.dirname(PKG), "include", "art_hip.h")).read()
    comment = raw[:raw.index("int " + NAME)].rsplit("/*", 1)[1]
    for word in ("SET", "ascending tile order", "alignment", "artamdErrorCount", "skipped"):
        assert word in comment, word


def _call(L, rows, n=None):
    """rows: (u, v, frames, first, lags, sums)"""
    k = max(len(rows), 1)
    col = lambda j, t: (t * k)(*[r[j] for r in rows])
    return getattr(L, NAME)(col(0, C.c_void_p), col(1, C.c_void_p), col(2, C.c_int), col(3, C.c_int), col(4, C.c_int), col(5, C.c_void_p),
                            len(rows) if n is None else n, None)


@pytest.mark.parametrize("width", [32, 64])
def test_refusals_need_no_device(width):
    """these calls never reach a device, so they answer the same with or without one, and none is counted"""
    L = A.binding(width).lib()
    fn = getattr(L, NAME)
    errors = L.artamdErrorCount()
    assert fn(None, None, None, None, None, None, 0, None) == 0
    assert fn(None, None, None, None, None, None, -3, None) == 0
    fake = 0x10000
    skipped = (None, None, 0, -1, 0, None)                       # (a row without frames may have anything in its place)
    assert _call(L, [skipped, (fake, fake, -5, 9, 9, fake)]) == 0
    bad = {"NULL u": (None, fake, 10, 0, 5, fake), "NULL v": (fake, None, 10, 0, 5, fake), "NULL sums": (fake, fake, 10, 0, 5, None),
           "negative first lag": (fake, fake, 10, -1, 4, fake), "zero lags": (fake, fake, 10, 0, 0, fake),
           "first + num > 8": (fake, fake, 10, 4, 5, fake), "9 lags": (fake, fake, 10, 0, 9, fake),
           "overflowing lags": (fake, fake, 10, 2, 2 ** 31 - 1, fake)}
    for what, row in bad.items():
        assert _call(L, [skipped, row]) == -1, what
        assert _call(L, [row, skipped]) == -1, what
    assert fn(None, None, None, None, None, None, 1, None) == -1
    assert L.artamdErrorCount() == errors
    with pytest.raises(RuntimeError):
        A.binding(width).lag_products_batch_device([fake], [fake], [10], [4], [5], [fake])
    with pytest.raises(ValueError):
        A.binding(width).lag_products_batch_device([fake], [fake], [10, 10], [0], [5], [fake])
    assert L.artamdErrorCount() == errors


def test_kernels_are_in_both_libraries_under_names_of_their_own():
    for path in (LIB32, LIB64):
        blob = open(path, "rb").read()
        for k in KERNELS:
            assert k.encode() in blob, (path, k)
    for k in KERNELS:
        assert not any(p in k for p in PINNED), k


@pytest.mark.parametrize("width", [32, 64])
def test_kernels_use_no_scratch_and_spill_nothing(tmp_path, monkeypatch, width):
    if width == 64:
        monkeypatch.setattr(T, "LIB32", LIB64)
    notes = _kernel_notes(tmp_path)
    new = {s: f for s, f in notes.items() if "lag_products" in s}
    assert len(new) == len(KERNELS) and all(any(k in s for s in new) for k in KERNELS), sorted(new)
    for s, f in sorted(new.items()):
        print(s, {k: f.get(k) for k in ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
                                        "vgpr_spill_count", "sgpr_spill_count")})
        assert int(f["private_segment_fixed_size"]) == 0, (s, f)
        assert int(f.get("vgpr_spill_count", 0)) == 0 and int(f.get("sgpr_spill_count", 0)) == 0, (s, f)


@pytest.mark.parametrize("width", [32, 64])
def test_design_needs_no_gpu_and_gives_the_librarys_values(width):
    import torch
    B = A.binding(width)
    sections = [("lowpass", 0.2), ("highpass", 0.02), ("lowpass", 44100 * 0.45 / 96000)]
    co = B.ClipBiquad.design(sections)
    assert co.shape == (3, 9) and co.dtype == (torch.float64 if width == 64 else torch.float32) and not co.is_cuda
    for row, (kind, freq) in zip(co.tolist(), sections):
        want = B.BiquadCoefficients()
        (B.lib().biquad_lowpass if kind == "lowpass" else B.lib().biquad_highpass)(C.byref(want), freq)
        assert row == [getattr(want, n) for n in ("a0", "a1", "a2", "a3", "a4", "b1", "b2", "b3", "b4")]
        assert any(row[:5]) and any(row[5:])
    for wrong in ([], [("lowpass", 0.1)] * 5, [("bandpass", 0.1)]):
        with pytest.raises(ValueError):
            B.ClipBiquad.design(wrong)
    # the constructor's checks need no GPU either
    with pytest.raises(ValueError):
        B.ClipBiquad(2, torch.zeros(5, 9, dtype=co.dtype))
    with pytest.raises(ValueError):
        B.ClipBiquad(2, torch.zeros(3, 2, 9, dtype=co.dtype))
    with pytest.raises(ValueError):
        B.ClipBiquad(2, torch.zeros(2, 9, dtype=torch.float64 if width == 32 else torch.float32))
    B.ClipBiquad(2, co).close()
