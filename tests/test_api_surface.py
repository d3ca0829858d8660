"""CPU: the Python binding's surface, pinned before its marshalling and clip front end were given one copy each — the public names of
both widths (tests/golden/api_names.txt), the signature of every public callable and of every public method of the object wrappers
(tests/golden/api_signatures.txt), what every module-level batch wrapper does with empty lists and with lists of mismatched length
(each C entry returns at n <= 0 before it looks at a device), the clip classes' front-end refusals on CPU tensors, in their order, and
the section design ClipFilter and ClipBiquad.design share.  The two fixtures are written by `PYTHONPATH=. python tests/test_api_surface.py`."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import audio_resampler_amd as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES, SIGNATURES = os.path.join(GOLDEN, "api_names.txt"), os.path.join(GOLDEN, "api_signatures.txt")
CLASSES = ("Resampler", "Decimator", "BiquadBank", "Stretcher", "ClipResampler", "ClipWarper", "ClipDecimator", "ClipFilter", "ClipBiquad",
           "ClipStretcher")
WIDTHS = [32, 64]


def _names(M):
    return sorted(k for k in vars(M) if not k.startswith("_"))


def _signatures(M):
    """one line per public callable (ctypes types have no signature and are left out) and per public method of CLASSES"""
    lines = []
    for name in _names(M):
        obj = getattr(M, name)
        if not callable(obj) or (isinstance(obj, type) and name not in CLASSES):
            continue
        lines.append(f"{name}{inspect.signature(obj)}")
        if name in CLASSES:
            for attr, member in sorted(vars(obj).items()):
                if (attr in ("__init__", "__call__") or not attr.startswith("_")) and callable(getattr(obj, attr)) and not isinstance(member, property):
                    lines.append(f"{name}.{attr}{inspect.signature(getattr(obj, attr))}")
    # (load_library's default is the build's own library, wherever the package lies or ARTAMD_LIB* points)
    return [re.sub(r"^load_library\(path='[^']*'\)$", "load_library(path=<the build's library>)", line) for line in lines]


@pytest.mark.parametrize("width", WIDTHS)
def test_public_names_are_the_recorded_ones(width):
    assert _names(A.binding(width)) == open(NAMES).read().split()


@pytest.mark.parametrize("width", WIDTHS)
def test_signatures_are_the_recorded_ones(width):
    got, want = _signatures(A.binding(width)), open(SIGNATURES).read().splitlines()
    assert all(c in A.binding(width).__dict__ for c in CLASSES)
    assert got == want, [pair for pair in zip(got, want) if pair[0] != pair[1]][:5]


def test_module_level_is_the_four_byte_binding():
    from audio_resampler_amd import api
    B = A.binding(32)
    for name in _names(B):
        if name != "width":
            assert getattr(api, name) is getattr(B, name), name
            assert getattr(A, name, getattr(B, name)) is getattr(B, name), name      # (the package lists a part of them)


# every module-level batch wrapper with nothing to do: (arguments, what comes back)
EMPTY = {
    "process_batch_device": (([], [], [], [], [], []), []),
    "process_and_flush_batch_device": (([], [], [], [], [], []), []),
    "process_batch_planar_device": (([], [], [], [], [], [], [], []), []),
    "process_and_flush_batch_planar_device": (([], [], None, [], [], None, [], []), []),
    "process_and_flush_clips_planar_device": (([], [], [], [], [], [], [], [], True), []),
    "adjoint_clips_planar_device": (([], [], [], [], [], None, [], []), 0),
    "process_schedule_batch_device": (([], [], [], [], [], [], None), (0, [])),
    "process_schedule_batch_planar_device": (([], [], None, [], [], None, [], [], []), (0, [])),
    "process_schedule_clips_planar_device": (([], [], [], [], [], [], [], [], None, True), (0, [])),
    "adjoint_schedule_clips_planar_device": (([], [], [], [], [], None, [], []), 0),
    "decimate_batch_device": (([], [], [], []), 0),
    "decimate_batch_planar_device": (([], [], None, [], [], []), 0),
    "decimate_clips_planar_device": (([], [], [], [], [], [], True, None), 0),
    "biquad_batch_device": (([], [], []), 0),
    "biquad_batch_planar_device": (([], [], None, []), 0),
    "biquad_clips_planar_device": (([], [], [], [], True), 0),
    "biquad_filter_clips_planar_device": (([], [], None, [], [], [], True), 0),
    "stretch_clips_batch_planar_device": (([], [], None, [], [], [], [], []), []),
    "stretch_clips_logged_batch_planar_device": (([], [], [], [], [], None, [], [], [], []), ([], [])),
    "stretch_adjoint_clips_planar_device": (([], [], [], [], [], [], [], None, []), 0),
    "ingest_batch_device": (([], [], [], [], [], [], []), 0),
    "extrapolate_batch_device": (([], [], [], [], [], [], None), 0),
    "lag_products_batch_device": (([], np.zeros(0, np.int64), [], [], np.zeros(0, np.int32), []), 0),
}


@pytest.mark.parametrize("width", WIDTHS)
def test_every_batch_wrapper_is_in_the_table(width):
    M = A.binding(width)
    wrappers = sorted(k for k in _names(M) if k.endswith("_device") and inspect.isfunction(getattr(M, k)))
    assert wrappers == sorted(EMPTY)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", sorted(EMPTY))
def test_batch_wrapper_with_empty_lists(width, name):
    M = A.binding(width)
    errors = M.lib().artamdErrorCount()
    args, want = EMPTY[name]
    got = getattr(M, name)(*args)
    assert got == want and type(got) is type(want)
    assert M.lib().artamdErrorCount() == errors


class _Ctx:
    """stands for a context in a call that is refused before its address is read"""
    p = None


PER_STREAM, PER_BLOCK = "one entry per stream in every list", "n_ins[i], caps[i] and ratios[i] must have one entry per block"
MISMATCHED = [
    ("process_schedule_batch_device", ([_Ctx()], [0, 0], [[1]], [0], [[1]], [[1.0]]), PER_STREAM),
    ("process_schedule_batch_device", ([_Ctx()], [0], [[1]], [0], [[1]], []), PER_STREAM),
    ("process_schedule_batch_device", ([_Ctx()], [0], [[1, 2]], [0], [[1]], [[1.0, 1.0]]), PER_BLOCK),
    ("process_schedule_batch_planar_device", ([_Ctx()], [0], [0], [[1]], [0, 0], [0], [[1]], [[1.0]]), PER_STREAM),
    ("process_schedule_batch_planar_device", ([_Ctx()], [0], None, [[1]], [0], None, [[1]], [[1.0, 2.0]]), PER_BLOCK),
    ("process_schedule_clips_planar_device", ([_Ctx()], [0], [0], [], [0], [0], [[1]], [[1.0]]), PER_STREAM),
    ("process_schedule_clips_planar_device", ([_Ctx()], [0], [0], [[]], [0], [0], [[1]], [[1.0]], None, True), PER_BLOCK),
    ("adjoint_schedule_clips_planar_device", ([_Ctx()], [0], [0], [5, 5], [0], [0], [[1]], [[1.0]]), "one entry per clip in every list"),
    ("adjoint_schedule_clips_planar_device", ([_Ctx()], [0], [0], [5], [0], [0], [[1, 1]], [[1.0]]),
     "n_ins[i] and ratios[i] must have one entry per block"),
    ("lag_products_batch_device", ([0, 0], [0], [1, 1], [0, 0], [1, 1], [0, 0]), "lag_products_batch_device: one entry per row in every list"),
    ("lag_products_batch_device", (np.zeros(2, np.int64), [0, 0], [1, 1], [0, 0], np.ones(3, np.int32), [0, 0]),
     "lag_products_batch_device: one entry per row in every list"),
]


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name, args, message", MISMATCHED, ids=[f"{m[0]}-{i}" for i, m in enumerate(MISMATCHED)])
def test_batch_wrapper_with_mismatched_lists(width, name, args, message):
    M = A.binding(width)
    with pytest.raises(ValueError) as e:
        getattr(M, name)(*args)
    assert str(e.value) == message


@pytest.mark.parametrize("width", WIDTHS)
def test_single_stream_schedules_check_their_lists(width):
    M = A.binding(width)
    r = object.__new__(M.Resampler)                               # (no context: every call below is answered in front of it)
    r.p, r.L = None, M.lib()
    for call in (lambda n, c, q: r.process_schedule_device(0, n, 0, c, q), lambda n, c, q: r.process_schedule_planar_device(0, 0, n, 0, 0, c, q)):
        for bad in (([1], [], [1.0]), ([1], [1], [1.0, 2.0]), ([], [1], [])):
            with pytest.raises(ValueError) as e:
                call(*bad)
            assert str(e.value) == "n_ins, caps and ratios must have one entry per block"


# ---- the clip classes' front end, on CPU tensors ----

def _clips(M):
    """(name, object, call(x, lengths)) of the six clip classes at two channels"""
    torch = pytest.importorskip("torch")
    dtype = torch.float64 if M.width == 64 else torch.float32
    co = torch.zeros(2, 9, dtype=dtype)
    made = [("ClipResampler", M.ClipResampler(2, 44100, 16000, taps=16, filters=16)), ("ClipWarper", M.ClipWarper(2, taps=16, filters=16, block=10)),
            ("ClipDecimator", M.ClipDecimator(2, 16, 2, 1.0, 44100, 0)), ("ClipFilter", M.ClipFilter(2, [("lowpass", 0.1)])),
            ("ClipBiquad", M.ClipBiquad(2, co)), ("ClipStretcher", M.ClipStretcher(2, 44100))]
    extra = {"ClipWarper": (1.0,), "ClipStretcher": (1.0,)}
    return [(name, obj, (lambda x, lengths=None, obj=obj, more=extra.get(name, ()): obj(x, *more, lengths=lengths))) for name, obj in made], dtype


@pytest.mark.parametrize("width", WIDTHS)
def test_clip_front_end_refusals_on_cpu_tensors(width):
    torch = pytest.importorskip("torch")
    M = A.binding(width)
    clips, dtype = _clips(M)
    other = torch.float32 if width == 64 else torch.float64
    expected = f"expected a CUDA {'float64' if width == 64 else 'float32'} tensor [B, 2, T]"
    for name, obj, call in clips:
        cases = [torch.zeros(25, dtype=dtype), torch.zeros(1, 2, 2, 25, dtype=dtype),          # wrong rank
                 torch.zeros(2, 3, 25, dtype=dtype), torch.zeros(3, 25, dtype=dtype),           # wrong channel count
                 torch.zeros(2, 2, 25, dtype=other), torch.zeros(2, 2, 25, dtype=torch.int16),  # wrong dtype
                 torch.zeros(2, 2, 25, dtype=dtype), torch.zeros(2, 25, dtype=dtype),           # on the CPU
                 torch.zeros(2, 2, 50, dtype=dtype)[:, :, ::2], torch.zeros(0, 2, 25, dtype=dtype)]
        for x in cases:
            with pytest.raises(ValueError) as e:
                call(x)
            assert str(e.value) == expected, (name, tuple(x.shape))
        # bad lengths on a CPU tensor: ClipWarper looks at lengths (and ratios) before it asks for the GPU, the others after
        x = torch.zeros(2, 2, 25, dtype=dtype)
        for bad in ([25], [25, 26], [-1, 25], torch.tensor([1, 2, 3]), np.array([25, 30])):
            with pytest.raises(ValueError) as e:
                call(x, bad)
            assert str(e.value) == ("lengths: one entry per clip, 0 .. T" if name == "ClipWarper" else expected), (name, bad)
        for good in ([25, 0], torch.tensor([3, 25]), np.array([0, 0]), (1.0, 2.9)):
            with pytest.raises(ValueError) as e:
                call(x, good)
            assert str(e.value) == expected, (name, good)
        pools = obj.pools if name == "ClipStretcher" else obj._banks if name == "ClipBiquad" else obj.pool
        assert not pools, name                                     # (no context was made on the way to a refusal)


@pytest.mark.parametrize("width", WIDTHS)
def test_clip_warper_refusals_come_in_their_order(width):
    torch = pytest.importorskip("torch")
    M = A.binding(width)
    dtype = torch.float64 if width == 64 else torch.float32
    w = M.ClipWarper(2, taps=16, filters=16, block=10)
    x = torch.zeros(2, 2, 25, dtype=dtype)
    grad = "ClipWarper: ratios that require grad: the ratio curve has no gradient (it would silently be zero)"
    shape = "ratios: a scalar, [B] or [B, K] with K >= ceil(max(lengths) / block)"
    for ratios, lengths, message in ((torch.ones(2, 3, requires_grad=True), None, grad), (torch.ones(2, 2, requires_grad=True), None, grad),
                                     (torch.ones(2, 3, requires_grad=True), [25, 26], "lengths: one entry per clip, 0 .. T"),
                                     (np.ones((2, 2)), None, shape), (np.ones((3, 3)), None, shape), (np.ones((2, 2)), [20, 3], None),
                                     ([1.0, 0.0], None, "ratios must be finite and > 0"), (float("nan"), None, "ratios must be finite and > 0")):
        with pytest.raises(ValueError) as e:
            w(x, ratios, lengths=lengths)
        assert str(e.value) == (message or f"expected a CUDA {'float64' if width == 64 else 'float32'} tensor [B, 2, T]")
    with pytest.raises(ValueError) as e:                          # (the shape of x comes first of all)
        w(torch.zeros(2, 3, 25, dtype=dtype), torch.ones(2, 3, requires_grad=True))
    assert str(e.value).startswith("expected a CUDA")
    assert w.pool == []


@pytest.mark.parametrize("width", WIDTHS)
def test_sections_are_checked_and_designed_once_for_both_classes(width):
    torch = pytest.importorskip("torch")
    M = A.binding(width)
    L = M.lib()
    message = 'sections: one to four of ("lowpass" | "highpass", frequency)'
    low = ("lowpass", 0.1)
    for bad in ([], [low] * 5, [("bandpass", 0.1)], [low, ("notch", 0.2)], iter([])):
        for make in (lambda s: M.ClipFilter(2, s), M.ClipBiquad.design):
            with pytest.raises(ValueError) as e:
                make(bad)
            assert str(e.value) == message
    sections = [("lowpass", 0.05), ("highpass", 0.2), ("lowpass", 0.31), ("highpass", 0.004)]
    for count in (1, 2, 4):
        part = sections[:count]
        want = []
        for kind, freq in part:
            co = M.BiquadCoefficients()
            (L.biquad_lowpass if kind == "lowpass" else L.biquad_highpass)(C.byref(co), float(freq))
            want.append(co)
        rows = M.ClipBiquad.design(iter(part))                    # (any iterable, read once)
        assert rows.dtype == (torch.float64 if width == 64 else torch.float32) and tuple(rows.shape) == (count, 9) and not rows.is_cuda
        assert rows.numpy().tobytes() == b"".join(bytes(co) for co in want)
        f = M.ClipFilter(3, iter(part), max_batch=0)
        assert (f.channels, f.nsections, f.max_batch, f.pool, f.launches) == (3, count, 1, [], 0)
        bank = (M.Biquad * (3 * count))()
        for c in range(3):
            for s in range(count):
                L.biquad_init(C.byref(bank[c * count + s]), C.byref(want[s]), 1.0)
        assert bytes(f._sections) == bytes(bank)


if __name__ == "__main__":                                        # records the two fixtures from the binding as it stands
    assert _names(A.binding(32)) == _names(A.binding(64)) and _signatures(A.binding(32)) == _signatures(A.binding(64))
    open(NAMES, "w").write("\n".join(_names(A.binding(32))) + "\n")
    open(SIGNATURES, "w").write("\n".join(_signatures(A.binding(32))) + "\n")
