"""ctypes mirror of include/{resampler,biquad,decimator,art_hip}.h.

`lib()` returns the loaded libartamd.so with argtypes set (`wide().lib()`: libartamd64.so, 8-byte samples); the functions keep the reference's names
(resampleInit, resampleProcessInterleaved, biquad_apply_buffer, decimateProcessInterleavedLE, ...).
`Resampler` / `Decimator` / `BiquadBank` are thin object wrappers used by tests and bench.py.
There is no fallback: if the library is missing or no GPU is present the constructors raise.
"""
import ctypes as C
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# resampler.h flags
SUBSAMPLE_INTERPOLATE, BLACKMAN_HARRIS, INCLUDE_LOWPASS, RESAMPLE_MULTITHREADED, NO_FILTER_REDUCTION = 0x1, 0x2, 0x4, 0x8, 0x10
RESAMPLE_FIXED_RATIO, EXTRAPOLATE_ENDPOINTS, EXTRAPOLATE_PREFILL, EXTEND_CONVOLUTION_MATH = 0x20, 0x40, 0x80, 0x100
RESAMPLER_FLUSHED, RESAMPLER_SNAP_OFFSET, RESAMPLE_STRICT_ORDER = 0x200, 0x400, 0x10000
# decimator.h flags
DITHER_HIGHPASS, DITHER_FLAT, DITHER_LOWPASS = 0x1, 0x2, 0x4
SHAPING_1ST_ORDER, SHAPING_2ND_ORDER, SHAPING_3RD_ORDER, SHAPING_ATH_CURVE = 0x100, 0x200, 0x400, 0x800
DECIMATE_MULTITHREADED = 0x1000
# stretch.h flags
STRETCH_FAST_FLAG, STRETCH_DUAL_FLAG = 0x1, 0x2

def _bind(width):
    """everything below exists once per sample width: 32 (libartamd.so, float) and 64 (libartamd64.so, double —
    the reference's PATH_WIDTH=64 builds, reference resampler.h:22-26)"""
    smp_c = C.c_double if width == 64 else C.c_float            # artsample_t of this build
    smp_np = np.float64 if width == 64 else np.float32
    smp_torch = "float64" if width == 64 else "float32"         # torch dtype name for device tensors
    LIB_PATH = os.environ.get("ARTAMD_LIB64" if width == 64 else "ARTAMD_LIB") or \
        os.path.join(HERE, "libartamd64.so" if width == 64 else "libartamd.so")     # ARTAMD_LIB*: A/B of two builds only
    f32p = C.POINTER(smp_c)                                      # (name kept from the 4-byte build)
    u8p = C.POINTER(C.c_ubyte)


    class ResampleResult(C.Structure):
        _fields_ = [("input_used", C.c_uint), ("output_generated", C.c_uint)]


    class Resample(C.Structure):
        _fields_ = [("numChannels", C.c_int), ("numSamples", C.c_int), ("numFilters", C.c_int), ("numTaps", C.c_int),
                    ("inputIndex", C.c_int), ("flags", C.c_int), ("tempFilter", C.c_void_p),
                    ("outputOffset", C.c_double), ("fixedRatio", C.c_double), ("lowpassRatio", C.c_double),
                    ("subsample", C.c_void_p), ("buffers", C.c_void_p), ("filters", C.POINTER(f32p)), ("hip", C.c_void_p)]


    class BiquadCoefficients(C.Structure):
        _fields_ = [(n, smp_c) for n in ("a0", "a1", "a2", "a3", "a4", "b1", "b2", "b3", "b4")]


    class Biquad(C.Structure):
        _fields_ = [("a", smp_c * 5), ("b", smp_c * 5), ("x", smp_c * 4), ("y", smp_c * 4),
                    ("order", C.c_int), ("index", C.c_int)]


    class Decimate(C.Structure):
        _fields_ = [("numChannels", C.c_int), ("outputBits", C.c_int), ("outputBytes", C.c_int), ("dither_type", C.c_int),
                    ("flags", C.c_int), ("outputGain", C.c_double), ("feedback", f32p), ("tpdf_generators", C.POINTER(C.c_uint32)),
                    ("noise_shapers", C.POINTER(Biquad)), ("hip", C.c_void_p)]


    class ArtamdSegment(C.Structure):
        _fields_ = [("first_output", C.c_uint), ("lin_base", C.c_int), ("base_offset", C.c_double)]


    class ArtamdPosition(C.Structure):
        _fields_ = [("numTaps", C.c_int), ("numFilters", C.c_int), ("flags", C.c_int), ("inputIndex", C.c_int),
                    ("floorActive", C.c_int), ("outputOffset", C.c_double), ("fixedRatio", C.c_double)]


    RP, DP = C.POINTER(Resample), C.POINTER(Decimate)
    ptr = C.c_void_p      # device pointers travel as plain addresses

    # every symbol the public headers declare: name -> (restype, argtypes)
    EXPORTED_SYMBOLS = {
        # resampler.h
        "resampleInit": (RP, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]),
        "resampleFixedRatioInit": (RP, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]),
        "resampleProcess": (ResampleResult, [RP, C.POINTER(f32p), C.c_int, C.POINTER(f32p), C.c_int, C.c_double]),
        "resampleProcessInterleaved": (ResampleResult, [RP, f32p, C.c_int, f32p, C.c_int, C.c_double]),
        "resampleProcessAndFlush": (ResampleResult, [RP, C.POINTER(f32p), C.c_int, C.POINTER(f32p), C.c_int, C.c_double]),
        "resampleProcessAndFlushInterleaved": (ResampleResult, [RP, f32p, C.c_int, f32p, C.c_int, C.c_double]),
        "resampleGetRequiredSamples": (C.c_uint, [RP, C.c_int, C.c_double]),
        "resampleGetExpectedOutput": (C.c_uint, [RP, C.c_int, C.c_double]),
        "resampleAdvancePosition": (None, [RP, C.c_double]),
        "resampleGetLowpassRatio": (C.c_double, [RP]),
        "resampleGetPosition": (C.c_double, [RP]),
        "resampleGetNumFilters": (C.c_int, [RP]),
        "resampleInterpolationUsed": (C.c_int, [RP]),
        "resampleReset": (None, [RP]),
        "resampleFree": (None, [RP]),
        # biquad.h
        "biquad_init": (None, [C.POINTER(Biquad), C.POINTER(BiquadCoefficients), C.c_double]),
        "biquad_lowpass": (None, [C.POINTER(BiquadCoefficients), C.c_double]),
        "biquad_highpass": (None, [C.POINTER(BiquadCoefficients), C.c_double]),
        "biquad_apply_buffer": (None, [C.POINTER(Biquad), f32p, C.c_int, C.c_int]),
        "biquad_apply_sample": (smp_c, [C.POINTER(Biquad), smp_c]),
        # decimator.h
        "floatIntegersLE": (None, [u8p, C.c_double, C.c_int, C.c_int, C.c_int, f32p, C.c_int]),
        "decimateInit": (DP, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]),
        "decimateProcessLE": (C.c_int, [DP, C.POINTER(f32p), C.c_int, C.POINTER(u8p)]),
        "decimateProcessInterleavedLE": (C.c_int, [DP, f32p, C.c_int, u8p]),
        "decimateFree": (None, [DP]),
        # art_hip.h
        "artamdDeviceCount": (C.c_int, []),
        "artamdDeviceAlloc": (ptr, [C.c_size_t]),
        "artamdDeviceFree": (None, [ptr]),
        "artamdUpload": (C.c_int, [ptr, ptr, C.c_size_t, ptr]),
        "artamdDownload": (C.c_int, [ptr, ptr, C.c_size_t, ptr]),
        "artamdDeviceZero": (C.c_int, [ptr, C.c_size_t, ptr]),
        "artamdStreamSynchronize": (C.c_int, [ptr]),
        "artamdVersion": (C.c_char_p, []),
        "artamdSetDevices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
        "resampleHipGetDevice": (C.c_int, [RP]),
        "resampleHipNumShards": (C.c_int, [RP]),
        "resampleHipShardInfo": (C.c_int, [RP, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "resampleHipSetStream": (None, [RP, ptr]),
        "resampleHipSynchronize": (None, [RP]),
        "resampleHipSetKernel": (None, [RP, C.c_int]),
        "resampleHipKeepRows": (None, [RP, C.c_int]),
        "resampleHipSetCutInvariant": (None, [RP, C.c_int]),
        "resampleHipCutInvariantFallbacks": (C.c_uint, [RP]),
        "resampleHipLastKernel": (C.c_int, [RP]),
        "resampleHipLastGathered": (C.c_int, [RP]),
        "resampleHipLastHandedBack": (C.c_uint, [RP]),
        "resampleHipLastFixedPoint": (C.c_int, [RP, C.POINTER(C.c_double)]),
        "resampleHipLastFixedPointKernel": (C.c_int, [RP]),
        "resampleHipSetTiming": (None, [RP, C.c_int]),
        "resampleHipReadTiming": (C.c_double, [RP, C.POINTER(C.c_int)]),
        "resampleHipReadPrepTiming": (C.c_double, [RP]),
        "resampleProcessInterleavedDevice": (ResampleResult, [RP, ptr, C.c_int, ptr, C.c_int, C.c_double]),
        "resampleProcessAndFlushInterleavedDevice": (ResampleResult, [RP, ptr, C.c_int, ptr, C.c_int, C.c_double]),
        "resampleProcessPlanarDevice": (ResampleResult, [RP, ptr, C.c_long, C.c_int, ptr, C.c_long, C.c_int, C.c_double]),
        "artamdBuildFilterBank": (None, [C.c_int, C.c_int, C.c_double, C.c_int, f32p]),
        "artamdPlanCall": (C.c_int, [C.POINTER(ArtamdPosition), C.c_int, C.c_int, C.c_double, C.POINTER(ResampleResult),
                                     C.POINTER(ArtamdSegment), C.c_int, C.POINTER(C.c_int)]),
        "biquadBankCreate": (ptr, [C.POINTER(Biquad), C.c_int, C.c_int]),
        "biquadBankCreateMulti": (ptr, [C.POINTER(Biquad), C.c_int, C.c_int]),
        "biquadBankShardCount": (C.c_int, [ptr]),
        "biquadBankSetStream": (None, [ptr, ptr]),
        "biquadBankApplyInterleavedDevice": (None, [ptr, ptr, C.c_int]),
        "biquadBankRead": (None, [ptr, C.POINTER(Biquad)]),
        "biquadBankFree": (None, [ptr]),
        "biquadBankRepairs": (C.c_uint, [ptr]),
        "artamdBiquadRepairs": (C.c_uint, []),
        "biquadBankApplyBatchInterleavedDevice": (C.c_int, [ptr, C.c_int, ptr, ptr]),
        "biquadBankApplyPlanarDevice": (None, [ptr, ptr, C.c_long, C.c_int]),
        "biquadBankApplyBatchPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr]),
        "biquadBankApplyClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, C.c_int]),
        "biquadBankFilterClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, C.c_int]),
        "biquadBankReset": (None, [ptr]),
        "decimateHipSetStream": (None, [DP, ptr]),
        "decimateProcessInterleavedLEDevice": (None, [DP, ptr, C.c_int, ptr]),
        "decimateHipClipped": (C.c_long, [DP]),
        "decimateHipShardCount": (C.c_int, [DP]),
        "decimateProcessBatchInterleavedLEDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr]),
        "decimateProcessPlanarLEDevice": (None, [DP, ptr, C.c_long, C.c_int, ptr, C.c_long]),
        "decimateProcessBatchPlanarLEDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr]),
        "decimateHipReset": (None, [DP]),
        "decimateProcessClipsPlanarLEDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, C.c_int, ptr]),
        "artamdErrorCount": (C.c_int, []),
        "artamdPeriodMultiple": (C.c_int, [C.c_int]),
        "artamdPeriodMultipleRows": (C.c_int, [C.c_int, C.c_int]),
        "artamdLastError": (C.c_char_p, []),
        "floatIntegersLEDevice": (None, [ptr, C.c_double, C.c_int, C.c_int, C.c_int, ptr, C.c_int, ptr]),
        "floatIntegersBatchLEDevice": (C.c_int, [ptr, ptr, ptr, ptr, ptr, ptr, ptr, C.c_int, ptr]),
        "artamdExtrapolateBatchDevice": (C.c_int, [ptr, ptr, ptr, ptr, ptr, ptr, C.c_int, ptr]),
        "artamdLagProductsBatchDevice": (C.c_int, [ptr, ptr, ptr, ptr, ptr, ptr, C.c_int, ptr]),
        # stretch.h
        "stretchInit": (ptr, [C.c_int, C.c_int, C.c_int, C.c_int]),
        "stretchGetOutputCapacity": (C.c_int, [ptr, C.c_int, C.c_double]),
        "stretchProcess": (C.c_int, [ptr, f32p, C.c_int, f32p, C.c_double]),
        "stretchFlush": (C.c_int, [ptr, f32p]),
        "stretchReset": (None, [ptr]),
        "stretchFree": (None, [ptr]),
        "stretchHipSetStream": (None, [ptr, ptr]),
        "stretchProcessDevice": (C.c_int, [ptr, ptr, C.c_int, ptr, C.c_double]),
        "stretchFlushDevice": (C.c_int, [ptr, ptr]),
        "resampleProcessBatchInterleavedDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleProcessAndFlushBatchInterleavedDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleProcessScheduleInterleavedDevice": (C.c_int, [RP, C.c_int, ptr, ptr, ptr, ptr, ptr, C.c_int, ptr]),
        "stretchProcessBatchDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr]),
        "stretchFlushBatchDevice": (C.c_int, [ptr, C.c_int, ptr, ptr]),
        "resampleProcessAndFlushPlanarDevice": (ResampleResult, [RP, ptr, C.c_long, C.c_int, ptr, C.c_long, C.c_int, C.c_double]),
        "resampleProcessBatchPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleProcessAndFlushBatchPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleProcessAndFlushClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, C.c_int, ptr]),
        "resampleAdjointClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "stretchProcessAndFlushBatchPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, C.c_int, ptr]),
        "artamdStretchClipCapacity": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double]),
        "artamdStretchLogCapacity": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]),
        "stretchProcessAndFlushLoggedBatchPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "stretchAdjointClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleProcessSchedulePlanarDevice": (C.c_int, [RP, C.c_int, ptr, C.c_long, ptr, ptr, C.c_long, ptr, ptr, C.c_int, ptr]),
        "resampleProcessScheduleBatchInterleavedDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleProcessScheduleBatchPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleProcessScheduleClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, C.c_int, ptr, ptr]),
        "resampleAdjointScheduleClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleRateGradientScheduleClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleSampleClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleSampleAdjointClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleSamplePositionGradientClipsPlanarDevice": (C.c_int, [ptr, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleSampleBandClipsPlanarDevice": (C.c_int, [ptr, C.c_int, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleSampleBandAdjointClipsPlanarDevice": (C.c_int, [ptr, C.c_int, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
        "resampleSampleBandGradientsClipsPlanarDevice": (C.c_int, [ptr, C.c_int, C.c_int, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr]),
    }

    _state = {"lib": None}


    def load_library(path=LIB_PATH):
        if _state["lib"] is None:
            # torch bundles its own HIP runtime; whichever libamdhip64 is loaded first owns the process.
            # Import torch first so that device memory, streams and RCCL handed in from torch and the
            # kernels launched by libartamd.so live in ONE runtime (set ARTAMD_NO_TORCH=1 for torch-free use).
            if not os.environ.get("ARTAMD_NO_TORCH"):
                try:
                    import torch  # noqa: F401
                except Exception:
                    pass
            if not os.path.exists(path):
                raise RuntimeError(f"{path} is missing — build it with `python -m audio_resampler_amd.build` "
                                   "(there is no CPU fallback)")
            L = C.CDLL(path)
            for name, (res, args) in EXPORTED_SYMBOLS.items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = res, args
            _state["lib"] = L
        return _state["lib"]


    def lib():
        return load_library()


    def _np_f32(a):
        return np.ascontiguousarray(a, dtype=smp_np)


    def _dev_ptr(t):
        """address of a torch CUDA tensor (or a raw int)."""
        return t if isinstance(t, int) else int(t) if isinstance(t, np.integer) else (t.data_ptr() if t is not None else None)

    # -- the argument arrays of the batch entries: each takes a list or a numpy array and the entry's item count (a longer list raises
    #    IndexError, a shorter one is filled with zeros); a wrapper below is these, its C call and its return convention --
    def _contexts(objs, n):
        """void *[n] of the contexts of objects with .p (a typed pointer, an address or None)"""
        return (C.c_void_p * n)(*[p if type(p) is int or p is None else C.c_void_p.from_buffer(p).value for p in [o.p for o in objs]])

    def _dev_ptrs(v, n):
        """void *[n] of device addresses: tensors, ints or None"""
        return (C.c_void_p * n)(*(v.tolist() if isinstance(v, np.ndarray) else map(_dev_ptr, v)))

    def _ints(v, n):
        return (C.c_int * n)(*map(int, v.tolist() if isinstance(v, np.ndarray) else v))

    def _longs(v, n):
        """long[n], or None for None (a pitch list: every item interleaved)"""
        return None if v is None else (C.c_long * n)(*map(int, v.tolist() if isinstance(v, np.ndarray) else v))

    def _doubles(v, n):
        return (C.c_double * n)(*map(float, v.tolist() if isinstance(v, np.ndarray) else v))

    def _rows(ctype, convert, lists):
        """a ctypes array per item of `lists` (never of no element), to go into a _table"""
        return [(ctype * max(len(v), 1))(*map(convert, v)) for v in lists]

    def _flat(pairs):
        return [v for pair in pairs for v in pair]

    def _table(arrays, n):
        """void *[n] of the addresses of per-item ctypes arrays (which the caller keeps alive)"""
        return (C.c_void_p * n)(*map(C.addressof, arrays))

    def _raw_stream(stream):
        """a torch stream, a raw address or None (the null stream) as the address the entries take"""
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else stream

    def _results(res, n):
        return [(res[k].input_used, res[k].output_generated) for k in range(n)]


    class Resampler:
        """Object wrapper over the C API.  Host arrays are numpy [frames, channels] (interleaved);
        device tensors are torch float32 CUDA tensors of the same shape."""

        def __init__(self, channels, taps, filters, lowpass_ratio=0.0, flags=BLACKMAN_HARRIS | SUBSAMPLE_INTERPOLATE, fixed=None):
            L = lib()
            if fixed is None:
                self.p = L.resampleInit(channels, taps, filters, lowpass_ratio, flags)
            else:
                src, dst, lowpass_freq = fixed
                self.p = L.resampleFixedRatioInit(channels, taps, filters, float(src), float(dst), int(lowpass_freq), flags)
            if not self.p:
                raise RuntimeError("resampleInit failed (bad parameters, or no MI355X visible — there is no CPU path)")
            self.channels = channels
            self.L = L

        def close(self):
            if getattr(self, "p", None):
                self.L.resampleFree(self.p)
                self.p = None

        __del__ = close

        @property
        def c(self):
            return self.p.contents

        def state(self):
            c = self.c
            return (np.float64(c.outputOffset).view(np.uint64).item(), c.inputIndex, c.flags & 0xffff)

        def bank(self):
            c = self.c
            return np.stack([np.ctypeslib.as_array(c.filters[i], shape=(c.numTaps,)).copy() for i in range(c.numFilters + 1)])

        def advance(self, delta):
            self.L.resampleAdvancePosition(self.p, delta)

        def reset(self):
            self.L.resampleReset(self.p)

        def position(self):
            return self.L.resampleGetPosition(self.p)

        def set_stream(self, stream_ptr):
            self.L.resampleHipSetStream(self.p, stream_ptr)

        def shards(self):
            """[(device, first_channel, channels), ...] of a RESAMPLE_MULTITHREADED context spread over devices; [] otherwise"""
            out = []
            for k in range(self.L.resampleHipNumShards(self.p)):
                d, f, n = C.c_int(), C.c_int(), C.c_int()
                self.L.resampleHipShardInfo(self.p, k, C.byref(d), C.byref(f), C.byref(n))
                out.append((d.value, f.value, n.value))
            return out

        def set_kernel(self, which):
            self.L.resampleHipSetKernel(self.p, which)

        def set_cut_invariant(self, on=True):
            """the cut-invariant stream policy (art_hip.h): one arithmetic per stream, the same bits for any cut of the input into calls"""
            self.L.resampleHipSetCutInvariant(self.p, 1 if on else 0)

        def cut_invariant_fallbacks(self):
            return self.L.resampleHipCutInvariantFallbacks(self.p)

        def keep_rows(self, on):
            self.L.resampleHipKeepRows(self.p, 1 if on else 0)

        def last_kernel(self):
            return self.L.resampleHipLastKernel(self.p)

        def last_gathered(self):
            return self.L.resampleHipLastGathered(self.p)

        def synchronize(self):
            self.L.resampleHipSynchronize(self.p)

        def fixed_point(self):
            """(state, pairs): state 0 = the last call's FIR was not the fixed-point matrix kernel, 1 = it was, 2 = it stood down
            for the f32 kernel; pairs = digit-pair products per 32-tap chunk (9..13)"""
            pairs = C.c_double(0.0)
            state = self.L.resampleHipLastFixedPoint(self.p, C.byref(pairs))
            return state, pairs.value

        def fixed_point_kernel(self):
            """the form of the fixed-point kernel the last call's last launch was given to (art_hip.h), as its name; None: not fixed point"""
            return {1: "fir_i8_stream_kernel", 2: "fir_i8_dma_kernel", 3: "fir_i8_slab_kernel"}.get(self.L.resampleHipLastFixedPointKernel(self.p))

        def handed_back(self):
            return self.L.resampleHipLastHandedBack(self.p)

        def set_timing(self, on=True):
            self.L.resampleHipSetTiming(self.p, int(on))

        def read_timing(self):
            """(total FIR-kernel milliseconds, launches) since timing was enabled / last read"""
            n = C.c_int()
            ms = self.L.resampleHipReadTiming(self.p, C.byref(n))
            return ms, n.value

        def read_prep_timing(self):
            """milliseconds the launches of the last read_timing() spent before their dominant kernel (table / staging passes)"""
            return self.L.resampleHipReadPrepTiming(self.p)

        # -- host-pointer API (numpy) --
        def process(self, x, out_cap, ratio, flush=False, and_flush=False, threads=1):
            out = np.zeros((out_cap, self.channels), smp_np)
            op = out.ctypes.data_as(f32p)
            if flush:
                r = self.L.resampleProcessInterleaved(self.p, None, -1, op, out_cap, ratio)
            else:
                x = _np_f32(x)
                fn = self.L.resampleProcessAndFlushInterleaved if and_flush else self.L.resampleProcessInterleaved
                r = fn(self.p, x.ctypes.data_as(f32p), x.shape[0], op, out_cap, ratio)
            return r.input_used, r.output_generated, out[:r.output_generated]

        def process_planar(self, planes, out_cap, ratio, flush=False, and_flush=False):
            """planes: list of C float32 arrays [frames]; returns (used, generated, [C arrays])."""
            Cn = self.channels
            outs = [np.zeros(out_cap, smp_np) for _ in range(Cn)]
            op = (f32p * Cn)(*[o.ctypes.data_as(f32p) for o in outs])
            if flush:
                r = self.L.resampleProcess(self.p, None, -1, op, out_cap, ratio)
            else:
                planes = [_np_f32(p) for p in planes]
                ip = (f32p * Cn)(*[p.ctypes.data_as(f32p) for p in planes])
                fn = self.L.resampleProcessAndFlush if and_flush else self.L.resampleProcess
                r = fn(self.p, ip, len(planes[0]), op, out_cap, ratio)
            return r.input_used, r.output_generated, [o[:r.output_generated] for o in outs]

        # -- device-pointer API (torch tensors or raw addresses); asynchronous --
        def process_device(self, d_in, n_in, d_out, out_cap, ratio, and_flush=False):
            fn = self.L.resampleProcessAndFlushInterleavedDevice if and_flush else self.L.resampleProcessInterleavedDevice
            r = fn(self.p, _dev_ptr(d_in), n_in, _dev_ptr(d_out), out_cap, ratio)
            return r.input_used, r.output_generated

        def _schedule(self, name, d_in, n_ins, d_out, caps, ratios, flush_last, pitches=None):
            """the two schedule entries: the planar one takes a pitch behind each buffer"""
            n = len(n_ins)
            if len(caps) != n or len(ratios) != n:
                raise ValueError("n_ins, caps and ratios must have one entry per block")
            m = max(n, 1)
            res = (ResampleResult * m)()
            side = lambda d, k: (_dev_ptr(d),) if pitches is None else (_dev_ptr(d), int(pitches[k]))
            rc = getattr(self.L, name)(self.p, n, *side(d_in, 0), _ints(n_ins, m), *side(d_out, 1), _ints(caps, m), _doubles(ratios, m),
                                       1 if flush_last else 0, res)
            if rc < 0:
                raise RuntimeError(name + " failed")
            return rc, _results(res, n)

        def process_schedule_device(self, d_in, n_ins, d_out, caps, ratios, flush_last=False):
            """resampleProcessScheduleInterleavedDevice: blocks k = 0, 1, ... of this stream, contiguous in d_in, outputs packed in d_out
            (which holds sum(caps) frames).  Returns (blocks_made, [(input_used, output_generated), ...]); raises if a launch failed."""
            return self._schedule("resampleProcessScheduleInterleavedDevice", d_in, n_ins, d_out, caps, ratios, flush_last)

        def process_schedule_planar_device(self, d_in, in_pitch, n_ins, d_out, out_pitch, caps, ratios, flush_last=False):
            """resampleProcessSchedulePlanarDevice: process_schedule_device on channels-first buffers (pitches in samples, 0: that side
            interleaved): the blocks follow one another along every input plane, the outputs are packed along every output plane.
            Returns (blocks_made, [(input_used, output_generated), ...]); raises if a launch failed."""
            return self._schedule("resampleProcessSchedulePlanarDevice", d_in, n_ins, d_out, caps, ratios, flush_last, (in_pitch, out_pitch))

        def process_planar_device(self, d_in, in_pitch, n_in, d_out, out_pitch, out_cap, ratio):
            r = self.L.resampleProcessPlanarDevice(self.p, _dev_ptr(d_in), in_pitch, n_in, _dev_ptr(d_out), out_pitch, out_cap, ratio)
            return r.input_used, r.output_generated

        def process_and_flush_planar_device(self, d_in, in_pitch, n_in, d_out, out_pitch, out_cap, ratio):
            """resampleProcessAndFlushPlanarDevice: a whole clip in planes (pitches in samples, 0: that side interleaved); the flush writes
            behind the process call's frames in every plane"""
            r = self.L.resampleProcessAndFlushPlanarDevice(self.p, _dev_ptr(d_in), in_pitch, n_in, _dev_ptr(d_out), out_pitch, out_cap, ratio)
            return r.input_used, r.output_generated


    class Decimator:
        def __init__(self, channels, bits, nbytes, gain, rate, flags):
            self.L = lib()
            self.p = self.L.decimateInit(channels, bits, nbytes, gain, rate, flags)
            if not self.p:
                raise RuntimeError("decimateInit failed (bad parameters, or no MI355X visible — there is no CPU path)")
            self.channels, self.nbytes = channels, nbytes

        def close(self):
            if getattr(self, "p", None):
                self.L.decimateFree(self.p)
                self.p = None

        __del__ = close

        def process(self, x):
            """x float32 [frames, channels] -> (uint8 [frames*channels*nbytes], clipped)"""
            x = _np_f32(x)
            out = np.zeros(x.size * self.nbytes, np.uint8)
            clips = self.L.decimateProcessInterleavedLE(self.p, x.ctypes.data_as(f32p), x.shape[0], out.ctypes.data_as(u8p))
            return out, clips

        def process_planar(self, planes):
            Cn = self.channels
            planes = [_np_f32(p) for p in planes]
            n = len(planes[0])
            outs = [np.zeros(n * self.nbytes, np.uint8) for _ in range(Cn)]
            ip = (f32p * Cn)(*[p.ctypes.data_as(f32p) for p in planes])
            op = (u8p * Cn)(*[o.ctypes.data_as(u8p) for o in outs])
            clips = self.L.decimateProcessLE(self.p, ip, n, op)
            return outs, clips

        def process_device(self, d_in, frames, d_out):
            self.L.decimateProcessInterleavedLEDevice(self.p, _dev_ptr(d_in), frames, _dev_ptr(d_out))

        def process_planar_device(self, d_in, in_pitch, frames, d_out, out_pitch):
            """decimateProcessPlanarLEDevice: channel c of the input at d_in + c * in_pitch (samples), of the output at d_out + c * out_pitch
            (bytes); a pitch of 0: that side is interleaved.  The bytes of process_device on the transposed input, transposed back"""
            self.L.decimateProcessPlanarLEDevice(self.p, _dev_ptr(d_in), in_pitch, frames, _dev_ptr(d_out), out_pitch)

        def reset(self):
            """decimateHipReset: back to what the constructor left (the clip counter keeps its total), on the context's stream"""
            self.L.decimateHipReset(self.p)

        def clipped(self):
            return self.L.decimateHipClipped(self.p)

        def shards(self):
            return self.L.decimateHipShardCount(self.p)

        def set_stream(self, s):
            self.L.decimateHipSetStream(self.p, s)


    class BiquadBank:
        def __init__(self, sections, channels, nsections, multi=False):
            """sections: ctypes array (Biquad * (channels*nsections)), channel-major; multi: spread over the listed devices"""
            self.L = lib()
            self.p = (self.L.biquadBankCreateMulti if multi else self.L.biquadBankCreate)(sections, channels, nsections)
            if not self.p:
                raise RuntimeError("biquadBankCreate failed (no MI355X visible — there is no CPU path)")
            self.n = channels * nsections

        def close(self):
            if getattr(self, "p", None):
                self.L.biquadBankFree(self.p)
                self.p = None

        __del__ = close

        def apply_device(self, d_buf, frames):
            self.L.biquadBankApplyInterleavedDevice(self.p, _dev_ptr(d_buf), frames)

        def apply_planar_device(self, d_buf, pitch, frames):
            """in place over planes: channel c at d_buf + c * pitch samples (0: interleaved, the call above)"""
            self.L.biquadBankApplyPlanarDevice(self.p, _dev_ptr(d_buf), int(pitch), frames)

        def reset(self):
            """every section back to what the bank was created from, in stream order (biquadBankReset)"""
            self.L.biquadBankReset(self.p)

        def set_stream(self, s):
            self.L.biquadBankSetStream(self.p, s)

        def repairs(self):
            return self.L.biquadBankRepairs(self.p)

        def shards(self):
            return self.L.biquadBankShardCount(self.p)

        def read(self):
            out = (Biquad * self.n)()
            self.L.biquadBankRead(self.p, out)
            return out

    def process_batch_device(resamplers, d_ins, n_ins, d_outs, out_caps, ratios):
        """resampleProcessBatchInterleavedDevice over a list of Resampler objects: one call per context, one launch for those
        the general kernel runs and one grouped launch per shape for those the f32 streaming matrix kernel runs un-split on kept rows
        (matrix-size calls under preference 6, anchored calls under the cut-invariant policy; a stream's first matrix call, which
        builds its rows, and everything else is made one by one).  Returns [(input_used, output_generated), ...] (raises if a launch failed)."""
        return _batch("resampleProcessBatchInterleavedDevice", False, resamplers, d_ins, None, n_ins, d_outs, None, out_caps, ratios)

    def process_and_flush_batch_device(resamplers, d_ins, n_ins, d_outs, out_caps, ratios):
        """resampleProcessAndFlushBatchInterleavedDevice over a list of Resampler objects: every context's
        resampleProcessAndFlushInterleavedDevice call, the process calls (general-kernel and matrix-core calls alike, as
        process_batch_device gathers them) and then the flushes gathered into shared launches (a
        d_ins entry may be None with n_ins 0: a pure flush).  Returns [(input_used, output_generated), ...] (raises if a launch failed)."""
        return _batch("resampleProcessAndFlushBatchInterleavedDevice", False, resamplers, d_ins, None, n_ins, d_outs, None, out_caps, ratios)

    def _batch(name, planar, resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios, *more):
        """the body of the five wrappers around it: a planar entry takes a pitch array behind each side's addresses, and `more` in front
        of the results"""
        n = len(resamplers)
        res = (ResampleResult * n)()
        side = lambda d, pitches: (_dev_ptrs(d, n), _longs(pitches, n)) if planar else (_dev_ptrs(d, n),)
        rc = getattr(lib(), name)(_contexts(resamplers, n), n, *side(d_ins, in_pitches), _ints(n_ins, n), *side(d_outs, out_pitches),
                                  _ints(out_caps, n), _doubles(ratios, n), *more, res)
        if rc:
            raise RuntimeError(name + " failed")
        return _results(res, n)

    def process_batch_planar_device(resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios):
        """resampleProcessBatchPlanarDevice: process_batch_device with a pitch per buffer, in samples (channel c of item i at
        d_ins[i] + c * in_pitches[i]; 0: that side of that item interleaved; None for a pitch list: every item's is).  Calls the single
        planar call would stage are transposed by one launch in front of the FIR launches and one behind.
        Returns [(input_used, output_generated), ...] (raises if a launch failed)."""
        return _batch("resampleProcessBatchPlanarDevice", True, resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios)

    def process_and_flush_batch_planar_device(resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios):
        """resampleProcessAndFlushBatchPlanarDevice: process_and_flush_batch_device on channels-first buffers (pitches as in
        process_batch_planar_device; a d_ins entry may be None with n_ins 0: a pure flush).  The flushes write behind the process
        calls' frames in every plane.  Returns [(input_used, output_generated), ...] (raises if a launch failed)."""
        return _batch("resampleProcessAndFlushBatchPlanarDevice", True, resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios)

    def process_and_flush_clips_planar_device(resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios, from_start=False):
        """resampleProcessAndFlushClipsPlanarDevice: process_and_flush_batch_planar_device, with from_start every context first as after
        its reset() — the contexts on the first one's stream put back by one zeroing launch for all of them, no memset per context."""
        return _batch("resampleProcessAndFlushClipsPlanarDevice", True, resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios,
                             1 if from_start else 0)

    def adjoint_clips_planar_device(resamplers, d_gouts, gout_pitches, n_outs, d_gins, gin_pitches, n_ins, ratios):
        """resampleAdjointClipsPlanarDevice: the gradient of whole clips.  Item i: frames 0 .. n_ins[i]-1 of every channel of d_gins[i] are
        set to the transpose of the clips entry's map (a fresh context of resamplers[i]'s parameters, process then flush) applied to the
        first n_outs[i] frames of d_gouts[i]; pitches as in process_batch_planar_device.  The contexts are only read, and one may be
        listed any number of times.  Returns the launch count (raises if the call returned -1)."""
        n = len(resamplers)
        rc = lib().resampleAdjointClipsPlanarDevice(
            _contexts(resamplers, n), n, _dev_ptrs(d_gouts, n), _longs(gout_pitches, n), _ints(n_outs, n),
            _dev_ptrs(d_gins, n), _longs(gin_pitches, n), _ints(n_ins, n), _doubles(ratios, n))
        if rc < 0:
            raise RuntimeError("resampleAdjointClipsPlanarDevice failed")
        return rc

    def _rows_readable(t):
        """rows that are only read (a grad_y of the resampler adjoints): frames consecutive, planes apart; clips may overlap, but a batch
        stride of 0 is not taken"""
        B, Cn, T = t.shape
        return not ((T and t.stride(2) != 1) or (Cn > 1 and t.stride(1) < T) or (B > 1 and t.stride(0) < 1))

    def _rows_apart(t):
        """rows that may be written, and every operand of the biquad and stretch entries: frames consecutive, planes and clips apart"""
        B, Cn, T = t.shape
        return not ((T and t.stride(2) != 1) or (Cn > 1 and t.stride(1) < T) or (B > 1 and t.stride(0) < max(Cn * T, 1)))

    def _plane_ptrs(t):
        """addresses of the planes of t [..., T] (frames consecutive) as a numpy array of t's leading shape"""
        at = np.zeros(tuple(t.shape[:-1]), np.int64)
        for d in range(t.dim() - 1):
            at = at + (np.arange(t.shape[d], dtype=np.int64) * t.stride(d)).reshape([-1 if k == d else 1 for k in range(t.dim() - 1)])
        return t.data_ptr() + at * t.element_size()

    def _clip_ptrs(t):
        """addresses of the clips of t [B, C, T], a list, and the pitch the planar entries take for them (0: one channel, the same call in
        either layout)"""
        base, step = t.data_ptr(), t.stride(0) * t.element_size()
        return (list(range(base, base + t.shape[0] * step, step)) if step else [base] * t.shape[0]), (t.stride(1) if t.shape[1] > 1 else 0)

    # -- the front of a clip class's call: _clip_input, _pool_ready, then per chunk of _chunks the rows of _clip_ptrs --
    def _clip_input(x, channels, lengths, cuda=True, strided="copy"):
        """(x as [B, C, T], B, C, T, lengths as a checked list) of a call on x [B, C, T] or [C, T].  cuda=False: the caller asks for the
        GPU itself, later.  A stride along T other than 1 — "copy": through .contiguous() (any row pitch is taken as it is); "refuse":
        for a call in place; "keep": the caller looks at the rows itself"""
        import torch
        if x.dim() == 2:
            x = x.unsqueeze(0)
        if x.dim() != 3 or x.shape[1] != channels or (cuda and not x.is_cuda) or x.dtype != getattr(torch, smp_torch):
            raise ValueError(f"expected a CUDA {smp_torch} tensor [B, {channels}, T]")
        if strided != "keep" and x.shape[2] and x.stride(2) != 1:
            if strided == "refuse":
                raise ValueError("in place: the frames of a channel must be consecutive (stride 1 along T)")
            x = x.contiguous()
        B, Cn, T = x.shape
        if lengths is None:
            return x, B, Cn, T, [T] * B
        lengths = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
        if len(lengths) != B or any(v < 0 or v > T for v in lengths):
            raise ValueError("lengths: one entry per clip, 0 .. T")
        return x, B, Cn, T, lengths

    def _pool_ready(pool, need, make, stream):
        """`pool` grown to `need` contexts with make(), and those put on `stream`"""
        while len(pool) < need:
            pool.append(make())
        for p in pool[:need]:
            p.set_stream(stream)

    def _chunks(count, size):
        """`count` items as slices of at most `size`, in order"""
        for b0 in range(0, count, size):
            yield slice(b0, min(count, b0 + size))

    def _out_of_place(src, lengths):
        """a new contiguous tensor for the clips of src [B, C, T] filtered up to lengths[i]: frames at and past lengths[i] go through as
        they are, so src's values where a clip has such frames, else nothing yet"""
        import torch
        return src.clone(memory_format=torch.contiguous_format) if any(v < src.shape[2] for v in lengths) else \
            torch.empty(src.shape, dtype=src.dtype, device=src.device)

    def _grad_function(name, forward, backward):
        """() -> the once-differentiable torch.autograd.Function `name` of forward(ctx, ...) and backward(ctx, grad_y), made on first use
        (torch is imported late) and kept; every forward below notes what backward needs and returns y.view_as(y), which attaches y to the
        graph"""
        def made():
            if name not in _state:
                import torch
                _state[name] = type(name, (torch.autograd.Function,), {
                    "forward": staticmethod(forward), "backward": staticmethod(torch.autograd.function.once_differentiable(backward))})
            return _state[name]
        return made

    def _clip_backward(x_shape, gy, rows_ok, lead):
        """what an adjoint entry's backward starts from: (gx [B, C, T] of zeros, the entry's four row arguments — gy's addresses and pitches,
        then gx's); gy's rows as they lie where rows_ok(gy), else through .contiguous(); `lead` (the context the entry takes its stream from)
        is put on the current stream"""
        import torch
        B, Cn, T = x_shape
        if not rows_ok(gy):
            gy = gy.contiguous()
        gx = torch.zeros(B, Cn, T, dtype=gy.dtype, device=gy.device)     # (zero at and past lengths[i])
        lead.set_stream(torch.cuda.current_stream(gy.device).cuda_stream)
        (gy_ptrs, gy_pitch), (gx_ptrs, gx_pitch) = _clip_ptrs(gy), _clip_ptrs(gx)
        return gx, (gy_ptrs, [gy_pitch] * B, gx_ptrs, [gx_pitch] * B)

    def _clip_resample_forward(ctx, x, y, clip, lengths, made):
        ctx.clip, ctx.lengths, ctx.made, ctx.x_shape = clip, lengths, made, x.shape
        return y.view_as(y)

    def _clip_resample_backward(ctx, gy):
        clip = ctx.clip
        if not clip.pool:
            raise RuntimeError("the ClipResampler was closed before backward")
        B = ctx.x_shape[0]
        gx, (gy_ptrs, gy_pitches, gx_ptrs, gx_pitches) = _clip_backward(ctx.x_shape, gy, _rows_readable, clip.pool[0])
        adjoint_clips_planar_device([clip.pool[0]] * B, gy_ptrs, gy_pitches, ctx.made, gx_ptrs, gx_pitches, ctx.lengths, [clip.ratio] * B)
        return gx, None, None, None, None

    _clip_resample_grad = _grad_function("ClipResampleGrad", _clip_resample_forward, _clip_resample_backward)

    def _schedule_batch(resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, caps, ratios, flush_last, clips=None):
        """(clips: None, or the clips entry's from_start)"""
        n = len(resamplers)
        if not (len(d_ins) == len(n_ins) == len(d_outs) == len(caps) == len(ratios) == n):
            raise ValueError("one entry per stream in every list")
        m = max(n, 1)
        counts = [len(v) for v in n_ins]
        if any(len(caps[i]) != counts[i] or len(ratios[i]) != counts[i] for i in range(n)):
            raise ValueError("n_ins[i], caps[i] and ratios[i] must have one entry per block")
        frames, room, rates = _rows(C.c_int, int, n_ins), _rows(C.c_int, int, caps), _rows(C.c_double, float, ratios)
        res = [(ResampleResult * max(k, 1))() for k in counts]
        made = (C.c_int * m)()
        head = [_contexts(resamplers, m), n, _ints(counts, m), _dev_ptrs(d_ins, m)]
        outs = _dev_ptrs(d_outs, m)
        tail = [_table(rates, m), None if flush_last is None else _ints([1 if f else 0 for f in flush_last], m), _table(res, m), made]
        planar = lambda: (*head, _longs(in_pitches, m), _table(frames, m), outs, _longs(out_pitches, m), _table(room, m))
        if clips is not None:
            name = "resampleProcessScheduleClipsPlanarDevice"
            rc = lib().resampleProcessScheduleClipsPlanarDevice(*planar(), *tail[:2], 1 if clips else 0, *tail[2:])
        elif in_pitches is None and out_pitches is None:
            name = "resampleProcessScheduleBatchInterleavedDevice"
            rc = lib().resampleProcessScheduleBatchInterleavedDevice(*head, _table(frames, m), outs, _table(room, m), *tail)
        else:
            name = "resampleProcessScheduleBatchPlanarDevice"
            rc = lib().resampleProcessScheduleBatchPlanarDevice(*planar(), *tail)
        if rc < 0:
            raise RuntimeError(name + " failed")
        return rc, [(made[i], _results(res[i], counts[i])) for i in range(n)]

    def process_schedule_batch_device(resamplers, d_ins, n_ins, d_outs, caps, ratios, flush_last=None):
        """resampleProcessScheduleBatchInterleavedDevice: Resampler.process_schedule_device for every stream of a list in one call —
        n_ins[i], caps[i] and ratios[i] are stream i's blocks, contiguous in d_ins[i], the outputs packed in d_outs[i]; flush_last: a flag
        per stream, or None.  The gatherable blocks of all streams share one launch per kernel variant.
        Returns (launches, [(blocks_made_i, [(input_used, output_generated), ...]), ...]); raises if a launch failed."""
        return _schedule_batch(resamplers, d_ins, None, n_ins, d_outs, None, caps, ratios, flush_last)

    def process_schedule_batch_planar_device(resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, caps, ratios, flush_last=None):
        """resampleProcessScheduleBatchPlanarDevice: process_schedule_batch_device with a pitch per buffer, in samples (channel c of
        stream i at d_ins[i] + c * in_pitches[i]; 0: that side of that stream interleaved; None for a pitch list: every stream's is)."""
        if in_pitches is None and out_pitches is None:
            in_pitches = [0] * len(resamplers)
        return _schedule_batch(resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, caps, ratios, flush_last)

    def process_schedule_clips_planar_device(resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, caps, ratios, flush_last=None, from_start=False):
        """resampleProcessScheduleClipsPlanarDevice: process_schedule_batch_planar_device, with from_start every context first as after its
        reset() — the contexts on the first one's stream put back by one zeroing launch for all of them (it counts as one launch).
        Returns (launches, [(blocks_made_i, [(input_used, output_generated), ...]), ...]); raises if a launch failed."""
        return _schedule_batch(resamplers, d_ins, in_pitches, n_ins, d_outs, out_pitches, caps, ratios, flush_last, clips=bool(from_start))

    def adjoint_schedule_clips_planar_device(resamplers, d_gouts, gout_pitches, n_outs, d_gins, gin_pitches, n_ins, ratios):
        """resampleAdjointScheduleClipsPlanarDevice: the gradient of whole clips made block by block.  n_ins[i] and ratios[i] are clip i's
        blocks (frames and ratio of each); frames 0 .. sum(n_ins[i])-1 of every channel of d_gins[i] are set to the transpose of the
        schedule clips entry's map (a fresh context of resamplers[i]'s parameters, the blocks in turn, then the flush) applied to the first
        n_outs[i] frames of d_gouts[i]; pitches as in process_batch_planar_device.  The contexts are only read, and one may be listed any
        number of times.  Returns the launch count (raises if the call returned -1)."""
        n = len(resamplers)
        if not (len(d_gouts) == len(n_outs) == len(d_gins) == len(n_ins) == len(ratios) == n):
            raise ValueError("one entry per clip in every list")
        if any(len(n_ins[i]) != len(ratios[i]) for i in range(n)):
            raise ValueError("n_ins[i] and ratios[i] must have one entry per block")
        m = max(n, 1)
        counts = [len(v) for v in n_ins]
        frames, rates = _rows(C.c_int, int, n_ins), _rows(C.c_double, float, ratios)
        rc = lib().resampleAdjointScheduleClipsPlanarDevice(
            _contexts(resamplers, m), n, _ints(counts, m), _dev_ptrs(d_gouts, m), _longs(gout_pitches, m), _ints(n_outs, m),
            _dev_ptrs(d_gins, m), _longs(gin_pitches, m), _table(frames, m), _table(rates, m))
        if rc < 0:
            raise RuntimeError("resampleAdjointScheduleClipsPlanarDevice failed")
        return rc

    def _clip_warp_forward(ctx, x, y, clip, blocks, rates, made):
        ctx.clip, ctx.blocks, ctx.rates, ctx.made, ctx.x_shape = clip, blocks, rates, made, x.shape
        return y.view_as(y)

    def _clip_warp_backward(ctx, gy):
        import torch
        clip, B = ctx.clip, ctx.x_shape[0]
        if not B:                                                 # (no clip: no context was ever needed)
            return torch.zeros(ctx.x_shape, dtype=gy.dtype, device=gy.device), None, None, None, None, None
        if not clip.pool:
            raise RuntimeError("the ClipWarper was closed before backward")
        gx, (gy_ptrs, gy_pitches, gx_ptrs, gx_pitches) = _clip_backward(ctx.x_shape, gy, _rows_readable, clip.pool[0])
        adjoint_schedule_clips_planar_device([clip.pool[0]] * B, gy_ptrs, gy_pitches, ctx.made, gx_ptrs, gx_pitches, ctx.blocks, ctx.rates)
        return gx, None, None, None, None, None

    _clip_warp_grad = _grad_function("ClipWarpGrad", _clip_warp_forward, _clip_warp_backward)

    class ClipWarper:
        """Whole clips, channels-first, at a rate that changes inside the clip: x [B, C, T] (or [C, T]) on the GPU and a ratio per block of
        `block` frames in, (y [B, C, Tout_max], out_lengths) out — one resampleProcessScheduleClipsPlanarDevice call per pool on the
        tensor's own rows.  Clip i's block k is frames [k * block, min((k + 1) * block, lengths[i])) at ratios[i][k] (output rate over input
        rate, as resampleProcess takes it); clip i is what a fresh context makes of those blocks in turn and then of the flush (an empty
        clip: the flush's outputs alone); y[i, :, out_lengths[i]:] is zero.  `ratios` holds host values: a scalar, [B] or [B, K] with
        K >= ceil(max(lengths) / block) (a list, a numpy array or a CPU tensor; a CUDA tensor is downloaded once).
        Differentiable once with respect to the samples: where x requires grad (and grad mode is on) y is attached to the graph, and
        backward is ONE resampleAdjointScheduleClipsPlanarDevice call on the rows of grad_y, zero at and past lengths[i].  The ratio curve
        gets no gradient: a `ratios` tensor that requires grad is refused.  Without gradients the call is the forward alone."""

        def __init__(self, channels, taps=380, filters=380, flags=BLACKMAN_HARRIS | SUBSAMPLE_INTERPOLATE | INCLUDE_LOWPASS, lowpass_ratio=0.0,
                     block=1024, max_batch=1024):
            if flags & EXTRAPOLATE_ENDPOINTS:
                raise ValueError("ClipWarper: EXTRAPOLATE_ENDPOINTS is not linear in the samples (no adjoint)")
            if int(block) < 1:
                raise ValueError("ClipWarper: block must be at least one frame")
            self.channels, self.taps, self.block, self.max_batch = channels, taps, int(block), max(1, int(max_batch))
            self._init = (channels, taps, filters, float(lowpass_ratio), flags)
            self.pool = []

        def close(self):
            for r in self.pool:
                r.close()
            self.pool = []

        def blocks(self, lengths, ratios):
            """([frames of every block of clip i], [their ratios]) — the host part of a call, with its checks"""
            B = len(lengths)
            if getattr(ratios, "requires_grad", False):
                raise ValueError("ClipWarper: ratios that require grad: the ratio curve has no gradient (it would silently be zero)")
            if hasattr(ratios, "detach"):
                ratios = ratios.detach().cpu().numpy()
            r = np.asarray(ratios, dtype=np.float64)
            need = [max(1, -(-n // self.block)) for n in lengths]
            if r.ndim == 0:
                r = np.broadcast_to(r, (B, max(need, default=1)))
            elif r.ndim == 1 and r.shape[0] == B:
                r = np.broadcast_to(r[:, None], (B, max(need, default=1)))
            elif r.ndim != 2 or r.shape[0] != B or r.shape[1] < max(need, default=1):
                raise ValueError("ratios: a scalar, [B] or [B, K] with K >= ceil(max(lengths) / block)")
            frames = [[min(self.block, n - k * self.block) for k in range(need[i])] if n else [0] for i, n in enumerate(lengths)]
            rates = [[float(v) for v in r[i, :need[i]]] for i in range(B)]
            if any(not (v > 0.0 and v < float("inf")) for row in rates for v in row):
                raise ValueError("ratios must be finite and > 0")
            return frames, rates

        def __call__(self, x, ratios, lengths=None):
            import torch
            # (the GPU is asked for behind the host checks, those of `ratios` included: they need none)
            x, B, Cn, T, lengths = _clip_input(x, self.channels, lengths, cuda=False, strided="keep")
            frames, rates = self.blocks(lengths, ratios)
            if not x.is_cuda:
                raise ValueError(f"expected a CUDA {smp_torch} tensor [B, {self.channels}, T]")
            if x.shape[2] and x.stride(2) != 1:
                x = x.contiguous()                                # (frames of a channel must be consecutive; any row pitch is taken as it is)
            stream = torch.cuda.current_stream(x.device).cuda_stream
            _pool_ready(self.pool, min(B, self.max_batch), lambda: Resampler(*self._init), stream)
            # room so that no block is cut: a block of n frames moves the position by at most n frames past where the block before left it
            # (not behind the input), the flush by half a window more
            caps = [[int((n + 2) * q) + 4 for n, q in zip(f, r)] for f, r in zip(frames, rates)]
            for c, f, r in zip(caps, frames, rates):
                c[-1] = int((f[-1] + self.taps // 2 + 2) * r[-1]) + 4
            y = torch.zeros(B, Cn, max((sum(c) for c in caps), default=0), dtype=x.dtype, device=x.device)
            (xs, in_pitch), (ys, out_pitch) = _clip_ptrs(x), _clip_ptrs(y)
            made = []
            for rows in _chunks(B, self.max_batch):
                k = rows.stop - rows.start
                _, got = process_schedule_clips_planar_device(
                    self.pool[:k], xs[rows], [in_pitch] * k, frames[rows], ys[rows], [out_pitch] * k, caps[rows], rates[rows],
                    flush_last=[True] * k, from_start=True)
                for i, (blocks_made, res) in enumerate(got, rows.start):
                    if blocks_made != len(frames[i]) or any(used != n for (used, _), n in zip(res, frames[i])):
                        raise RuntimeError(f"ClipWarper: clip {i} was cut short ({blocks_made} of {len(frames[i])} blocks made)")
                    made.append(sum(g for _, g in res))
            out_lengths = torch.tensor(made, dtype=torch.int64)
            y = y[:, :, :max(made, default=0)]
            if x.requires_grad and torch.is_grad_enabled():      # (the samples above are the detached call's; backward is the adjoint kernel)
                y = _clip_warp_grad().apply(x, y, self, frames, rates, made)
            return y, out_lengths

    class ClipResampler:
        """Whole clips, channels-first, from one fixed rate to another: x [B, C, T] (or [C, T]) on the GPU in, (y [B, C, Tout_max],
        out_lengths) out — one resampleProcessAndFlushClipsPlanarDevice call on the tensor's own rows, no copy of the samples on the way.
        Clip i is what a fresh fixed-ratio context makes of x[i, :, :lengths[i]] with resampleProcessAndFlushPlanarDevice (its lead-in
        of half a filter length included); y[i, :, out_lengths[i]:] is zero.  Holds a pool of up to max_batch contexts, started afresh by
        every call (one zeroing launch for all of them); a larger batch is made max_batch clips at a time.
        Differentiable once: where x requires grad (and grad mode is on) y is attached to the graph, and backward is ONE
        resampleAdjointClipsPlanarDevice call on the rows of grad_y (the exact transpose, tap by tap: the stage is linear) that gives a
        gradient shaped like x, zero at and past lengths[i]; out_lengths carries no gradient.  Without gradients the call is unchanged."""

        def __init__(self, channels, src_rate, dst_rate, taps=380, filters=380, flags=BLACKMAN_HARRIS | SUBSAMPLE_INTERPOLATE | INCLUDE_LOWPASS,
                     max_batch=1024):
            self.channels, self.taps, self.max_batch = channels, taps, max(1, int(max_batch))
            self._init = (channels, taps, filters, 0.0, flags, (float(src_rate), float(dst_rate), 0))
            self.ratio = float(dst_rate) / float(src_rate)
            self.pool = []
            self._expected = {}                                  # clip length -> the process call's output frames (a dry run on a reset context)

        def close(self):
            for r in self.pool:
                r.close()
            self.pool = []

        def _room(self, frames):
            """output frames a clip of `frames` frames can make: the process call's (resampleGetExpectedOutput, the context just reset)
            plus the flush's share — half a window of appended silence at the stream's ratio, rounded up, with a few frames to spare (the dry run steps the position by addition, the call by division)"""
            if frames not in self._expected:
                self._expected[frames] = lib().resampleGetExpectedOutput(self.pool[0].p, frames, self.ratio)
            return self._expected[frames] + int(self.taps / 2 * self.ratio) + 4

        def __call__(self, x, lengths=None):
            import torch
            x, B, Cn, T, lengths = _clip_input(x, self.channels, lengths)
            stream = torch.cuda.current_stream(x.device).cuda_stream
            _pool_ready(self.pool, min(B, self.max_batch), lambda: Resampler(*self._init[:5], fixed=self._init[5]), stream)
            if any(v not in self._expected for v in lengths):
                self.pool[0].reset()                              # (the dry run of a new length wants one context at its start)
            rooms = [self._room(v) for v in lengths]
            y = torch.zeros(B, Cn, max(rooms, default=0), dtype=x.dtype, device=x.device)
            (xs, in_pitch), (ys, out_pitch) = _clip_ptrs(x), _clip_ptrs(y)
            made = []
            for rows in _chunks(B, self.max_batch):
                k = rows.stop - rows.start
                got = process_and_flush_clips_planar_device(
                    self.pool[:k], xs[rows], [in_pitch] * k, lengths[rows], ys[rows], [out_pitch] * k, rooms[rows], [self.ratio] * k, from_start=True)
                made += [g for _, g in got]
            out_lengths = torch.tensor(made, dtype=torch.int64)
            y = y[:, :, :max(made, default=0)]
            if x.requires_grad and torch.is_grad_enabled():      # (the samples above are the detached call's; backward is the adjoint kernel)
                y = _clip_resample_grad().apply(x, y, self, lengths, made)
            return y, out_lengths

    def decimate_batch_device(decimators, d_ins, n_ins, d_outs):
        """decimateProcessBatchInterleavedLEDevice over a list of Decimator objects: one launch per class of work for the
        contexts on the first one's stream.  Returns the launch count (raises if the call returned -1)."""
        n = len(decimators)
        rc = lib().decimateProcessBatchInterleavedLEDevice(_contexts(decimators, n), n, _dev_ptrs(d_ins, n), _ints(n_ins, n), _dev_ptrs(d_outs, n))
        if rc < 0:
            raise RuntimeError("decimateProcessBatchInterleavedLEDevice failed")
        return rc

    def decimate_batch_planar_device(decimators, d_ins, in_pitches, n_ins, d_outs, out_pitches):
        """decimateProcessBatchPlanarLEDevice: decimate_batch_device with a pitch per buffer (channel c of item i's input at
        d_ins[i] + c * in_pitches[i] samples, of its output at d_outs[i] + c * out_pitches[i] bytes; 0: that side of that item is
        interleaved; None for a pitch list: every item's is).  Returns the launch count (raises if the call returned -1)."""
        n = len(decimators)
        rc = lib().decimateProcessBatchPlanarLEDevice(
            _contexts(decimators, n), n, _dev_ptrs(d_ins, n), _longs(in_pitches, n), _ints(n_ins, n), _dev_ptrs(d_outs, n), _longs(out_pitches, n))
        if rc < 0:
            raise RuntimeError("decimateProcessBatchPlanarLEDevice failed")
        return rc

    def decimate_clips_planar_device(decimators, d_ins, in_pitches, n_ins, d_outs, out_pitches, from_start=False, d_clip_counts=None):
        """decimateProcessClipsPlanarLEDevice: decimate_batch_planar_device, with from_start every context first as after its reset()
        — the shared launches read each context's first state from the image its constructor left, no copy per context — and with
        d_clip_counts (len(decimators) uint64 / int64 entries of device memory) entry i SET to item i's count of clipped samples by
        the launches themselves, to be read with one download behind the call.  Returns the launch count (raises on -1)."""
        n = len(decimators)
        rc = lib().decimateProcessClipsPlanarLEDevice(
            _contexts(decimators, n), n, _dev_ptrs(d_ins, n), _longs(in_pitches, n), _ints(n_ins, n), _dev_ptrs(d_outs, n), _longs(out_pitches, n),
            1 if from_start else 0, _dev_ptr(d_clip_counts))
        if rc < 0:
            raise RuntimeError("decimateProcessClipsPlanarLEDevice failed")
        return rc

    class ClipDecimator:
        """Whole clips, channels-first, to integer PCM: x [B, C, T] (or [C, T]) on the GPU in, (pcm uint8 [B, C, T * nbytes], clipped)
        out — one decimateProcessClipsPlanarLEDevice call on the tensor's own rows, no copy of the samples on the way.  Clip i is what
        a fresh Decimator makes of x[i, :, :lengths[i]]; pcm[i, :, lengths[i] * nbytes:] is zero; clipped[i] is clip i's count of
        clipped samples (counted by the launches into one device tensor, read with one download: that waits for the call).  Holds a
        pool of up to max_batch contexts, started afresh by every call without an operation per context, on the caller's current
        torch stream; a larger batch is made max_batch clips at a time (`launches`: how many the last call enqueued).  Takes
        ClipResampler's (y, out_lengths) as they come."""

        def __init__(self, channels, bits, nbytes, gain, rate, flags, max_batch=1024):
            self.channels, self.bits, self.nbytes, self.max_batch = channels, bits, nbytes, max(1, int(max_batch))
            self._init = (channels, bits, nbytes, gain, rate, flags)
            self.pool = []
            self.launches = 0

        def close(self):
            for d in self.pool:
                d.close()
            self.pool = []

        def as_int(self, pcm):
            """pcm of 2 or 4 bytes per sample as int16 / int32 [B, C, T] (a view: little-endian samples on a little-endian host)"""
            import torch
            if self.nbytes not in (2, 4):
                raise ValueError("as_int: 2 or 4 bytes per sample")
            return pcm.view(torch.int16 if self.nbytes == 2 else torch.int32)

        def __call__(self, x, lengths=None):
            import torch
            x, B, Cn, T, lengths = _clip_input(x, self.channels, lengths)
            stream = torch.cuda.current_stream(x.device).cuda_stream
            _pool_ready(self.pool, min(B, self.max_batch), lambda: Decimator(*self._init), stream)
            pcm = torch.zeros(B, Cn, T * self.nbytes, dtype=torch.uint8, device=x.device)
            (xs, in_pitch), (ps, out_pitch) = _clip_ptrs(x), _clip_ptrs(pcm)
            counts = torch.empty(B, dtype=torch.int64, device=x.device)     # (every entry is set by the call that takes its clip)
            self.launches = 0
            for rows in _chunks(B, self.max_batch):
                k = rows.stop - rows.start
                self.launches += decimate_clips_planar_device(
                    self.pool[:k], xs[rows], [in_pitch] * k, lengths[rows], ps[rows], [out_pitch] * k, from_start=True,
                    d_clip_counts=counts.data_ptr() + 8 * rows.start)
            return pcm, counts.cpu()

    def biquad_batch_device(banks, d_bufs, frames):
        """biquadBankApplyBatchInterleavedDevice over a list of BiquadBank objects: one launch per section count for the banks on
        the first one's stream.  Returns the launch count (raises if the call returned -1)."""
        n = len(banks)
        rc = lib().biquadBankApplyBatchInterleavedDevice(_contexts(banks, n), n, _dev_ptrs(d_bufs, n), _ints(frames, n))
        if rc < 0:
            raise RuntimeError("biquadBankApplyBatchInterleavedDevice failed")
        return rc

    def biquad_batch_planar_device(banks, d_bufs, pitches, frames):
        """biquadBankApplyBatchPlanarDevice: biquad_batch_device with a pitch per buffer (channel c of item i at d_bufs[i] + c * pitches[i]
        samples; 0: that item is interleaved; None for the list: every item is).  Returns the launch count (raises if the call
        returned -1)."""
        n = len(banks)
        rc = lib().biquadBankApplyBatchPlanarDevice(_contexts(banks, n), n, _dev_ptrs(d_bufs, n), _longs(pitches, n), _ints(frames, n))
        if rc < 0:
            raise RuntimeError("biquadBankApplyBatchPlanarDevice failed")
        return rc

    def biquad_clips_planar_device(banks, d_bufs, pitches, frames, from_start=False):
        """biquadBankApplyClipsPlanarDevice: biquad_batch_planar_device whose long time-parallel calls share launches as well (one copy
        launch and three launches per section count and layout, whatever the number of banks).  from_start: every bank as after its
        reset(), without a copy per bank.  Returns the launch count (raises if the call returned -1)."""
        n = len(banks)
        rc = lib().biquadBankApplyClipsPlanarDevice(_contexts(banks, n), n, _dev_ptrs(d_bufs, n), _longs(pitches, n), _ints(frames, n),
                                                    1 if from_start else 0)
        if rc < 0:
            raise RuntimeError("biquadBankApplyClipsPlanarDevice failed")
        return rc

    def biquad_filter_clips_planar_device(banks, d_ins, in_pitches, d_outs, out_pitches, frames, reversed=False):
        """biquadBankFilterClipsPlanarDevice: whole clips out of place from the banks' first state — item i: frames 0 .. frames[i]-1 of
        every channel of d_outs[i] are what a fresh bank of banks[i]'s sections makes of d_ins[i] (which is only read); reversed: with
        time running backwards, which is the transpose of the forward map (its gradient).  Pitches as in biquad_clips_planar_device,
        one list per side.  The banks are only read, and one may be listed any number of times.  Returns the launch count (raises if
        the call returned -1)."""
        n = len(banks)
        rc = lib().biquadBankFilterClipsPlanarDevice(
            _contexts(banks, n), n, _dev_ptrs(d_ins, n), _longs(in_pitches, n), _dev_ptrs(d_outs, n), _longs(out_pitches, n), _ints(frames, n),
            1 if reversed else 0)
        if rc < 0:
            raise RuntimeError("biquadBankFilterClipsPlanarDevice failed")
        return rc

    def _clip_filter_rows(bank, src, dst, lengths, reversed):
        """one biquad_filter_clips_planar_device call on the rows of src [B, C, T] into those of dst, `bank` listed B times"""
        B = src.shape[0]
        (src_ptrs, src_pitch), (dst_ptrs, dst_pitch) = _clip_ptrs(src), _clip_ptrs(dst)
        return biquad_filter_clips_planar_device([bank] * B, src_ptrs, [src_pitch] * B, dst_ptrs, [dst_pitch] * B, lengths, reversed=reversed)

    def _sections_designed(sections):
        """[("lowpass" | "highpass", frequency), ...], one to four -> [BiquadCoefficients] as biquad_lowpass / biquad_highpass design them"""
        sections = list(sections)
        if not 1 <= len(sections) <= 4 or any(kind not in ("lowpass", "highpass") for kind, _ in sections):
            raise ValueError('sections: one to four of ("lowpass" | "highpass", frequency)')
        L, designed = lib(), []
        for kind, freq in sections:
            designed.append(BiquadCoefficients())
            (L.biquad_lowpass if kind == "lowpass" else L.biquad_highpass)(C.byref(designed[-1]), float(freq))
        return designed

    def _clip_filter_forward(ctx, x, y, clip, lengths):
        ctx.clip, ctx.lengths = clip, lengths
        return y.view_as(y)

    def _clip_filter_backward(ctx, gy):
        import torch
        clip, lengths = ctx.clip, ctx.lengths
        if not clip.pool:
            raise RuntimeError("the ClipFilter was closed before backward")
        if not _rows_apart(gy):
            gy = gy.contiguous()
        gx = _out_of_place(gy, lengths)                           # (the gradient at and past lengths[i] goes through as the frames did)
        clip.pool[0].set_stream(torch.cuda.current_stream(gy.device).cuda_stream)
        _clip_filter_rows(clip.pool[0], gy, gx, lengths, True)
        return gx, None, None, None

    _clip_filter_grad = _grad_function("ClipFilterGrad", _clip_filter_forward, _clip_filter_backward)

    class ClipFilter:
        """Whole clips, channels-first, through a cascade of one to four second-order sections, IN PLACE: x [B, C, T] (or [C, T]) on the
        GPU in, the same tensor out — one biquadBankApplyClipsPlanarDevice call on the tensor's own rows, the clips' long runs in
        shared launches (`launches`: how many the last call enqueued).  sections: [("lowpass" | "highpass", frequency), ...] (frequency as biquad_lowpass / biquad_highpass take it: a fraction
        of the sample rate; gain 1.0); ART's -p is two low-passes at one frequency.  Clip i is what a fresh bank makes of
        x[i, :, :lengths[i]]; x[i, :, lengths[i]:] is not touched.  Holds a pool of up to max_batch banks, reset for every call, on the
        caller's current torch stream; a larger batch is made max_batch clips at a time.  Takes and gives what ClipResampler and
        ClipDecimator take.

        Differentiable: when x requires grad (and grad mode is on) x is NOT written.  The call returns a new tensor with exactly the
        values the in-place call would have left in x (x[i, :, lengths[i]:] copied through), made by one
        biquadBankFilterClipsPlanarDevice call that lists the pool's first bank once per clip and attached to the graph by a
        once-differentiable autograd.Function.  Its backward is the same entry with time reversed on the rows of grad_y — the exact
        transpose of the forward map, from the same kernels — with the gradient at and past lengths[i] passed through; it raises
        after close().  A non-contiguous x is taken through .contiguous() on this path."""

        def __init__(self, channels, sections, max_batch=1024):
            designed = _sections_designed(sections)
            self.channels, self.nsections, self.max_batch = channels, len(designed), max(1, int(max_batch))
            L = lib()
            self._sections = (Biquad * (channels * self.nsections))()
            for s, co in enumerate(designed):
                for c in range(channels):
                    L.biquad_init(C.byref(self._sections[c * self.nsections + s]), C.byref(co), 1.0)
            self.pool = []
            self.launches = 0

        def close(self):
            for b in self.pool:
                b.close()
            self.pool = []

        def __call__(self, x, lengths=None):
            import torch
            whole = x
            tracked = x.requires_grad and torch.is_grad_enabled()
            # (in place a stride along T is refused: there is no copy to write back; a tracked x is taken through _rows_apart below)
            x, B, Cn, T, lengths = _clip_input(x, self.channels, lengths, strided="keep" if tracked else "refuse")
            make = lambda: BiquadBank(self._sections, Cn, self.nsections)
            stream = torch.cuda.current_stream(x.device).cuda_stream
            if tracked:
                # out of place, for autograd: x and everything the graph saved stay as they are
                _pool_ready(self.pool, 1, make, stream)
                src = x if _rows_apart(x) else x.contiguous()
                with torch.no_grad():
                    y = _out_of_place(src, lengths)
                    self.launches = _clip_filter_rows(self.pool[0], src, y, lengths, False) if B else 0
                y = _clip_filter_grad().apply(src, y, self, lengths)
                return y[0] if whole.dim() == 2 else y
            _pool_ready(self.pool, min(B, self.max_batch), make, stream)
            xs, pitch = _clip_ptrs(x)
            self.launches = 0
            for rows in _chunks(B, self.max_batch):
                k = rows.stop - rows.start
                self.launches += biquad_clips_planar_device(self.pool[:k], xs[rows], [pitch] * k, lengths[rows], from_start=True)
            return whole

    class _BiquadBankSet:
        """the banks one set of ClipBiquad coefficient values needs, made on first use: the whole cascade; for the coefficient
        gradient its prefixes 1..s, its suffixes s+1..S and each section's all-pole part.  co: numpy [C, S, 9], the build's dtype."""

        def __init__(self, co):
            self.co, (self.channels, self.nsections, _) = co, co.shape
            self.banks = {}

        def bank(self, kind, s=0):
            """'full'; ('prefix', s): sections 1..s; ('suffix', s): sections s+1..S; ('pole', s): 1 / (1 + b1 z^-1 + ...) of section s"""
            Cn, S = self.channels, self.nsections
            if (kind == "prefix" and s == S) or (kind == "suffix" and s == 0):
                kind, s = "full", 0
            if (kind, s) not in self.banks:
                which = {"full": range(S), "prefix": range(s), "suffix": range(s, S), "pole": [s - 1]}[kind]
                L = lib()
                secs = (Biquad * (Cn * len(which)))()
                for c in range(Cn):
                    for j, k in enumerate(which):
                        v = [float(q) for q in self.co[c, k]]
                        if kind == "pole":
                            v[:5] = [1.0, 0.0, 0.0, 0.0, 0.0]
                        L.biquad_init(C.byref(secs[c * len(which) + j]), C.byref(BiquadCoefficients(*v)), 1.0)
                self.banks[(kind, s)] = BiquadBank(secs, Cn, len(which))
            return self.banks[(kind, s)]

        def close(self):
            for b in self.banks.values():
                b.close()
            self.banks = {}

    def _clip_biquad_forward(ctx, x, coefficients, y, kept, clip, banks, lengths):
        ctx.clip, ctx.banks, ctx.lengths, ctx.generation, ctx.co = clip, banks, lengths, clip._generation, coefficients
        ctx.save_for_backward(x, y, kept)
        return y.view_as(y)

    def _clip_biquad_backward(ctx, gy):
        import torch
        clip, banks, lengths = ctx.clip, ctx.banks, ctx.lengths
        if clip._generation != ctx.generation:
            raise RuntimeError("the ClipBiquad was closed before backward")
        x, y, kept = ctx.saved_tensors
        need_x, need_co = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not _rows_apart(gy):
            gy = gy.contiguous()
        B, Cn, T = gy.shape
        S = banks.nsections
        stream = torch.cuda.current_stream(gy.device).cuda_stream
        gx = _out_of_place(gy, lengths) if need_x else None      # (the gradient at and past lengths[i] goes through as the frames did)
        gy_ptrs, gy_pitch = _clip_ptrs(gy)
        clip.backward_launches = [0, 0, 0]
        if not need_co:
            banks.bank("full").set_stream(stream)
            clip.backward_launches[0] = _clip_filter_rows(banks.bank("full"), gy, gx, lengths, True) if B else 0
            return gx, None, None, None, None, None, None
        # g_s, s = 0 .. S-1: grad_y through the reversed sections s+1 .. S (g_0 is grad_x; g_S is grad_y itself)
        g = torch.empty((max(S - 1, 0), B, Cn, T), dtype=gy.dtype, device=gy.device)
        outs = ([(0, gx)] if need_x else []) + [(s, g[s - 1]) for s in range(1, S)]
        if outs and B:
            call = [banks.bank("suffix", s) for s, _ in outs for _ in range(B)]
            call[0].set_stream(stream)
            optr = np.concatenate([_clip_ptrs(o)[0] for _, o in outs])
            pitch = [gy_pitch] * len(call)
            clip.backward_launches[0] = biquad_filter_clips_planar_device(
                call, np.tile(gy_ptrs, len(outs)), pitch, optr, [T if Cn > 1 else 0] * len(call), lengths * len(outs), reversed=True)
        # u_s, s = 1 .. S: g_s through the all-pole part of section s, reversed
        u = torch.empty((S, B, Cn, T), dtype=gy.dtype, device=gy.device)
        sums = torch.zeros((B, Cn, S, 9), dtype=torch.float64, device=gy.device)
        if B:
            call = [banks.bank("pole", s) for s in range(1, S + 1) for _ in range(B)]
            call[0].set_stream(stream)
            iptr = np.concatenate([_clip_ptrs(g[s - 1])[0] for s in range(1, S)] + [gy_ptrs])
            ipitch = [T if Cn > 1 else 0] * ((S - 1) * B) + [gy_pitch] * B
            clip.backward_launches[1] = biquad_filter_clips_planar_device(
                call, iptr, ipitch, _plane_ptrs(u)[..., 0].reshape(-1), [T if Cn > 1 else 0] * (S * B), lengths * S, reversed=True)
            # the lagged sums: per clip, channel and section (u_s, y_{s-1}, lags 0..4) and (u_s, y_s, lags 1..4)
            up = _plane_ptrs(u).transpose(1, 2, 0)                                     # [B, C, S]
            ys = [_plane_ptrs(x)] + [_plane_ptrs(kept[s]) for s in range(S - 1)] + [_plane_ptrs(y)]
            before, after = np.stack(ys[:-1], axis=-1), np.stack(ys[1:], axis=-1)      # y_{s-1}, y_s: [B, C, S]
            sp = _plane_ptrs(sums)
            frames = np.broadcast_to(np.asarray(lengths, np.int64).reshape(B, 1, 1), (B, Cn, S))
            rows = lambda a, b: np.concatenate([a.reshape(-1), b.reshape(-1)])
            count = B * Cn * S
            clip.backward_launches[2] = lag_products_batch_device(
                rows(up, up), rows(before, after), rows(frames, frames), [0] * count + [1] * count, [5] * count + [4] * count,
                rows(sp, sp + 5 * 8), stream=stream)
        sums = sums.sum(0)
        if ctx.co.dim() == 2:
            sums = sums.sum(0)
        sums[..., 5:] = -sums[..., 5:]
        return gx, sums.to(dtype=ctx.co.dtype).to(ctx.co.device), None, None, None, None, None

    _clip_biquad_grad = _grad_function("ClipBiquadGrad", _clip_biquad_forward, _clip_biquad_backward)

    class ClipBiquad:
        """Whole clips, channels-first, through a cascade of one to four sections whose COEFFICIENTS can be learnt: x [B, C, T] (or
        [C, T]) on the GPU in, y out — always a NEW tensor, x is never written.  coefficients: a tensor [S, 9] (one cascade for every
        channel) or [channels, S, 9], 1 <= S <= 4, columns a0..a4, b1..b4 of (a0 + a1 z^-1 + ... + a4 z^-4) / (1 + b1 z^-1 + ... +
        b4 z^-4) (biquad.h), of the build's sample type — so the filter runs on the parameter's exact values — on the CPU or the GPU.
        It is held by reference (the caller's nn.Parameter) and read at every call: the banks (biquad_init with gain 1.0) are cached
        on its _version and data_ptr and rebuilt only when those change; a GPU tensor costs one small download per rebuild.
        ClipBiquad.design(sections) gives the [S, 9] values ClipFilter builds for the same sections.

        y[i, :, :lengths[i]] is, bit for bit, what biquad_filter_clips_planar_device makes of a fresh bank of those sections;
        y[i, :, lengths[i]:] is x copied through.  A non-contiguous x is taken through .contiguous(); work runs on the current torch
        stream; `launches`: the kernel launches the last forward call enqueued.

        Differentiable in x and in the coefficients (once).  Nothing tracked, or only x: one filter call with B items; grad_x is the
        same entry with time reversed, as in ClipFilter.  coefficients.requires_grad (grad mode on): the forward is ONE filter call
        whose items are the prefixes 1..s of every clip's cascade (y_1 .. y_{S-1} are kept), and the backward is one reversed call
        for g_s = grad_y through sections s+1..S (g_0 is grad_x), one reversed call through each section's all-pole part for u_s, and
        ONE artamdLagProductsBatchDevice call of 2 B C S rows:
            dL/da_k (section s) =  sum_{t >= k} u_s[t] y_{s-1}[t-k], k = 0..4;   dL/db_k (section s) = -sum_{t >= k} u_s[t] y_s[t-k], k = 1..4
        summed in fp64 over clips (and channels, for [S, 9]), cast to the coefficients' dtype and moved to their device
        (`backward_launches`: the three calls' launch counts).  All nine columns get a gradient, whatever order biquad_init derived.
        Frames at and past lengths[i] add nothing to it; their grad_y passes through to grad_x.  The backward holds the banks of its
        forward call (a rebuild in between does not change it) and raises after close().

        Filters that do not forget within 1,024 frames take the entry's serial route, as everywhere: correct, but slow on long clips."""

        def __init__(self, channels, coefficients):
            self.channels, self.coefficients = int(channels), coefficients
            self._check()
            self._banks, self._key, self._generation = None, None, 0
            self.launches, self.backward_launches = 0, [0, 0, 0]

        def _check(self):
            import torch
            co = self.coefficients
            if not isinstance(co, torch.Tensor) or co.dtype != getattr(torch, smp_torch):
                raise ValueError(f"coefficients: a {smp_torch} tensor")
            if co.dim() not in (2, 3) or co.shape[-1] != 9 or not 1 <= co.shape[-2] <= 4 or (co.dim() == 3 and co.shape[0] != self.channels):
                raise ValueError(f"coefficients: [S, 9] or [{self.channels}, S, 9], one to four sections")

        @staticmethod
        def design(sections):
            """[("lowpass" | "highpass", frequency), ...] -> tensor [S, 9] of the build's dtype (on the CPU; needs no GPU): the values
            ClipFilter builds for the same sections"""
            import torch
            rows = [[getattr(co, n) for n, _ in BiquadCoefficients._fields_] for co in _sections_designed(sections)]
            return torch.tensor(rows, dtype=getattr(torch, smp_torch))

        def close(self):
            if self._banks is not None:
                self._banks.close()
            self._banks, self._key = None, None
            self._generation += 1

        def _bank_set(self):
            co = self.coefficients
            key = (co._version, co.data_ptr())
            if self._banks is None or key != self._key:
                self._check()
                host = co.detach().cpu().numpy().astype(smp_np, copy=True)             # (a GPU tensor: the one small download)
                if host.ndim == 2:
                    host = np.broadcast_to(host, (self.channels,) + host.shape)
                # (the set before is not closed here: a graph made from it may still run its backward; it goes with its last holder)
                self._banks, self._key = _BiquadBankSet(np.ascontiguousarray(host)), key
            return self._banks

        def __call__(self, x, lengths=None):
            import torch
            whole = x
            x, B, Cn, T, lengths = _clip_input(x, self.channels, lengths, strided="keep")     # (the rows: _rows_apart below)
            banks = self._bank_set()
            S = banks.nsections
            grad = torch.is_grad_enabled()
            track_x, track_co = grad and x.requires_grad, grad and self.coefficients.requires_grad
            stream = torch.cuda.current_stream(x.device).cuda_stream
            src = x if _rows_apart(x) else x.contiguous()
            with torch.no_grad():
                y = _out_of_place(src, lengths)
                kept = None
                self.launches = 0
                if not track_co:
                    banks.bank("full").set_stream(stream)
                    if B:
                        self.launches = _clip_filter_rows(banks.bank("full"), src, y, lengths, False)
                else:
                    # one call: the prefixes 1 .. s of every clip's cascade; y_1 .. y_{S-1} are kept for the coefficient gradient
                    kept = torch.empty((S - 1, B, Cn, T), dtype=src.dtype, device=src.device)
                    if B:
                        call = [banks.bank("prefix", s) for s in range(1, S + 1) for _ in range(B)]
                        call[0].set_stream(stream)
                        iptr, ipitch = _clip_ptrs(src)
                        optr = np.concatenate([_clip_ptrs(kept[s])[0] for s in range(S - 1)] + [_clip_ptrs(y)[0]])
                        self.launches = biquad_filter_clips_planar_device(
                            call, np.tile(iptr, S), [ipitch] * (S * B), optr, [T if Cn > 1 else 0] * (S * B), lengths * S, reversed=False)
            if track_x or track_co:
                y = _clip_biquad_grad().apply(src, self.coefficients, y, kept, self, banks, lengths)
            return y[0] if whole.dim() == 2 else y

    class Stretcher:
        """Owner of a Stretch * (stretch.h): periods in frames, one or two channels, flags STRETCH_FAST_FLAG | STRETCH_DUAL_FLAG"""

        def __init__(self, shortest, longest, channels, flags=0):
            self.L = lib()
            self.p = self.L.stretchInit(shortest, longest, channels, flags)
            if not self.p:
                raise RuntimeError("stretchInit failed (bad periods or channels, or no MI355X visible — there is no CPU path)")
            self.channels, self.shortest, self.longest, self.flags = channels, shortest, longest, flags

        def close(self):
            if getattr(self, "p", None):
                self.L.stretchFree(self.p)
                self.p = None

        __del__ = close

        def set_stream(self, s):
            self.L.stretchHipSetStream(self.p, s)

    def stretch_clips_batch_planar_device(ctxs, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios, from_start=True):
        """stretchProcessAndFlushBatchPlanarDevice over a list of Stretcher objects: every clip's process call and all its flushes in one
        launch, one workgroup per clip (channel c of item i's input at d_ins[i] + c * in_pitches[i] samples, of its output at
        d_outs[i] + c * out_pitches[i]; 0: that side of that item is interleaved; None for a pitch list: every item's is; a d_ins entry
        may be None with n_ins 0).  out_caps in frames, at least artamdStretchClipCapacity each.  from_start: every context first put
        where stretchInit left it.  Returns the frames made per clip (raises if the call returned -1)."""
        n = len(ctxs)
        produced = (C.c_int * max(n, 1))()
        rc = lib().stretchProcessAndFlushBatchPlanarDevice(
            _contexts(ctxs, n), n, _dev_ptrs(d_ins, n), _longs(in_pitches, n), _ints(n_ins, n), _dev_ptrs(d_outs, n), _longs(out_pitches, n),
            _ints(out_caps, n), _doubles(ratios, n), 1 if from_start else 0, produced)
        if rc < 0:
            raise RuntimeError("stretchProcessAndFlushBatchPlanarDevice failed")
        return list(produced[:n])

    STRETCH_COPY = -2**31                                 # ARTAMD_STRETCH_COPY: `to` of a segment that copies

    def stretch_clips_logged_batch_planar_device(ctxs, d_ins, in_pitches, n_ins, d_outs, out_pitches, out_caps, ratios, d_logs, log_caps):
        """stretchProcessAndFlushLoggedBatchPlanarDevice: stretch_clips_batch_planar_device from a fresh start that also writes the splice
        logs (art_hip.h: int32 records out, count, from, to, in values).  d_logs: per clip a pair of device addresses (the second None
        for a single stage), log_caps: per clip a pair of capacities in segments, at least artamdStretchLogCapacity each.  Returns
        (frames made per clip, (segments of stage 1, of stage 2) per clip); raises if the call returned -1."""
        n = len(ctxs)
        produced, counts = (C.c_int * max(n, 1))(), (C.c_int * max(2 * n, 1))()
        rc = lib().stretchProcessAndFlushLoggedBatchPlanarDevice(
            _contexts(ctxs, n), n, _dev_ptrs(d_ins, n), _longs(in_pitches, n), _ints(n_ins, n), _dev_ptrs(d_outs, n), _longs(out_pitches, n),
            _ints(out_caps, n), _doubles(ratios, n), produced, _dev_ptrs(_flat(d_logs), 2 * n), _ints(_flat(log_caps), 2 * n), counts)
        if rc < 0:
            raise RuntimeError("stretchProcessAndFlushLoggedBatchPlanarDevice failed")
        return list(produced[:n]), [(counts[2 * i], counts[2 * i + 1]) for i in range(n)]

    def stretch_adjoint_clips_planar_device(ctxs, d_logs, log_counts, d_gouts, gout_pitches, n_outs, d_gins, gin_pitches, n_ins):
        """stretchAdjointClipsPlanarDevice: the gradient of logged clips.  Item i: frames 0 .. n_ins[i]-1 of every channel of d_gins[i] are
        set to the transpose of the map its logs spell out (d_logs, log_counts: pairs per clip, as the logged entry took and gave them)
        applied to the first n_outs[i] frames of d_gouts[i]; pitches as in stretch_clips_batch_planar_device.  The contexts are only read,
        and one may be listed any number of times.  Returns the launch count (raises if the call returned -1)."""
        n = len(ctxs)
        rc = lib().stretchAdjointClipsPlanarDevice(
            _contexts(ctxs, n), n, _dev_ptrs(_flat(d_logs), 2 * n), _ints(_flat(log_counts), 2 * n),
            _dev_ptrs(d_gouts, n), _longs(gout_pitches, n), _ints(n_outs, n), _dev_ptrs(d_gins, n), _longs(gin_pitches, n), _ints(n_ins, n))
        if rc < 0:
            raise RuntimeError("stretchAdjointClipsPlanarDevice failed")
        return rc

    def _clip_stretch_forward(ctx, x, y, clip, record):
        ctx.clip, ctx.record, ctx.x_shape = clip, record, x.shape
        return y.view_as(y)

    def _clip_stretch_backward(ctx, gy):
        import torch
        owners, logs, counts, lengths, made, _ = ctx.record   # (logs: addresses inside the device tensor the record keeps alive)
        if any(o.p is None for o in owners):
            raise RuntimeError("the ClipStretcher was closed before backward")
        if not owners:                                        # (no clip: no context to take a stream from)
            return torch.zeros(ctx.x_shape, dtype=gy.dtype, device=gy.device), None, None, None
        gx, (gy_ptrs, gy_pitches, gx_ptrs, gx_pitches) = _clip_backward(ctx.x_shape, gy, _rows_apart, owners[0])
        stretch_adjoint_clips_planar_device(owners, logs, counts, gy_ptrs, gy_pitches, [min(m, gy.shape[2]) for m in made],
                                            gx_ptrs, gx_pitches, lengths)
        return gx, None, None, None

    _clip_stretch_grad = _grad_function("ClipStretchGrad", _clip_stretch_forward, _clip_stretch_backward)

    class ClipStretcher:
        """Whole clips, channels-first, stretched in time without a change of pitch: x [B, C, T] (or [C, T]) on the GPU and a ratio
        (output length over input length, as stretchProcess takes it; a float, or one value per clip) in, (y [B, C, Tout_max],
        out_lengths) out — one stretchProcessAndFlushBatchPlanarDevice call per pool on the tensor's own rows, no copy of the samples on
        the way.  Clip i is what a fresh context with periods rate // 350 and rate // 50 (ART's choice) makes of x[i, :, :lengths[i]],
        process call and flushes together; y[i, :, out_lengths[i]:] is zero.  flags=None keeps two pools of up to max_batch contexts, a
        single stage for ratios in 0.5 .. 2 and a STRETCH_DUAL_FLAG pair outside, and sends each clip to the one its ratio needs; given
        flags make one pool.  Ratios outside 0.25 .. 4 (0.5 .. 2 for given flags without STRETCH_DUAL_FLAG) and more than two channels
        raise.  Runs on the caller's current torch stream; a larger batch is made max_batch clips at a time.  Its output feeds
        ClipResampler as it comes: a pitch shift by `pitch` at a tempo change `tempo` is ClipStretcher at the ratio pitch / tempo
        followed by ClipResampler from rate * pitch to rate.

        Differentiable: when x requires grad (and grad mode is on) the same clips go through stretchProcessAndFlushLoggedBatchPlanarDevice
        — the same samples and lengths, bit for bit — which also records every splice; the logs stay on the device, held by a
        once-differentiable autograd.Function that attaches y to the graph.  The period search's choices are piecewise constant in
        the samples, so between their boundaries a clip is the sparse linear map its log spells out, and backward is that map's
        transpose (stretchAdjointClipsPlanarDevice, one call for the whole batch, both pools together) on the rows of grad_y: the
        gradient is shaped like x and zero at and past lengths[i]; the ratio and out_lengths carry none.  Backward raises after close().
        segments=True: the call returns a third value, per clip a list of one or two int32 numpy arrays [n, 4] (out, count, from, to in
        VALUES, frame * channels + channel; to == STRETCH_COPY: a copy) — the exact time map from input to output, for labels that must
        follow a stretched clip; with or without grad, at the price of the logged entry and one download."""

        def __init__(self, channels, rate, flags=None, max_batch=1024, segments=False):
            if channels not in (1, 2):
                raise ValueError("mono or stereo only")
            self.channels, self.rate, self.flags, self.max_batch = channels, int(rate), flags, max(1, int(max_batch))
            self.segments = bool(segments)
            self.shortest, self.longest = self.rate // 350, self.rate // 50
            self.pools = {}                                      # flags -> contexts

        def close(self):
            for pool in self.pools.values():
                for s in pool:
                    s.close()
            self.pools = {}

        def _flags_for(self, ratio):
            if not 0.25 <= ratio <= 4.0:                         # (also refuses a ratio that is not a number)
                raise ValueError("ratio: 0.25 .. 4")
            if self.flags is None:
                return 0 if 0.5 <= ratio <= 2.0 else STRETCH_DUAL_FLAG
            if not self.flags & STRETCH_DUAL_FLAG and not 0.5 <= ratio <= 2.0:
                raise ValueError("ratio: 0.5 .. 2 without STRETCH_DUAL_FLAG")
            return self.flags

        def __call__(self, x, ratio, lengths=None):
            import torch
            x, B, Cn, T, lengths = _clip_input(x, self.channels, lengths)
            if Cn > 1 and x.stride(1) < T:
                x = x.contiguous()                                # (a broadcast channel dimension: a pitch of 0 would mean interleaved)
            if hasattr(ratio, "tolist"):
                ratio = ratio.tolist()
            ratios = [float(v) for v in ratio] if isinstance(ratio, (list, tuple)) else [float(ratio)] * B
            if len(ratios) != B:
                raise ValueError("ratio: a float, or one value per clip")
            groups = {}                                          # flags -> the clips of that pool
            for i, r in enumerate(ratios):
                groups.setdefault(self._flags_for(r), []).append(i)
            L = lib()
            rooms = [0] * B
            for flags, idx in groups.items():
                for i in idx:
                    rooms[i] = L.artamdStretchClipCapacity(self.longest, flags, lengths[i], ratios[i])
                    if rooms[i] < 0:
                        raise ValueError("clip too long")
            tracked = x.requires_grad and torch.is_grad_enabled()
            logged = tracked or self.segments
            if logged:
                # one tensor of records for the call; clip i's stages at caps_at[i] and behind
                stages = {i: (2 if flags & STRETCH_DUAL_FLAG else 1) for flags, idx in groups.items() for i in idx}
                caps = [[0, 0] for _ in range(B)]
                for flags, idx in groups.items():
                    for i in idx:
                        for s in range(stages[i]):
                            caps[i][s] = L.artamdStretchLogCapacity(self.shortest, self.longest, flags, lengths[i], ratios[i], s)
                starts, total = [], 0
                for i in range(B):
                    starts.append((total, total + caps[i][0]))
                    total += caps[i][0] + caps[i][1]
                records = torch.empty(max(total, 1), 4, dtype=torch.int32, device=x.device)
                log_ptrs = [(records.data_ptr() + 16 * starts[i][0], records.data_ptr() + 16 * starts[i][1] if stages[i] == 2 else None)
                            for i in range(B)]
                counts = [(0, 0)] * B
            stream = torch.cuda.current_stream(x.device).cuda_stream
            y = torch.zeros(B, Cn, max(rooms, default=0), dtype=x.dtype, device=x.device)
            (xs, in_pitch), (ys, out_pitch) = _clip_ptrs(x), _clip_ptrs(y)
            made = [0] * B
            for flags, idx in groups.items():
                pool = self.pools.setdefault(flags, [])
                _pool_ready(pool, min(len(idx), self.max_batch), lambda: Stretcher(self.shortest, self.longest, Cn, flags), stream)
                for rows in _chunks(len(idx), self.max_batch):
                    part = idx[rows]
                    k = len(part)
                    args = (pool[:k], [xs[i] for i in part], [in_pitch] * k, [lengths[i] for i in part],
                            [ys[i] for i in part], [out_pitch] * k, [rooms[i] for i in part], [ratios[i] for i in part])
                    if logged:
                        got, cnt = stretch_clips_logged_batch_planar_device(*args, [log_ptrs[i] for i in part], [caps[i] for i in part])
                        for i, c in zip(part, cnt):
                            counts[i] = c
                    else:
                        got = stretch_clips_batch_planar_device(*args, from_start=True)
                    for i, g in zip(part, got):
                        made[i] = g
            out_lengths = torch.tensor(made, dtype=torch.int64)
            y = y[:, :, :max(made, default=0)]
            if tracked:
                # the adjoint only reads its contexts: each clip's pool's first one stands for it
                owners = [None] * B
                for flags, idx in groups.items():
                    for i in idx:
                        owners[i] = self.pools[flags][0]
                y = _clip_stretch_grad().apply(x, y, self, (owners, log_ptrs, counts, lengths, made, records))
            if self.segments:
                host = records.cpu().numpy()
                maps = [[host[starts[i][s]:starts[i][s] + counts[i][s]].copy() for s in range(stages[i])] for i in range(B)]
                return y, out_lengths, maps
            return y, out_lengths

    def ingest_batch_device(d_ins, gains, bits, nbytes, strides, d_outs, counts, stream=None):
        """floatIntegersBatchLEDevice: item i as floatIntegersLEDevice (d_ins[i], gains[i], bits[i], nbytes[i], strides[i], d_outs[i],
        counts[i]), all in one launch on `stream` (a torch stream, a raw address or None: the null stream).  Returns the launch
        count (raises if the call returned -1)."""
        n = len(d_ins)
        rc = lib().floatIntegersBatchLEDevice(_dev_ptrs(d_ins, n), _doubles(gains, n), _ints(bits, n), _ints(nbytes, n), _ints(strides, n),
                                              _dev_ptrs(d_outs, n), _ints(counts, n), n, _raw_stream(stream))
        if rc < 0:
            raise RuntimeError("floatIntegersBatchLEDevice failed")
        return rc

    def extrapolate_batch_device(d_known, counts, strides, backward, d_outs, extras, stream=None):
        """artamdExtrapolateBatchDevice: run i fits counts[i] known samples at d_known[i] (stride strides[i], oldest first) and writes
        extras[i] samples to d_outs[i] (same stride): past the newest, or before the oldest (nearest first) where backward[i], all in
        one launch on `stream` (a torch stream, a raw address or None: the null stream).  Raises if the call returned -1."""
        n = len(d_known)
        rc = lib().artamdExtrapolateBatchDevice(_dev_ptrs(d_known, n), _ints(counts, n), _ints(strides, n), _ints([bool(v) for v in backward], n),
                                                _dev_ptrs(d_outs, n), _ints(extras, n), n, _raw_stream(stream))
        if rc < 0:
            raise RuntimeError("artamdExtrapolateBatchDevice failed")
        return rc

    def lag_products_batch_device(d_us, d_vs, frames, first_lags, num_lags, d_sums, stream=None):
        """artamdLagProductsBatchDevice: row i sets d_sums[i][q] (doubles), q = 0 .. num_lags[i] - 1, to the fp64 sum over
        t = k .. frames[i] - 1 of d_us[i][t] * d_vs[i][t - k], k = first_lags[i] + q (k < 8), all rows in two launches on `stream` (a
        torch stream, a raw address or None: the null stream).  Rows are planes with stride 1; the lists may be numpy arrays of
        addresses and counts.  Returns the launch count (raises if the call returned -1)."""
        n = len(d_us)
        ptrs = lambda v: np.ascontiguousarray(v if isinstance(v, np.ndarray) else [_dev_ptr(d) or 0 for d in v], dtype=np.uintp)
        ints = lambda v: np.ascontiguousarray(v, dtype=np.intc)
        keep = [ptrs(d_us), ptrs(d_vs), ints(frames), ints(first_lags), ints(num_lags), ptrs(d_sums)]
        if any(len(a) != n for a in keep):
            raise ValueError("lag_products_batch_device: one entry per row in every list")
        rc = lib().artamdLagProductsBatchDevice(*[a.ctypes.data for a in keep[:5]], keep[5].ctypes.data, n, _raw_stream(stream))
        if rc < 0:
            raise RuntimeError("artamdLagProductsBatchDevice failed")
        return rc

    # (_private: the helpers above for the modules beside this one — rate_grad.py — which add to the binding without copying them)
    return types.SimpleNamespace(**{k: v for k, v in locals().items() if not k.startswith("_") and k != "width"}, width=width,
                                 _private=types.SimpleNamespace(**{k: v for k, v in locals().items() if k.startswith("_") and callable(v)}))


_bound = {}


def binding(width=32):
    if width not in _bound:
        ns = _bind(width)
        # the flag values (resampler.h / decimator.h) are the same for both builds
        vars(ns).update({k: v for k, v in globals().items() if k.isupper() and isinstance(v, int)})
        _bound[width] = ns
    return _bound[width]


def wide():
    """the PATH_WIDTH=64 binding: same names (lib, Resampler, Decimator, BiquadBank, Biquad, ...), double samples"""
    return binding(64)


globals().update({k: v for k, v in vars(binding(32)).items() if k not in ("width", "_private")})      # module level = the 4-byte build
