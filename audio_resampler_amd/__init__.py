"""audio_resampler_amd — MI355X-native windowed-sinc resampler, biquad and decimator.

The product is the C-ABI shared library `libartamd.so` (and `libartamd64.so`, the same tree compiled for
8-byte samples, reached through `wide()`): C host layer + hand-written gfx950 HIP
kernels, see csrc/ and ../include/).  This Python package is only plumbing: a ctypes binding that
mirrors the reference's C API name for name (`api.py`), helpers to hand torch device tensors to
the device-pointer entry points, and the build script.
"""
from .api import (  # noqa: F401
    lib, load_library, Resampler, Decimator, BiquadBank, ResampleResult, Resample, Decimate, Biquad, BiquadCoefficients,
    SUBSAMPLE_INTERPOLATE, BLACKMAN_HARRIS, INCLUDE_LOWPASS, RESAMPLE_MULTITHREADED, NO_FILTER_REDUCTION,
    RESAMPLE_FIXED_RATIO, EXTRAPOLATE_ENDPOINTS, EXTEND_CONVOLUTION_MATH, RESAMPLER_FLUSHED, RESAMPLER_SNAP_OFFSET,
    RESAMPLE_STRICT_ORDER, DITHER_HIGHPASS, DITHER_FLAT, DITHER_LOWPASS, SHAPING_1ST_ORDER, SHAPING_2ND_ORDER,
    SHAPING_3RD_ORDER, SHAPING_ATH_CURVE, DECIMATE_MULTITHREADED, EXPORTED_SYMBOLS, wide, binding, decimate_batch_device,
    biquad_batch_device, ingest_batch_device, extrapolate_batch_device, process_and_flush_batch_device,
    process_batch_device, process_batch_planar_device, process_and_flush_batch_planar_device, ClipResampler,
    process_schedule_batch_device, process_schedule_batch_planar_device,
    process_schedule_clips_planar_device, adjoint_schedule_clips_planar_device, ClipWarper,
    decimate_batch_planar_device, decimate_clips_planar_device, process_and_flush_clips_planar_device, adjoint_clips_planar_device, ClipDecimator, biquad_batch_planar_device, biquad_clips_planar_device, ClipFilter,
    biquad_filter_clips_planar_device, lag_products_batch_device, ClipBiquad,
    STRETCH_FAST_FLAG, STRETCH_DUAL_FLAG, Stretcher, stretch_clips_batch_planar_device, ClipStretcher,
    stretch_clips_logged_batch_planar_device, stretch_adjoint_clips_planar_device, STRETCH_COPY,
)
