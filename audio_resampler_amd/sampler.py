"""Whole clips evaluated at a position curve that lies on the GPU — the 1-D, windowed-sinc counterpart of grid_sample: the wrappers of
resampleSampleClipsPlanarDevice, resampleSampleAdjointClipsPlanarDevice and resampleSamplePositionGradientClipsPlanarDevice, and ClipSampler,
which is differentiable in the samples and in the positions.

The position convention: a position is a double in input frames, and p = 0 is ALIGNED — output m is centred on input frame p[m], a fresh
context's position after resampleAdvancePosition(taps / 2).  p[m] = m / ratio resamples aligned; p[m] = m / ratio - taps / 2 is the plain
clip classes' output (ClipResampler, ClipWarper: their lead-in of half a filter length).  An offset, a ratio, a polynomial drift, an LFO
or an alignment path are torch expressions in front of the call, and autograd carries dL/dp to them.

The names live beside the binding (audio_resampler_amd.api), not in it: `binding(width)` here returns a namespace of them for that sample
width, built on api.binding(width) and on the helpers it hands out under `_private`, and handing out its own curve helpers the same way
(audio_resampler_amd.band builds on them); the module level is the 4-byte build."""
import types

from . import api


def _bind(width):
    B = api.binding(width)
    P = B._private
    smp_torch = "float64" if width == 64 else "float32"

    def _one_per_clip(n, *lists):
        if any(v is not None and len(v) != n for v in lists):
            raise ValueError("one entry per clip in every list")
        return max(n, 1)

    def sample_clips_planar_device(resamplers, d_ins, in_pitches, n_ins, d_positions, n_outs, d_outs, out_pitches):
        """resampleSampleClipsPlanarDevice: output m of clip i is resamplers[i]'s interpolator evaluated at the double d_positions[i][m]
        (device memory, in input frames; p = 0 is centred on frame 0) on the n_ins[i] frames at d_ins[i]; n_outs[i] frames of d_outs[i]
        are set, a position without a window (not finite, below -(taps / 2 + 1), at or past n_ins[i] + taps / 2) to exactly 0; pitches as
        in process_batch_planar_device.  The contexts are only read, and one may be listed any number of times.  Returns the launch
        count, 1 or 0 (raises if the call returned -1)."""
        n = len(resamplers)
        m = _one_per_clip(n, d_ins, in_pitches, n_ins, d_positions, n_outs, d_outs, out_pitches)
        rc = B.lib().resampleSampleClipsPlanarDevice(
            P._contexts(resamplers, m), n, P._dev_ptrs(d_ins, m), P._longs(in_pitches, m), P._ints(n_ins, m),
            P._dev_ptrs(d_positions, m), P._ints(n_outs, m), P._dev_ptrs(d_outs, m), P._longs(out_pitches, m))
        if rc < 0:
            raise RuntimeError("resampleSampleClipsPlanarDevice failed")
        return rc

    def sample_adjoint_clips_planar_device(resamplers, d_positions, n_outs, d_gouts, gout_pitches, d_gins, gin_pitches, n_ins):
        """resampleSampleAdjointClipsPlanarDevice: frames 0 .. n_ins[i]-1 of every channel of d_gins[i] are set to the transpose of
        sample_clips_planar_device's map applied to the n_outs[i] frames of d_gouts[i].  PRECONDITION: the positions of a clip do not
        decrease (sort them, and the gradient with them, where they do: ClipSampler's backward does).  A clip without outputs or without
        frames is not touched: nothing is zeroed.  Returns the launch count, 1 or 0 (raises if the call returned -1)."""
        n = len(resamplers)
        m = _one_per_clip(n, d_positions, n_outs, d_gouts, gout_pitches, d_gins, gin_pitches, n_ins)
        rc = B.lib().resampleSampleAdjointClipsPlanarDevice(
            P._contexts(resamplers, m), n, P._dev_ptrs(d_positions, m), P._ints(n_outs, m), P._dev_ptrs(d_gouts, m), P._longs(gout_pitches, m),
            P._dev_ptrs(d_gins, m), P._longs(gin_pitches, m), P._ints(n_ins, m))
        if rc < 0:
            raise RuntimeError("resampleSampleAdjointClipsPlanarDevice failed")
        return rc

    def sample_position_gradient_clips_planar_device(resamplers, d_ins, in_pitches, n_ins, d_positions, n_outs, d_gouts, gout_pitches, d_gpositions):
        """resampleSamplePositionGradientClipsPlanarDevice: the n_outs[i] doubles at d_gpositions[i] are set to dL/d positions for
        L = sum(gy * y), y sample_clips_planar_device's output and gy the n_outs[i] frames of d_gouts[i] — per output the slope of the
        interpolation cell the forward used, summed over the channels; interpolating contexts only.  Returns the launch count, 1 or 0
        (raises if the call returned -1)."""
        n = len(resamplers)
        m = _one_per_clip(n, d_ins, in_pitches, n_ins, d_positions, n_outs, d_gouts, gout_pitches, d_gpositions)
        rc = B.lib().resampleSamplePositionGradientClipsPlanarDevice(
            P._contexts(resamplers, m), n, P._dev_ptrs(d_ins, m), P._longs(in_pitches, m), P._ints(n_ins, m),
            P._dev_ptrs(d_positions, m), P._ints(n_outs, m), P._dev_ptrs(d_gouts, m), P._longs(gout_pitches, m), P._dev_ptrs(d_gpositions, m))
        if rc < 0:
            raise RuntimeError("resampleSamplePositionGradientClipsPlanarDevice failed")
        return rc

    def _curve_ptrs(p):
        """addresses of the rows of p [B, M] (float64, consecutive along M; a broadcast curve is one row listed B times)"""
        return [p.data_ptr() + i * p.stride(0) * 8 for i in range(p.shape[0])]

    def _monotone(p, outs, gy, *along):
        """(curve, gy, *along) in an order the adjoint kernels take: they bisect the curve, so they want positions that do not decrease.
        The check runs on the device, within outs; its one boolean is all that comes back.  A curve that fails it (reverse playback,
        scratching, a NaN) is sorted — stably, what lies past outs moved to the end first — and gy [B, C, M] and every tensor [B, M] of
        `along` gathered into the same order: A sums over the outputs, so A^T does not care about their order, as long as every output
        keeps what belongs to it."""
        import torch
        M = p.shape[1]
        past = torch.arange(M, device=p.device)[None, :] >= torch.tensor(outs, device=p.device)[:, None]
        if bool(((p[:, 1:] >= p[:, :-1]) | past[:, 1:]).all()):
            return (p, gy) + along
        curve, order = torch.sort(p.masked_fill(past, float("inf")), dim=1, stable=True)
        return (curve, torch.gather(gy, 2, order[:, None, :].expand(-1, gy.shape[1], -1))) + tuple(torch.gather(t, 1, order) for t in along)

    def _check_positions(positions, B_):
        import torch
        if not torch.is_tensor(positions) or positions.dtype not in (torch.float32, torch.float64) or positions.dim() not in (1, 2) or \
                (positions.dim() == 2 and B_ is not None and positions.shape[0] != B_):
            raise ValueError("positions: a float32 or float64 tensor [B, M] or [M]")

    def _outs(out_lengths, B_, M):
        if out_lengths is None:
            return [M] * B_
        outs = [int(v) for v in (out_lengths.tolist() if hasattr(out_lengths, "tolist") else out_lengths)]
        if len(outs) != B_ or any(v < 0 or v > M for v in outs):
            raise ValueError("out_lengths: one entry per clip, 0 .. M")
        return outs

    def _on_device(x, channels, **curves):
        """the samples on the GPU with consecutive frames, and every curve given (by its name in the message) beside them"""
        if not x.is_cuda:
            raise ValueError(f"expected a CUDA {smp_torch} tensor [B, {channels}, T]")
        for name, t in curves.items():
            if t is not None and t.device != x.device:
                raise ValueError(f"{name}: on the samples' device (they are not downloaded)")
        # (frames of a channel must be consecutive; any row pitch is taken as it is)
        return x.contiguous() if x.shape[2] and x.stride(2) != 1 else x

    def _rows(t, B_, M):
        """t [B, M] or [M] as float64 rows [B, M], consecutive along M — torch ops in front of the custom function: autograd sums a
        broadcast curve's gradient back and narrows it to the caller's dtype"""
        import torch
        t = t if t.dim() == 2 else t[None, :].expand(B_, M)
        if t.dtype != torch.float64:
            t = t.to(torch.float64)
        return t.contiguous() if M > 1 and t.stride(1) != 1 else t

    def _forward(ctx, x, p, clip, lengths, outs):
        ctx.save_for_backward(x, p)                               # (an edit of either in place before backward is caught)
        ctx.clip, ctx.lengths, ctx.outs = clip, lengths, outs
        return clip._sample(x, p, lengths, outs)

    def _backward(ctx, gy):
        import torch
        x, p = ctx.saved_tensors
        clip, lengths, outs = ctx.clip, ctx.lengths, ctx.outs
        need_x, need_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        B_, M = p.shape
        gx = torch.zeros(x.shape, dtype=gy.dtype, device=gy.device) if need_x else None       # (zero at and past lengths[i])
        gp = torch.zeros(B_, M, dtype=torch.float64, device=gy.device) if need_p else None     # (zero at and past out_lengths[i])
        if not B_ or not M:                                       # (no output: no context was ever needed)
            return gx, gp, None, None, None
        if not clip.pool:
            raise RuntimeError("the ClipSampler was closed before backward")
        lead = clip.pool[0]
        if not P._rows_readable(gy):
            gy = gy.contiguous()
        lead.set_stream(torch.cuda.current_stream(gy.device).cuda_stream)
        if need_x:
            curve, g = _monotone(p, outs, gy)
            (g_ptrs, g_pitch), (gx_ptrs, gx_pitch) = P._clip_ptrs(g), P._clip_ptrs(gx)
            sample_adjoint_clips_planar_device([lead] * B_, _curve_ptrs(curve), outs, g_ptrs, [g_pitch] * B_, gx_ptrs, [gx_pitch] * B_, lengths)
        if need_p:
            (x_ptrs, x_pitch), (gy_ptrs, gy_pitch) = P._clip_ptrs(x), P._clip_ptrs(gy)
            sample_position_gradient_clips_planar_device([lead] * B_, x_ptrs, [x_pitch] * B_, lengths, _curve_ptrs(p), outs, gy_ptrs, [gy_pitch] * B_,
                                                         _curve_ptrs(gp))
        return gx, gp, None, None, None

    _clip_sample_grad = P._grad_function("ClipSampleGrad", _forward, _backward)

    class ClipSampler:
        """Whole clips, channels-first, at a position curve on the GPU: x [B, C, T] (or [C, T]) and positions [B, M] (or [M], for every clip)
        in, y [B, C, M] out — y[i, c, m] is the windowed-sinc interpolator of this sampler's filter bank evaluated at positions[i, m] on
        x[i, c, :lengths[i]], ONE resampleSampleClipsPlanarDevice call on the tensors' own rows.  The positions are a CUDA tensor, float64
        or float32 (widened by a torch op), and are never downloaded; the output length is the curve's.

        The position convention: positions are in input frames and p = 0 is aligned — output m is centred on input frame p[m].
        p[m] = m / ratio resamples aligned (no lead-in); p[m] = m / ratio - taps / 2 is the plain clip classes' output.  Frames before
        the clip and at and past lengths[i] are silence (never read); a position that is not finite, below -(taps / 2 + 1) or at or past
        lengths[i] + taps / 2 gives exactly 0.  out_lengths[i] <= M limits clip i's outputs: y[i, :, out_lengths[i]:] is zero and grad_y
        there is not read.

        The bank's cut-off is fixed at construction, like ClipWarper's: the curve does not move it, so pick lowpass_ratio for the
        steepest step of the curve (a step of s > 1 input frames per output wants a cut-off of 1 / s or below against aliasing).

        Differentiable once, in both operands.  x: ONE resampleSampleAdjointClipsPlanarDevice call, the exact transpose; its kernel
        wants a curve that does not decrease, which backward checks on the device (one boolean read back), and a curve that fails the
        check — reverse playback, scratching — is sorted first, the gradient gathered into the same order, so it gets correct
        gradients too and monotone curves pay nothing.  positions: ONE resampleSamplePositionGradientClipsPlanarDevice call, elementwise —
        the slope of the interpolation cell the forward used (on a filter boundary the cell floor picks) — which comes back in the
        positions' dtype and shape; it needs SUBSAMPLE_INTERPOLATE (with the nearest filter it would be zero almost everywhere: a
        positions tensor that requires grad is refused there).  Without gradients the call is the forward launch alone.  Holds one
        Resampler, made on first use, which is only read."""

        def __init__(self, channels, taps=380, filters=380, flags=api.BLACKMAN_HARRIS | api.SUBSAMPLE_INTERPOLATE | api.INCLUDE_LOWPASS, lowpass_ratio=0.0):
            if flags & api.EXTRAPOLATE_ENDPOINTS:
                raise ValueError("ClipSampler: EXTRAPOLATE_ENDPOINTS is not linear in the samples (no adjoint)")
            self.channels, self.taps, self.flags = channels, taps, flags
            self._init = (channels, taps, filters, float(lowpass_ratio), flags)
            self.pool = []

        def close(self):
            for r in self.pool:
                r.close()
            self.pool = []

        def _sample(self, x, p, lengths, outs):
            """the forward launch: x [B, C, T] and p [B, M] float64 on the GPU, detached"""
            import torch
            B_, Cn, M = x.shape[0], x.shape[1], p.shape[1]
            y = torch.zeros(B_, Cn, M, dtype=x.dtype, device=x.device)            # (zero at and past out_lengths[i])
            if B_ and M:
                P._pool_ready(self.pool, 1, lambda: B.Resampler(*self._init), torch.cuda.current_stream(x.device).cuda_stream)
                (xs, x_pitch), (ys, y_pitch) = P._clip_ptrs(x), P._clip_ptrs(y)
                sample_clips_planar_device([self.pool[0]] * B_, xs, [x_pitch] * B_, lengths, _curve_ptrs(p), outs, ys, [y_pitch] * B_)
            return y

        def __call__(self, x, positions, lengths=None, out_lengths=None):
            import torch
            # (the GPU is asked for behind the host checks: they need none)
            x, B_, Cn, T, lengths = P._clip_input(x, self.channels, lengths, cuda=False, strided="keep")
            _check_positions(positions, B_)
            M = positions.shape[-1]
            outs = _outs(out_lengths, B_, M)
            grad = torch.is_grad_enabled()
            if grad and positions.requires_grad and not self.flags & api.SUBSAMPLE_INTERPOLATE:
                raise ValueError("ClipSampler: without SUBSAMPLE_INTERPOLATE the position gradient is zero almost everywhere")
            x = _on_device(x, self.channels, positions=positions)
            p = _rows(positions, B_, M)
            if grad and (x.requires_grad or p.requires_grad):
                return _clip_sample_grad().apply(x, p, self, lengths, outs)
            return self._sample(x.detach(), p.detach(), lengths, outs)

    _private = types.SimpleNamespace(_one_per_clip=_one_per_clip, _curve_ptrs=_curve_ptrs, _monotone=_monotone, _check_positions=_check_positions,
                                     _outs=_outs, _on_device=_on_device, _rows=_rows)       # (what audio_resampler_amd.band builds on)
    return types.SimpleNamespace(**{k: v for k, v in locals().items() if not k.startswith("_") and k not in ("width", "B", "P", "smp_torch")}, width=width,
                                 _private=_private)


_bound = {}


def binding(width=32):
    if width not in _bound:
        _bound[width] = _bind(width)
    return _bound[width]


globals().update({k: v for k, v in vars(binding(32)).items() if k not in ("width", "_private")})      # module level = the 4-byte build
