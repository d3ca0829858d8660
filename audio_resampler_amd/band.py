"""Whole clips at a position curve on the GPU, BAND-LIMITED PER OUTPUT from a ladder of filter banks — what a mip chain is to a texture
sampler: the wrappers of resampleSampleBandClipsPlanarDevice, resampleSampleBandAdjointClipsPlanarDevice and
resampleSampleBandGradientsClipsPlanarDevice, and ClipBandSampler, which is differentiable in the samples, the positions and the levels.

ClipSampler's bank has one cut-off for the whole curve; on a curve whose step varies — a pitch contour, a drift, scratching, a learned
warp — the clip aliases wherever the curve steps faster than that bank allows, or is low-passed everywhere for its steepest moment.  Here
several banks of one shape at descending cut-offs form a ladder, and a level curve beside the positions picks, per output, two
neighbouring rungs and their blend: level k means rung k, level k + lam the blend (1 - lam) rung k + lam rung k + 1.  The kernels read only
the one or two banks an output needs.  Positions as in audio_resampler_amd.sampler: doubles in input frames, p = 0 aligned.

The names live beside the binding (audio_resampler_amd.api) and beside audio_resampler_amd.sampler, in neither: `binding(width)` here
returns a namespace of them for that sample width, built on the curve helpers sampler.binding(width) hands out under `_private` — the list
and curve checks, the rows, the sort of a curve that decreases — so that only what is the ladder's stands here; the module level is the
4-byte build."""
import math
import types

from . import api, sampler


def _bind(width):
    B = api.binding(width)
    P = B._private
    S = sampler.binding(width)._private                           # (the curve helpers: ClipSampler's own)
    _one_per_clip, _curve_ptrs = S._one_per_clip, S._curve_ptrs

    def _ladder(resamplers, rungs):
        """the contexts of a call: `resamplers` holds len / rungs clips' ladders, rung k of clip i at [i * rungs + k]"""
        rungs = int(rungs)
        if rungs < 1 or len(resamplers) % rungs:
            raise ValueError("resamplers: rungs contexts per clip")
        return rungs, len(resamplers) // rungs

    def sample_band_clips_planar_device(resamplers, rungs, d_ins, in_pitches, n_ins, d_positions, d_levels, n_outs, d_outs, out_pitches):
        """resampleSampleBandClipsPlanarDevice: sample_clips_planar_device on a ladder of `rungs` contexts per clip (rung k of clip i is
        resamplers[i * rungs + k]; one shape, all interpolating, only read) with a level per output in d_levels[i] (doubles in device
        memory beside d_positions[i]).  A level l: not above 0 (or a NaN) is rung 0, at or above rungs - 1 the last rung, else rung
        floor(l) blended with the next by l - floor(l); on a whole level the output is sample_clips_planar_device's on that rung bit for
        bit.  Returns the launch count, 1 or 0 (raises if the call returned -1)."""
        rungs, n = _ladder(resamplers, rungs)
        m = _one_per_clip(n, d_ins, in_pitches, n_ins, d_positions, d_levels, n_outs, d_outs, out_pitches)
        rc = B.lib().resampleSampleBandClipsPlanarDevice(
            P._contexts(resamplers, max(len(resamplers), 1)), n, rungs, P._dev_ptrs(d_ins, m), P._longs(in_pitches, m), P._ints(n_ins, m),
            P._dev_ptrs(d_positions, m), P._dev_ptrs(d_levels, m), P._ints(n_outs, m), P._dev_ptrs(d_outs, m), P._longs(out_pitches, m))
        if rc < 0:
            raise RuntimeError("resampleSampleBandClipsPlanarDevice failed")
        return rc

    def sample_band_adjoint_clips_planar_device(resamplers, rungs, d_positions, d_levels, n_outs, d_gouts, gout_pitches, d_gins, gin_pitches, n_ins):
        """resampleSampleBandAdjointClipsPlanarDevice: frames 0 .. n_ins[i]-1 of every channel of d_gins[i] are set to the transpose of
        sample_band_clips_planar_device's map applied to the n_outs[i] frames of d_gouts[i].  PRECONDITION: the positions of a clip do not
        decrease (sort them, and the gradient and the levels with them, where they do: ClipBandSampler's backward does); the levels may
        be anything.  A clip without outputs or without frames is not touched.  Returns the launch count, 1 or 0 (raises if the call
        returned -1)."""
        rungs, n = _ladder(resamplers, rungs)
        m = _one_per_clip(n, d_positions, d_levels, n_outs, d_gouts, gout_pitches, d_gins, gin_pitches, n_ins)
        rc = B.lib().resampleSampleBandAdjointClipsPlanarDevice(
            P._contexts(resamplers, max(len(resamplers), 1)), n, rungs, P._dev_ptrs(d_positions, m), P._dev_ptrs(d_levels, m), P._ints(n_outs, m),
            P._dev_ptrs(d_gouts, m), P._longs(gout_pitches, m), P._dev_ptrs(d_gins, m), P._longs(gin_pitches, m), P._ints(n_ins, m))
        if rc < 0:
            raise RuntimeError("resampleSampleBandAdjointClipsPlanarDevice failed")
        return rc

    def sample_band_gradients_clips_planar_device(resamplers, rungs, d_ins, in_pitches, n_ins, d_positions, d_levels, n_outs, d_gouts, gout_pitches,
                                                  d_gpositions, d_glevels):
        """resampleSampleBandGradientsClipsPlanarDevice: for L = sum(gy * y) of sample_band_clips_planar_device's output, the n_outs[i]
        doubles at d_gpositions[i] are set to dL/d positions (the blended slope of the cell the forward used) and those at d_glevels[i]
        to dL/d levels (the difference of the level's two rungs; the closed ends 0 and rungs - 1 pass it, levels outside, a NaN, a
        single rung and outputs without a window get exactly 0).  Either list may be None — not wanted, and not paid for; not both.
        Returns the launch count, 1 or 0 (raises if the call returned -1)."""
        rungs, n = _ladder(resamplers, rungs)
        m = _one_per_clip(n, d_ins, in_pitches, n_ins, d_positions, d_levels, n_outs, d_gouts, gout_pitches, d_gpositions, d_glevels)
        rc = B.lib().resampleSampleBandGradientsClipsPlanarDevice(
            P._contexts(resamplers, max(len(resamplers), 1)), n, rungs, P._dev_ptrs(d_ins, m), P._longs(in_pitches, m), P._ints(n_ins, m),
            P._dev_ptrs(d_positions, m), P._dev_ptrs(d_levels, m), P._ints(n_outs, m), P._dev_ptrs(d_gouts, m), P._longs(gout_pitches, m),
            None if d_gpositions is None else P._dev_ptrs(d_gpositions, m), None if d_glevels is None else P._dev_ptrs(d_glevels, m))
        if rc < 0:
            raise RuntimeError("resampleSampleBandGradientsClipsPlanarDevice failed")
        return rc

    def _forward(ctx, x, p, lev, clip, lengths, outs):
        ctx.save_for_backward(x, p, lev)                          # (an edit of any in place before backward is caught)
        ctx.clip, ctx.lengths, ctx.outs = clip, lengths, outs
        return clip._sample(x, p, lev, lengths, outs)

    def _backward(ctx, gy):
        import torch
        x, p, lev = ctx.saved_tensors
        clip, lengths, outs = ctx.clip, ctx.lengths, ctx.outs
        need_x, need_p, need_l = ctx.needs_input_grad[:3]
        B_, M = p.shape
        gx = torch.zeros(x.shape, dtype=gy.dtype, device=gy.device) if need_x else None       # (zero at and past lengths[i])
        gp = torch.zeros(B_, M, dtype=torch.float64, device=gy.device) if need_p else None     # (zero at and past out_lengths[i])
        gl = torch.zeros(B_, M, dtype=torch.float64, device=gy.device) if need_l else None
        if not B_ or not M:                                       # (no output: no context was ever needed)
            return gx, gp, gl, None, None, None
        if not clip.pool:
            raise RuntimeError("the ClipBandSampler was closed before backward")
        if not P._rows_readable(gy):
            gy = gy.contiguous()
        for rung in clip.pool:                                    # (the entries want a call's contexts on one stream)
            rung.set_stream(torch.cuda.current_stream(gy.device).cuda_stream)
        ladder, K = clip.pool * B_, len(clip.pool)
        if need_x:
            # ClipSampler's rule: a curve that decreases within out_lengths is sorted, and gy AND THE LEVELS gathered into the same order
            curve, g, lv = S._monotone(p, outs, gy, lev)
            (g_ptrs, g_pitch), (gx_ptrs, gx_pitch) = P._clip_ptrs(g), P._clip_ptrs(gx)
            sample_band_adjoint_clips_planar_device(ladder, K, _curve_ptrs(curve), _curve_ptrs(lv), outs, g_ptrs, [g_pitch] * B_, gx_ptrs, [gx_pitch] * B_,
                                                    lengths)
        if need_p or need_l:
            (x_ptrs, x_pitch), (gy_ptrs, gy_pitch) = P._clip_ptrs(x), P._clip_ptrs(gy)
            sample_band_gradients_clips_planar_device(ladder, K, x_ptrs, [x_pitch] * B_, lengths, _curve_ptrs(p), _curve_ptrs(lev), outs, gy_ptrs,
                                                      [gy_pitch] * B_, _curve_ptrs(gp) if need_p else None, _curve_ptrs(gl) if need_l else None)
        return gx, gp, gl, None, None, None

    _clip_band_grad = P._grad_function("ClipBandSampleGrad", _forward, _backward)

    class ClipBandSampler:
        """Whole clips, channels-first, at a position curve on the GPU with a cut-off PER OUTPUT: x [B, C, T] (or [C, T]), positions
        [B, M] (or [M], for every clip) and levels [B, M] (or [M]; None: automatic) in, y [B, C, M] out — ClipSampler on a ladder of
        filter banks, ONE resampleSampleBandClipsPlanarDevice call on the tensors' own rows.

        The ladder: one bank per entry of `cutoffs` — 1 to 8 of them, strictly decreasing, in (0, 1], as fractions of the input Nyquist;
        1.0 is a bank without low-pass — all of one shape (taps, filters, window).  Level k is rung k; a level between two whole
        numbers blends the two neighbouring rungs' outputs linearly; a level not above 0 (or a NaN) is rung 0, one at or above
        len(cutoffs) - 1 the last rung.  Between rungs the filter is therefore a blend of two windowed sincs, not a sinc at the
        interpolated cut-off: its response steps down in two stages across the cell, and a denser ladder tightens it.  With the taps
        fixed, the transition band of a low rung is as wide in Hz as the top rung's — relative to its cut-off it is wider, so the
        low rungs guard less sharply; `guard` below 1 moves every cut-off choice down to make room.

        levels=None picks them from the curve (levels_of): the step s[m] = |p[m+1] - p[m-1]| / 2 in input frames per output (one-sided
        at the two ends of out_lengths[i], 1 for a single output), the target cut-off guard / max(s, 1), and the level at which the
        ladder, piecewise linear in the log of the cut-off, reaches it: sum_k clamp((ln c_k - ln target) / (ln c_k - ln c_{k+1}), 0, 1) —
        0 for a step of 1 or less, len(cutoffs) - 1 from 1 / c_last up.  A step that is not finite gives a NaN level, which the kernels
        read as level 0.  The automatic levels are made by torch ops on positions.detach(): no gradient flows through them.  levels
        given: a float32 or float64 tensor on the samples' device, never downloaded; it may require grad.  levels_of returns what
        levels=None uses, so a caller can bias or smooth it.

        Positions, lengths, out_lengths and the silence around a clip are ClipSampler's.  Differentiable once in x, positions and levels:
        ONE resampleSampleBandAdjointClipsPlanarDevice call serves x (a curve that decreases is sorted first, as ClipSampler sorts it,
        with the gradient and the levels gathered into the same order), ONE resampleSampleBandGradientsClipsPlanarDevice call positions
        and levels together, with NULL for whichever is not needed.  The level gradient is the difference of the level's two rungs; at
        the closed ends 0 and len(cutoffs) - 1 it passes (a learned level that starts on a rung is not stuck there), outside them it is
        zero.  Gradients come back in the caller's dtype and shape.  Holds one Resampler per rung, made on first use and only read."""

        def __init__(self, channels, cutoffs=(1.0, 2 ** -0.5, 0.5, 2 ** -1.5, 0.25), taps=380, filters=380,
                     flags=api.BLACKMAN_HARRIS | api.SUBSAMPLE_INTERPOLATE | api.INCLUDE_LOWPASS, guard=1.0):
            if flags & api.EXTRAPOLATE_ENDPOINTS:
                raise ValueError("ClipBandSampler: EXTRAPOLATE_ENDPOINTS is not linear in the samples (no adjoint)")
            if not flags & api.SUBSAMPLE_INTERPOLATE:
                raise ValueError("ClipBandSampler: the rungs are blended within one interpolation cell: SUBSAMPLE_INTERPOLATE is needed")
            try:
                cutoffs = tuple(float(c) for c in cutoffs)
            except TypeError:
                raise ValueError("cutoffs: 1 to 8 cut-offs in (0, 1], strictly decreasing") from None
            if not 1 <= len(cutoffs) <= 8 or not all(0.0 < c <= 1.0 for c in cutoffs) or any(b >= a for a, b in zip(cutoffs, cutoffs[1:])):
                raise ValueError("cutoffs: 1 to 8 cut-offs in (0, 1], strictly decreasing")
            guard = float(guard)
            if not (guard > 0.0 and math.isfinite(guard)):
                raise ValueError("guard: a positive factor on the target cut-off")
            self.channels, self.taps, self.flags, self.cutoffs, self.guard = channels, taps, flags, cutoffs, guard
            self._init = [(channels, taps, filters, c, flags | api.INCLUDE_LOWPASS) for c in cutoffs]   # (resampleInit clears the flag at 1.0)
            self._log = [math.log(c) for c in cutoffs]
            self.pool = []

        def close(self):
            for r in self.pool:
                r.close()
            self.pool = []

        def _levels(self, p, outs):
            """the automatic levels of p [B, M] float64 (detached) within outs — torch ops on p's device"""
            import torch
            B_, M = p.shape
            if not B_ or not M:
                return torch.zeros(B_, M, dtype=torch.float64, device=p.device)
            n = torch.tensor(outs, dtype=torch.int64, device=p.device)[:, None]
            m = torch.arange(M, dtype=torch.int64, device=p.device)[None, :].expand(B_, M)
            lo, hi = (m - 1).clamp(min=0), torch.minimum(m + 1, (n - 1).clamp(min=0).expand(B_, M))
            span = (hi - lo).to(torch.float64)
            step = (torch.gather(p, 1, hi) - torch.gather(p, 1, lo)).abs() / span.clamp(min=1.0)
            step = torch.where(span > 0, step, torch.ones_like(step))                          # (a single output; what lies past out_lengths)
            step = torch.where(torch.isfinite(step), step, torch.full_like(step, float("nan")))
            at = torch.log(self.guard / step.clamp(min=1.0))
            level = step * 0.0                                                                  # (a NaN stays one, whatever the ladder)
            for k in range(len(self._log) - 1):
                level = level + ((self._log[k] - at) / (self._log[k] - self._log[k + 1])).clamp(0.0, 1.0)
            return torch.where(m < n, level, torch.zeros_like(level))

        def levels_of(self, positions, out_lengths=None):
            """what levels=None uses for this curve: [B, M] float64 on the positions' device, no graph attached (B = len(out_lengths), or
            1, for positions [M]); zero at and past out_lengths[i]"""
            import torch
            S._check_positions(positions, None)
            p = positions.detach()
            if p.dim() == 1:
                p = p[None, :].expand(1 if out_lengths is None else len(out_lengths), p.shape[0])
            return self._levels(p.to(torch.float64), S._outs(out_lengths, p.shape[0], p.shape[1]))

        def _sample(self, x, p, lev, lengths, outs):
            """the forward launch: x [B, C, T], p and lev [B, M] float64 on the GPU, detached"""
            import torch
            B_, Cn, M = x.shape[0], x.shape[1], p.shape[1]
            y = torch.zeros(B_, Cn, M, dtype=x.dtype, device=x.device)            # (zero at and past out_lengths[i])
            if B_ and M:
                made = iter(self._init[len(self.pool):])
                P._pool_ready(self.pool, len(self._init), lambda: B.Resampler(*next(made)), torch.cuda.current_stream(x.device).cuda_stream)
                (xs, x_pitch), (ys, y_pitch) = P._clip_ptrs(x), P._clip_ptrs(y)
                sample_band_clips_planar_device(self.pool * B_, len(self.pool), xs, [x_pitch] * B_, lengths, _curve_ptrs(p), _curve_ptrs(lev), outs,
                                                ys, [y_pitch] * B_)
            return y

        def __call__(self, x, positions, levels=None, lengths=None, out_lengths=None):
            import torch
            # (the GPU is asked for behind the host checks: they need none)
            x, B_, Cn, T, lengths = P._clip_input(x, self.channels, lengths, cuda=False, strided="keep")
            S._check_positions(positions, B_)
            M = positions.shape[-1]
            outs = S._outs(out_lengths, B_, M)
            if levels is not None and (not torch.is_tensor(levels) or levels.dtype not in (torch.float32, torch.float64) or levels.dim() not in (1, 2) or
                                       levels.shape[-1] != M or (levels.dim() == 2 and levels.shape[0] != B_)):
                raise ValueError("levels: a float32 or float64 tensor [B, M] or [M], or None")
            x = S._on_device(x, self.channels, positions=positions, levels=levels)
            p = S._rows(positions, B_, M)
            lev = self._levels(p.detach(), outs) if levels is None else S._rows(levels, B_, M)
            if torch.is_grad_enabled() and (x.requires_grad or p.requires_grad or lev.requires_grad):
                return _clip_band_grad().apply(x, p, lev, self, lengths, outs)
            return self._sample(x.detach(), p.detach(), lev.detach(), lengths, outs)

    return types.SimpleNamespace(**{k: v for k, v in locals().items() if not k.startswith("_") and k not in ("width", "B", "P", "S")}, width=width)


_bound = {}


def binding(width=32):
    if width not in _bound:
        _bound[width] = _bind(width)
    return _bound[width]


globals().update({k: v for k, v in vars(binding(32)).items() if k != "width"})      # module level = the 4-byte build
