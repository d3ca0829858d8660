"""Gradients of whole clips with respect to their ratio curve: resampleRateGradientScheduleClipsPlanarDevice's wrapper and ClipRateWarper,
a ClipWarper whose `ratios` may be a torch tensor that requires grad.

The names live beside the binding (audio_resampler_amd.api), not in it: `binding(width)` here returns a namespace of the two for that
sample width, built on api.binding(width) and on the helpers it hands out under `_private`; the module level is the 4-byte build."""
import ctypes as C
import types

from . import api


def _bind(width):
    B = api.binding(width)
    P = B._private

    def rate_gradient_schedule_clips_planar_device(resamplers, d_ins, in_pitches, d_gouts, gout_pitches, n_outs, n_ins, ratios, d_grads):
        """resampleRateGradientScheduleClipsPlanarDevice: the gradient of whole clips made block by block with respect to the blocks' ratios.
        n_ins[i] and ratios[i] are clip i's blocks (frames and ratio of each); the len(n_ins[i]) doubles at d_grads[i] are set to
        dL/d ratios[i] for L = sum(gy * y), y the schedule clips entry's output for the samples at d_ins[i] (a fresh context of
        resamplers[i]'s parameters, the blocks in turn, then the flush) and gy the first n_outs[i] frames of d_gouts[i]; pitches as in
        process_batch_planar_device.  The contexts are only read, and one may be listed any number of times.  Returns the launch count
        (raises if the call returned -1)."""
        n = len(resamplers)
        if not (len(d_ins) == len(d_gouts) == len(n_outs) == len(n_ins) == len(ratios) == len(d_grads) == n):
            raise ValueError("one entry per clip in every list")
        if any(len(n_ins[i]) != len(ratios[i]) for i in range(n)):
            raise ValueError("n_ins[i] and ratios[i] must have one entry per block")
        m = max(n, 1)
        counts = [len(v) for v in n_ins]
        frames, rates = P._rows(C.c_int, int, n_ins), P._rows(C.c_double, float, ratios)
        rc = B.lib().resampleRateGradientScheduleClipsPlanarDevice(
            P._contexts(resamplers, m), n, P._ints(counts, m), P._dev_ptrs(d_ins, m), P._longs(in_pitches, m),
            P._dev_ptrs(d_gouts, m), P._longs(gout_pitches, m), P._ints(n_outs, m), P._table(frames, m), P._table(rates, m), P._dev_ptrs(d_grads, m))
        if rc < 0:
            raise RuntimeError("resampleRateGradientScheduleClipsPlanarDevice failed")
        return rc

    def _forward(ctx, x, r, y, clip, blocks, rates, made):
        ctx.save_for_backward(x)                                  # (an edit of x in place before backward is caught)
        ctx.clip, ctx.blocks, ctx.rates, ctx.made, ctx.r_like = clip, blocks, rates, made, (tuple(r.shape), r.dtype, r.device)
        return y.view_as(y)

    def _backward(ctx, gy):
        import torch
        (x,) = ctx.saved_tensors
        clip, (r_shape, r_dtype, r_device) = ctx.clip, ctx.r_like
        need_x, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        B_ = x.shape[0]
        if not B_:                                                # (no clip: no context was ever needed)
            return (torch.zeros(x.shape, dtype=gy.dtype, device=gy.device) if need_x else None,
                    torch.zeros(r_shape, dtype=r_dtype, device=r_device) if need_r else None, None, None, None, None, None)
        if not clip.pool:
            raise RuntimeError("the ClipRateWarper was closed before backward")
        lead, gx, gr = clip.pool[0], None, None
        if need_x:
            gx, (gy_ptrs, gy_pitches, gx_ptrs, gx_pitches) = P._clip_backward(x.shape, gy, P._rows_readable, lead)
            B.adjoint_schedule_clips_planar_device([lead] * B_, gy_ptrs, gy_pitches, ctx.made, gx_ptrs, gx_pitches, ctx.blocks, ctx.rates)
        if need_r:
            if not P._rows_readable(gy):
                gy = gy.contiguous()
            lead.set_stream(torch.cuda.current_stream(gy.device).cuda_stream)
            g = torch.zeros(r_shape, dtype=torch.float64, device=gy.device)      # (zero past a clip's block count)
            (x_ptrs, x_pitch), (gy_ptrs, gy_pitch), step = P._clip_ptrs(x), P._clip_ptrs(gy), r_shape[1] * 8
            rate_gradient_schedule_clips_planar_device([lead] * B_, x_ptrs, [x_pitch] * B_, gy_ptrs, [gy_pitch] * B_, ctx.made, ctx.blocks, ctx.rates,
                                                       [g.data_ptr() + i * step for i in range(B_)])
            gr = g.to(dtype=r_dtype).to(r_device)
        return gx, gr, None, None, None, None, None

    _clip_rate_warp_grad = P._grad_function("ClipRateWarpGrad", _forward, _backward)

    class ClipRateWarper(B.ClipWarper):
        """ClipWarper whose ratio curve can be learned: `ratios` may also be a torch tensor that requires grad — a scalar, [B] or [B, K],
        float32 or float64, on the CPU or the GPU (its values are downloaded once, for the planner).  Where it does (and grad mode is on) y
        is attached to the graph through x and through the ratios, broadcast to [B, K] by torch ops in front of the custom function so that
        autograd sums the gradient back to the caller's shape.  Backward makes the calls its inputs need: ONE
        resampleAdjointScheduleClipsPlanarDevice call for x (ClipWarper's bits), ONE resampleRateGradientScheduleClipsPlanarDevice call for
        the ratios — the slope of the interpolation cell the forward used, the output counts held fixed — which comes back in the ratios'
        dtype and on their device, zero for entries past a clip's block count.  Differentiable once; out_lengths carries no gradient;
        without gradients the call is ClipWarper's, bit for bit.  The context must interpolate (SUBSAMPLE_INTERPOLATE): with the nearest
        filter the gradient would be zero almost everywhere."""

        def __init__(self, channels, taps=380, filters=380, flags=api.BLACKMAN_HARRIS | api.SUBSAMPLE_INTERPOLATE | api.INCLUDE_LOWPASS, lowpass_ratio=0.0,
                     block=1024, max_batch=1024):
            super().__init__(channels, taps, filters, flags, lowpass_ratio, block, max_batch)
            if not flags & api.SUBSAMPLE_INTERPOLATE:
                raise ValueError("ClipRateWarper: without SUBSAMPLE_INTERPOLATE the ratio gradient is zero almost everywhere")

        def __call__(self, x, ratios, lengths=None):
            import torch
            if not (torch.is_tensor(ratios) and ratios.requires_grad and torch.is_grad_enabled()):
                return super().__call__(x, ratios.detach() if torch.is_tensor(ratios) else ratios, lengths)
            # the parent's checks in the parent's order (x, lengths, ratios; the GPU is asked for by its call below), on the values downloaded once
            x, B_, Cn, T, lengths = P._clip_input(x, self.channels, lengths, cuda=False, strided="keep")
            if ratios.dtype not in (torch.float32, torch.float64):
                raise ValueError("ratios that require grad: a float32 or float64 tensor")
            host = ratios.detach().cpu().numpy()
            blocks, rates = self.blocks(lengths, host)
            if x.is_cuda and x.shape[2] and x.stride(2) != 1:
                x = x.contiguous()
            y, out_lengths = super().__call__(x.detach(), host, lengths)         # (the forward alone: ClipWarper's bits)
            K = max((len(b) for b in blocks), default=1)
            r = ratios.expand(B_, K) if ratios.dim() == 0 else ratios[:, None].expand(B_, K) if ratios.dim() == 1 else ratios[:, :K]
            return _clip_rate_warp_grad().apply(x, r, y, self, blocks, rates, out_lengths.tolist()), out_lengths

    return types.SimpleNamespace(**{k: v for k, v in locals().items() if not k.startswith("_") and k not in ("width", "B", "P")}, width=width)


_bound = {}


def binding(width=32):
    if width not in _bound:
        _bound[width] = _bind(width)
    return _bound[width]


globals().update({k: v for k, v in vars(binding(32)).items() if k != "width"})      # module level = the 4-byte build
