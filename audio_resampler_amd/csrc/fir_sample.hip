// fir_sample.hip — whole clips evaluated at a position curve that lies in device memory (gfx950): the kernels of
// resampleSampleClipsPlanarDevice, resampleSampleAdjointClipsPlanarDevice and resampleSamplePositionGradientClipsPlanarDevice.  The 1-D,
// windowed-sinc counterpart of grid_sample: no planner, no context state, no history — the context supplies its bank and flags.
//
// A position p (a double, in input frames) of a clip of N frames: whole = floor (p), fr = (p - whole) * F (neither fused), fi = floor (fr) and
// frac = fr - fi on an interpolating context, fi = floor (fr + 0.5) and frac = 0 on a nearest-filter one; tap t reads input frame
// whole - half + 1 + t — locate ()'s arithmetic with off = p, so that p = 0 is centred on frame 0.  Frames below 0 or at and past N are
// silence: their taps are LEFT OUT, not multiplied by zero.  A position that is not finite, below -(half + 1) or at or past N + half has no
// window at all: the comparison is made on the double, before any conversion to int, and such an output is exactly 0, reads nothing and
// has no term in either gradient.  (p - whole can round up to 1 for a tiny negative p, and fi to F: taken as fi = F - 1, frac = 1 — the
// same value and weight from rows inside the bank, and the slope of the cell p lies in.)
//
// Every launch is one flattened task space over the call; a workgroup finds its item by bisection over the items' first tasks (as
// fir_rate_grad.hip does), so one long clip and a thousand short ones spread over the chip alike.  No atomics, no counters: every value is
// one fixed tree of its own clip's terms whatever the batch, the item's place in it, the layout, the pitches or the stream.
//   fir_sample_kernel          a task is a tile of SM_TILE consecutive outputs, a lane one output: its position read coalesced, the
//                              samples read from global memory as they lie, per channel the fp64 chains of explicit fused multiply-adds
//                              with bank rows fi and fi + 1, t ascending — SM_CH channels' chains in flight together — then the
//                              reference's lerp.  The bank (580 KB at the defaults) does not fit the LDS and is served from L2, as in
//                              fir_rate_grad_tile_kernel.
//   fir_sample_adjoint_kernel  a task is a tile of ADJ_TILE consecutive INPUT frames and one channel group, a lane one frame j.
//                              PRECONDITION: the item's positions do not decrease.  The outputs whose windows hold j are then one range,
//                              found by bisection on the position array itself (on the doubles: a position far out of range, or an
//                              infinity, sorts where it lies; a NaN counts as +infinity), and walked by adj_walk — fir_adjoint.hip's
//                              blocks kernel's walk, the same weights in the same order — with the positions as its source.  On a curve
//                              that decreases somewhere the sums are unspecified, and every index still lies in [0, M], every row inside
//                              the bank: an output in the range whose position has no window is placed where no frame is.
//   fir_sample_slope_kernel    a map: a lane sets gp [m] = sum_c gy [c, m] D [c, m], D = F * (fir_rate_grad_tile_kernel's chain of
//                              (bank [fi + 1][t] - bank [fi][t]) x): the slope of the cell floor picks, no average on a boundary.
//
// Compiled with -ffp-contract=off: the only fused operations are the chains' explicit ones.
#include <cstring>
#include "fir_sample_common.hip.h"
#include "staging.hip.h"

namespace {

template <bool INTERP>
__device__ __forceinline__ void sample_output (const ArtSampleItem &it, unsigned int m)
{
    const int T = it.T, half = T / 2, N = it.in_frames, C = it.C;
    Pos pos;

    if (!sample_locate<INTERP> (it.pos [m], N, T, it.F, pos)) {
        for (int c = 0; c < C; ++c) sample_store (it, c, m, (art_s) 0);
        return;
    }
    if (!INTERP && !it.lowpass && (pos.fi % it.F) == 0) {      // the pass-through: direct_sample ()'s copy
        const int j = pos.ip + pos.fi / it.F;
        for (int c = 0; c < C; ++c) {
            art_s v = 0;
            if (j >= 0 && j < N) v = it.in_pitch ? it.in [(size_t) c * it.in_pitch + j] : it.in [(size_t) j * C + c];
            sample_store (it, c, m, v);
        }
        return;
    }

    const int j0 = pos.ip - half + 1;                          // input frame of tap 0; the taps that read a frame of the clip are [t_lo, t_hi)
    const int t_lo = max (0, -j0), t_hi = min (T, N - j0);
    const art_s *const row_lo = it.bank + (size_t) pos.fi * T, *const row_hi = row_lo + (INTERP ? T : 0);
    const long step = it.in_pitch ? 1 : C;

    for (int c0 = 0; c0 < C; c0 += SM_CH) {
        double s0 [SM_CH], s1 [SM_CH];
        long at [SM_CH];
#pragma unroll
        for (int u = 0; u < SM_CH; ++u) {                      // (a chain past the last channel repeats it, and is dropped)
            const int c = min (c0 + u, C - 1);
            s0 [u] = 0.0; s1 [u] = 0.0;
            at [u] = it.in_pitch ? (long) c * it.in_pitch + j0 : (long) j0 * C + c;
        }
        for (int t = t_lo; t < t_hi; ++t) {
            const double b0 = (double) row_lo [t], b1 = (double) row_hi [t];
#pragma unroll
            for (int u = 0; u < SM_CH; ++u) {
                const double v = (double) it.in [at [u] + t * step];
                s0 [u] = fused (b0, v, s0 [u]);
                if (INTERP) s1 [u] = fused (b1, v, s1 [u]);
            }
        }
#pragma unroll
        for (int u = 0; u < SM_CH; ++u) {
            const int c = c0 + u;
            if (c < C) {
                art_s y;
                if (INTERP) {
                    const double left = s0 [u] * (1.0 - pos.frac), right = s1 [u] * pos.frac;
                    y = (art_s)(left + right);
                }
                else y = (art_s) s0 [u];
                sample_store (it, c, m, y);
            }
        }
    }
}

__global__ __launch_bounds__ (SM_TILE)
void fir_sample_kernel (const ArtSampleItem *items, int count)
{
    const unsigned int task = blockIdx.x;
    const ArtSampleItem &it = items [sample_item_of (items, count, task)];
    const unsigned int m = (task - it.task0) * SM_TILE + threadIdx.x;
    if (m >= it.gy_frames) return;
    if (it.interpolate) sample_output<true> (it, m); else sample_output<false> (it, m);
}

__global__ __launch_bounds__ (SM_TILE)
void fir_sample_slope_kernel (const ArtSampleItem *items, int count)
{
    const unsigned int task = blockIdx.x;
    const ArtSampleItem &it = items [sample_item_of (items, count, task)];
    const unsigned int m = (task - it.task0) * SM_TILE + threadIdx.x;
    if (m >= it.gy_frames) return;

    const int T = it.T, half = T / 2, N = it.in_frames, C = it.C;
    Pos pos;
    double s = 0.0;
    if (sample_locate<true> (it.pos [m], N, T, it.F, pos)) {
        const int j0 = pos.ip - half + 1;
        const int t_lo = max (0, -j0), t_hi = min (T, N - j0);
        const art_s *const row_lo = it.bank + (size_t) pos.fi * T, *const row_hi = row_lo + T;
        const long step = it.in_pitch ? 1 : C;

        for (int c0 = 0; c0 < C; c0 += SM_CH) {
            double acc [SM_CH];
            long at [SM_CH];
#pragma unroll
            for (int u = 0; u < SM_CH; ++u) {
                const int c = min (c0 + u, C - 1);
                acc [u] = 0.0;
                at [u] = it.in_pitch ? (long) c * it.in_pitch + j0 : (long) j0 * C + c;
            }
            for (int t = t_lo; t < t_hi; ++t) {
                const double d = (double) row_hi [t] - (double) row_lo [t];
#pragma unroll
                for (int u = 0; u < SM_CH; ++u) acc [u] = fused (d, (double) it.in [at [u] + t * step], acc [u]);
            }
#pragma unroll
            for (int u = 0; u < SM_CH; ++u) {
                const int c = c0 + u;
                if (c < C) {
                    const double D = (double) it.F * acc [u];
                    const art_s gy = it.gy_pitch ? it.gy [(size_t) c * it.gy_pitch + m] : it.gy [(size_t) m * C + c];
                    s += (double) gy * D;
                }
            }
        }
    }
    it.gp [m] = s;
}

__global__ __launch_bounds__ (ADJ_TILE)
void fir_sample_adjoint_kernel (const ArtSampleItem *items, int count)
{
    __shared__ int s_w [ADJ_CHUNK];                   // window start of each output of the chunk
    __shared__ int s_row [ADJ_CHUNK];                 // its filter row's offset in the bank, in taps
    __shared__ int s_pass [ADJ_CHUNK];                // nearest filter: the tap of the pass-through (-1: an ordinary row)
    __shared__ double s_f0 [ADJ_CHUNK], s_f1 [ADJ_CHUNK];      // 1.0 - frac, frac
    __shared__ art_s s_gy [ADJ_CHUNK * 4];
    __shared__ int s_range [2];                       // first output of the range, one past its last

    const unsigned int task = blockIdx.x;
    const ArtSampleItem &it = items [sample_item_of (items, count, task)];
    const int cg = sample_group (it.C), groups = (it.C + cg - 1) / cg;
    const int local = (int)(task - it.task0), tile = local / groups, ch0 = (local - tile * groups) * cg;

    // (the same branch for the whole workgroup: the item's)
    const SampleCurve curve = { it.pos };
    if (it.interpolate) {
        if (cg == 4) sample_adjoint_tile<4, true> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
        else if (cg == 2) sample_adjoint_tile<2, true> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
        else sample_adjoint_tile<1, true> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
    }
    else {
        if (cg == 4) sample_adjoint_tile<4, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
        else if (cg == 2) sample_adjoint_tile<2, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
        else sample_adjoint_tile<1, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
    }
}

} // namespace

extern "C" {

unsigned long arthip_fir_sample_tasks (const ArtSampleItem *it, int what)
{
    if (what != ART_SAMPLE_ADJOINT) return ((unsigned long) it->gy_frames + SM_TILE - 1) / SM_TILE;
    const int cg = sample_group (it->C);
    return (((unsigned long) it->in_frames + ADJ_TILE - 1) / ADJ_TILE) * (unsigned long)((it->C + cg - 1) / cg);
}

size_t arthip_fir_sample_bytes (int nitems) { return sizeof (ArtSampleItem) * (size_t) nitems; }

int arthip_fir_sample (const ArtSampleItem *items, int n, int what, void *d_table, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    if (n <= 0) return 0;
    const size_t bytes = arthip_fir_sample_bytes (n);
    Staging *sg = staging_take (bytes);
    if (!sg) return -1;

    ArtSampleItem *host = (ArtSampleItem *) sg->host;
    unsigned long next = 0;
    for (int i = 0; i < n; ++i) {
        host [i] = items [i];
        host [i].task0 = (unsigned int) next;
        next += arthip_fir_sample_tasks (&items [i], what);
    }
    if (next > 0x7fffffffUL) { (void) staging_give (sg, st); return -1; }

    if (hipMemcpyAsync (d_table, sg->host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { (void) staging_give (sg, st); return -1; }
    const ArtSampleItem *d_items = (const ArtSampleItem *) d_table;
    const dim3 grid ((unsigned int) next);
    switch (what) {
        case ART_SAMPLE_FORWARD: hipLaunchKernelGGL (fir_sample_kernel, grid, dim3 (SM_TILE), 0, st, d_items, n); break;
        case ART_SAMPLE_ADJOINT: hipLaunchKernelGGL (fir_sample_adjoint_kernel, grid, dim3 (ADJ_TILE), 0, st, d_items, n); break;
        default: hipLaunchKernelGGL (fir_sample_slope_kernel, grid, dim3 (SM_TILE), 0, st, d_items, n); break;
    }
    bool ok = hipGetLastError () == hipSuccess;
    if (staging_give (sg, st)) ok = false;
    return ok ? 1 : -1;
}

} // extern "C"
