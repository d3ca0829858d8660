// fir_sample.hip — whole clips evaluated at a position curve that lies in device memory (gfx950): the kernels of
// resampleSampleClipsPlanarDevice, resampleSampleAdjointClipsPlanarDevice and resampleSamplePositionGradientClipsPlanarDevice, and of their
// banded counterparts resampleSampleBandClipsPlanarDevice, resampleSampleBandAdjointClipsPlanarDevice and
// resampleSampleBandGradientsClipsPlanarDevice.  The 1-D, windowed-sinc counterpart of grid_sample: no planner, no context state, no history —
// the context supplies its bank and flags.  Both families share one item (ArtSampleItem), one launch function, the position arithmetic, the
// bisections, the stores and the adjoint's tile (sample_adjoint_tile over adj_walk, with a compile-time BAND switch).  The two forwards and the
// two slope kernels each keep the body they were measured with: one body for both with the same switch computed the same bits but cost the
// unbanded slope 1 % and the banded two-rung paths 1-2.5 % (profiles/clip_curve_one_body.txt), so the maps are the earlier lines, side by side.
//
// A position p (a double, in input frames) of a clip of N frames: whole = floor (p), fr = (p - whole) * F (neither fused), fi = floor (fr) and
// frac = fr - fi on an interpolating context, fi = floor (fr + 0.5) and frac = 0 on a nearest-filter one; tap t reads input frame
// whole - half + 1 + t — locate ()'s arithmetic with off = p, so that p = 0 is centred on frame 0.  Frames below 0 or at and past N are
// silence: their taps are LEFT OUT, not multiplied by zero.  A position that is not finite, below -(half + 1) or at or past N + half has no
// window at all: the comparison is made on the double, before any conversion to int, and such an output is exactly 0, reads nothing and
// has no term in any gradient.  (p - whole can round up to 1 for a tiny negative p, and fi to F: taken as fi = F - 1, frac = 1 — the
// same value and weight from rows inside the bank, and the slope of the cell p lies in.)
//
// BAND — what a mip chain is to a texture sampler: an item holds K banks of one shape at descending cut-offs (rung 0 the widest) and, beside
// its positions, a curve of levels — doubles in device memory.  An output's level l picks two neighbouring rungs and blends them:
//     !(l > 0) (a NaN, -0.0, a negative): L = 0, lam = 0;   l >= K - 1: L = K - 1, lam = 0;   else L = floor (l), lam = l - L.
// With a_k = s0 (1 - frac) + s1 frac the value of rung k in double (the chains and the lerp before the rounding), y = (art_s) a_L where
// lam == 0 — rung L + 1 is not read — and (art_s)(a_L (1.0 - lam) + a_{L+1} lam) elsewhere; the weights of the adjoint and the slopes blend the
// same way.  An unbanded item is the ladder of one rung with the level never read: on a whole level the banded results are the unbanded
// entries' on that rung's bank bit for bit.
//
// Every launch is one flattened task space over the call; a workgroup finds its item by bisection over the items' first tasks (as
// fir_rate_grad.hip does), so one long clip and a thousand short ones spread over the chip alike.  No atomics, no counters: every value is
// one fixed tree of its own clip's terms whatever the batch, the item's place in it, the layout, the pitches or the stream.
//   fir_sample_kernel, fir_band_kernel
//       a task is a tile of SM_TILE consecutive outputs, a lane one output: its position read coalesced, the samples read from global memory
//       as they lie, per channel the fp64 chains of explicit fused multiply-adds with bank rows fi and fi + 1, t ascending — SM_CH channels'
//       chains in flight together — then the reference's lerp.  The bank (580 KB at the defaults) does not fit the LDS and is served from L2,
//       as in fir_rate_grad_tile_kernel.  BAND: where lam != 0 the two rungs' chains run side by side over one pass of the samples; lanes of
//       a wave may sit on different rungs.  Unbanded only: the nearest filter, and its pass-through.
//   fir_sample_adjoint_kernel, fir_band_adjoint_kernel
//       a task is a tile of ADJ_TILE consecutive INPUT frames and one channel group, a lane one frame j.  PRECONDITION: the item's positions do
//       not decrease (the levels may be anything).  The outputs whose windows hold j are then one range, found by bisection on the position
//       array itself (on the doubles: a position far out of range, or an infinity, sorts where it lies; a NaN counts as +infinity), and walked
//       by adj_walk — fir_adjoint.hip's blocks kernel's walk, the same weights in the same order — with the positions as its source.  BAND:
//       the weight is (art_s)(w_L (1.0 - lam) + w_{L+1} lam), w_k = h0 f0 + h1 f1 unrounded, and rung L's own weight where lam == 0.  On a
//       curve that decreases somewhere the sums are unspecified, and every index still lies in [0, M], every row inside the bank: an output
//       in the range whose position has no window is placed where no frame is.
//   fir_sample_slope_kernel, fir_band_slope_kernel
//       a map: a lane sets gp [m] = sum_c gy [c, m] D [c, m], D = F * (fir_rate_grad_tile_kernel's chain of (bank [fi + 1][t] - bank [fi][t]) x):
//       the slope of the cell floor picks, no average on a boundary.  BAND: D = D_L where lam == 0 and D_L (1.0 - lam) + D_{L+1} lam elsewhere;
//       gl [m] = sum_c gy (a_{j+1} - a_j), j = min (L, K - 2), for 0 <= l <= K - 1 (-0.0 among them: the closed ends pass the gradient, as a
//       clamp's do) and exactly 0 elsewhere, for a NaN, for K = 1 and without a window.  An item asks for either or both; the value chains
//       are run only where gl is asked for.
//
// Compiled with -ffp-contract=off: the only fused operations are the chains' explicit ones.
#include <cstring>
#include "fir_common.hip.h"
#include "fir_adjoint_walk.hip.h"
#include "staging.hip.h"

namespace {

constexpr int SM_TILE = ART_SAMPLE_TILE; // outputs per task of the forward and the slope = their threads
constexpr int SM_CH = 4;                 // channels whose chains are in flight together
static_assert (ADJ_TILE == ART_SAMPLE_TILE, "the adjoint's tasks are counted in tiles of ART_SAMPLE_TILE input frames");

// the window of position p on a clip of N frames (pos.ip: floor (p)); false: none
template <bool INTERP>
__device__ __forceinline__ bool sample_locate (double p, int N, int T, int F, Pos &pos)
{
    const int half = T / 2;
    if (!(p >= -(double)(half + 1) && p < (double) N + (double) half)) return false;      // (a NaN fails the first)
    const double whole = floor (p);

    double fr = p - whole;
    fr = fr * (double) F;

    if (INTERP) {
        pos.fi = (int) floor (fr);
        pos.frac = fr - (double) pos.fi;
        if (pos.fi >= F) { pos.fi = F - 1; pos.frac = 1.0; }
    }
    else {
        pos.fi = (int) floor (fr + 0.5);
        pos.frac = 0.0;
    }

    pos.ip = (int) whole;
    return true;
}

// the rung and the blend of level l on a ladder of K rungs
__device__ __forceinline__ void band_level (double l, int K, int &L, double &lam)
{
    if (!(l > 0.0)) { L = 0; lam = 0.0; }
    else if (l >= (double)(K - 1)) { L = K - 1; lam = 0.0; }
    else {
        const double whole = floor (l);
        L = (int) whole;
        lam = l - whole;
    }
}

// adj_walk's position source: what the positions are laid over, and the curve — of a banded item with the levels beside it
struct SampleGrid { int N, T, F; };
struct SampleCurve { const double *pos; };
struct BandCurve : SampleCurve { const double *level; int K; };

template <bool INTERP>
__device__ __forceinline__ Pos adj_locate (const SampleGrid &g, const SampleCurve &c, unsigned int n)
{
    Pos pos;
    if (!sample_locate<INTERP> (c.pos [n], g.N, g.T, g.F, pos)) {
        pos.ip = g.T / 2 - 1 - g.T;                            // (the window starts at frame -T: it holds no frame of the clip)
        pos.fi = 0; pos.frac = 0.0;
    }
    return pos;
}

__device__ __forceinline__ void adj_level (const BandCurve &c, unsigned int n, int &rung, double &lam) { band_level (c.level [n], c.K, rung, lam); }

// the task's item: the last whose first task is <= task (every item of a launch has a task at least)
__device__ __forceinline__ int sample_item_of (const ArtSampleItem *items, int count, unsigned int task)
{
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items [mid].task0 <= task) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ void sample_store (const ArtSampleItem &it, int c, unsigned int m, art_s v)
{
    if (it.out_pitch) it.out [(size_t) c * it.out_pitch + m] = v;
    else it.out [(size_t) m * it.C + c] = v;
}

// ---- the unbanded maps ----

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
    const art_s *const row_lo = it.bank [0] + (size_t) pos.fi * T, *const row_hi = row_lo + (INTERP ? T : 0);
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
        const art_s *const row_lo = it.bank [0] + (size_t) pos.fi * T, *const row_hi = row_lo + T;
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

// ---- the banded maps ----

// The chains of R rungs over one pass of a channel group's samples: per rung r (row [r]: its row fi) and channel u, t ascending,
// VAL: s0 and s1, fir_sample_kernel's chains with rows fi and fi + 1;  SLOPE: d, fir_sample_slope_kernel's chain of their difference.
template <int R, bool VAL, bool SLOPE>
__device__ __forceinline__ void band_chains (const art_s *const (&row) [R], int T, const art_s *in, const long (&at) [SM_CH], long step, int t_lo, int t_hi,
                                             double (&s0) [R][SM_CH], double (&s1) [R][SM_CH], double (&d) [R][SM_CH])
{
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int u = 0; u < SM_CH; ++u) { s0 [r][u] = 0.0; s1 [r][u] = 0.0; d [r][u] = 0.0; }

    for (int t = t_lo; t < t_hi; ++t) {
        double b0 [R], b1 [R], db [R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            b0 [r] = (double) row [r][t]; b1 [r] = (double) row [r][T + t];
            db [r] = b1 [r] - b0 [r];
        }
#pragma unroll
        for (int u = 0; u < SM_CH; ++u) {
            const double v = (double) in [at [u] + t * step];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (VAL) { s0 [r][u] = fused (b0 [r], v, s0 [r][u]); s1 [r][u] = fused (b1 [r], v, s1 [r][u]); }
                if (SLOPE) d [r][u] = fused (db [r], v, d [r][u]);
            }
        }
    }
}

// a rung's value before its rounding: the sampler's lerp
__device__ __forceinline__ double band_lerp (double s0, double s1, double frac)
{
    const double left = s0 * (1.0 - frac), right = s1 * frac;
    return left + right;
}

__device__ __forceinline__ double band_blend (double lo, double hi, double lam)
{
    const double lower = lo * (1.0 - lam), upper = hi * lam;
    return lower + upper;
}

// a channel group's addresses of tap 0 (a chain past the last channel repeats it, and is dropped)
__device__ __forceinline__ void band_group (const ArtSampleItem &it, int c0, int j0, long (&at) [SM_CH])
{
#pragma unroll
    for (int u = 0; u < SM_CH; ++u) {
        const int c = min (c0 + u, it.C - 1);
        at [u] = it.in_pitch ? (long) c * it.in_pitch + j0 : (long) j0 * it.C + c;
    }
}

__global__ __launch_bounds__ (SM_TILE)
void fir_band_kernel (const ArtSampleItem *items, int count)
{
    const unsigned int task = blockIdx.x;
    const ArtSampleItem &it = items [sample_item_of (items, count, task)];
    const unsigned int m = (task - it.task0) * SM_TILE + threadIdx.x;
    if (m >= it.gy_frames) return;

    const int T = it.T, half = T / 2, N = it.in_frames, C = it.C;
    Pos pos;
    if (!sample_locate<true> (it.pos [m], N, T, it.F, pos)) {
        for (int c = 0; c < C; ++c) sample_store (it, c, m, (art_s) 0);
        return;
    }
    int L; double lam;
    band_level (it.level [m], it.rungs, L, lam);

    const int j0 = pos.ip - half + 1;                          // input frame of tap 0; the taps that read a frame of the clip are [t_lo, t_hi)
    const int t_lo = max (0, -j0), t_hi = min (T, N - j0);
    const size_t row = (size_t) pos.fi * T;
    const long step = it.in_pitch ? 1 : C;

    for (int c0 = 0; c0 < C; c0 += SM_CH) {
        long at [SM_CH];
        band_group (it, c0, j0, at);
        if (lam == 0.0) {
            const art_s *const rows [1] = { it.bank [L] + row };
            double s0 [1][SM_CH], s1 [1][SM_CH], d [1][SM_CH];
            band_chains<1, true, false> (rows, T, it.in, at, step, t_lo, t_hi, s0, s1, d);
#pragma unroll
            for (int u = 0; u < SM_CH; ++u)
                if (c0 + u < C) sample_store (it, c0 + u, m, (art_s) band_lerp (s0 [0][u], s1 [0][u], pos.frac));
        }
        else {
            const art_s *const rows [2] = { it.bank [L] + row, it.bank [L + 1] + row };
            double s0 [2][SM_CH], s1 [2][SM_CH], d [2][SM_CH];
            band_chains<2, true, false> (rows, T, it.in, at, step, t_lo, t_hi, s0, s1, d);
#pragma unroll
            for (int u = 0; u < SM_CH; ++u)
                if (c0 + u < C) {
                    const double lo = band_lerp (s0 [0][u], s1 [0][u], pos.frac), hi = band_lerp (s0 [1][u], s1 [1][u], pos.frac);
                    sample_store (it, c0 + u, m, (art_s) band_blend (lo, hi, lam));
                }
        }
    }
}

__device__ __forceinline__ double band_gy (const ArtSampleItem &it, int c, unsigned int m)
{
    return (double)(it.gy_pitch ? it.gy [(size_t) c * it.gy_pitch + m] : it.gy [(size_t) m * it.C + c]);
}

// one output of the gradients: WANT_P: gp, WANT_L: gl (one of them at least)
template <bool WANT_P, bool WANT_L>
__device__ __forceinline__ void band_gradients (const ArtSampleItem &it, unsigned int m)
{
    const int T = it.T, half = T / 2, N = it.in_frames, C = it.C, K = it.rungs;
    Pos pos;
    double gp = 0.0, gl = 0.0;
    if (sample_locate<true> (it.pos [m], N, T, it.F, pos)) {
        const double l = it.level [m];
        int L; double lam;
        band_level (l, K, L, lam);
        const bool moves = WANT_L && K >= 2 && l >= 0.0 && l <= (double)(K - 1);      // (a NaN fails both; -0.0 passes)

        const int j0 = pos.ip - half + 1;
        const int t_lo = max (0, -j0), t_hi = min (T, N - j0);
        const size_t row = (size_t) pos.fi * T;
        const long step = it.in_pitch ? 1 : C;
        const double F = (double) it.F;

        for (int c0 = 0; c0 < C; c0 += SM_CH) {
            long at [SM_CH];
            band_group (it, c0, j0, at);
            if (moves) {
                // rungs j and j + 1: the level's cell, whose two values gl needs; rung L, and L + 1 where lam != 0, are among them
                const int j = min (L, K - 2);
                const art_s *const rows [2] = { it.bank [j] + row, it.bank [j + 1] + row };
                double s0 [2][SM_CH], s1 [2][SM_CH], d [2][SM_CH];
                band_chains<2, true, WANT_P> (rows, T, it.in, at, step, t_lo, t_hi, s0, s1, d);
#pragma unroll
                for (int u = 0; u < SM_CH; ++u)
                    if (c0 + u < C) {
                        const double gy = band_gy (it, c0 + u, m);
                        const double lo = band_lerp (s0 [0][u], s1 [0][u], pos.frac), hi = band_lerp (s0 [1][u], s1 [1][u], pos.frac);
                        gl += gy * (hi - lo);
                        if (WANT_P) {
                            const double D0 = F * d [0][u], D1 = F * d [1][u];
                            const double D = lam != 0.0 ? band_blend (D0, D1, lam) : L > j ? D1 : D0;
                            gp += gy * D;
                        }
                    }
            }
            else if (WANT_P) {
                if (lam == 0.0) {
                    const art_s *const rows [1] = { it.bank [L] + row };
                    double s0 [1][SM_CH], s1 [1][SM_CH], d [1][SM_CH];
                    band_chains<1, false, true> (rows, T, it.in, at, step, t_lo, t_hi, s0, s1, d);
#pragma unroll
                    for (int u = 0; u < SM_CH; ++u)
                        if (c0 + u < C) {
                            const double D = F * d [0][u];
                            gp += band_gy (it, c0 + u, m) * D;
                        }
                }
                else {
                    const art_s *const rows [2] = { it.bank [L] + row, it.bank [L + 1] + row };
                    double s0 [2][SM_CH], s1 [2][SM_CH], d [2][SM_CH];
                    band_chains<2, false, true> (rows, T, it.in, at, step, t_lo, t_hi, s0, s1, d);
#pragma unroll
                    for (int u = 0; u < SM_CH; ++u)
                        if (c0 + u < C) {
                            const double D0 = F * d [0][u], D1 = F * d [1][u];
                            gp += band_gy (it, c0 + u, m) * band_blend (D0, D1, lam);
                        }
                }
            }
        }
    }
    if (WANT_P) it.gp [m] = gp;
    if (WANT_L) it.gl [m] = gl;
}

__global__ __launch_bounds__ (SM_TILE)
void fir_band_slope_kernel (const ArtSampleItem *items, int count)
{
    const unsigned int task = blockIdx.x;
    const ArtSampleItem &it = items [sample_item_of (items, count, task)];
    const unsigned int m = (task - it.task0) * SM_TILE + threadIdx.x;
    if (m >= it.gy_frames) return;
    // (the same branch for the whole launch: the entry's lists)
    if (it.gp && it.gl) band_gradients<true, true> (it, m);
    else if (it.gp) band_gradients<true, false> (it, m);
    else band_gradients<false, true> (it, m);
}

// ---- the adjoints ----

// first m in [0, count) whose position is not below `bound` (count: none); a NaN is not below anything
__device__ inline int sample_first_not_below (const double *pos, unsigned int count, double bound)
{
    unsigned int lo = 0, hi = count;
    while (lo < hi) {
        const unsigned int mid = lo + (hi - lo) / 2;
        if (!(pos [mid] < bound)) hi = mid; else lo = mid + 1;
    }
    return (int) lo;
}

// channels per group of an item's adjoint tasks
__host__ __device__ inline int sample_group (int C) { return C > 2 ? 4 : C == 2 ? 2 : 1; }

// One adjoint task: the tile's ADJ_TILE input frames of one channel group, a lane one frame j; `curve` is adj_walk's position source (its
// .pos the item's positions).  BAND: the walk blends two rungs of the item's ladder per output (s_rung, s_lam: its two more LDS rows).
template <int CG, bool INTERP, bool BAND, typename Curve>
__device__ __forceinline__ void sample_adjoint_tile (const ArtSampleItem &it, const Curve &curve, int tile, int ch0, int *s_w, int *s_row, int *s_pass,
                                                     double *s_f0, double *s_f1, art_s *s_gy, int *s_range, int *s_rung = nullptr, double *s_lam = nullptr)
{
    const int tid = threadIdx.x;
    const int T = it.T, half = T / 2, N = it.in_frames;
    const int j0 = tile * ADJ_TILE;
    const int j1 = min (j0 + ADJ_TILE, N);             // (j0 < N: the item has ceil (N / ADJ_TILE) tiles)
    const int j = j0 + tid;

    // windows [w, w + T - 1], w = floor (p) - half + 1, that meet the tile's frames [j0, j1 - 1]: floor (p) >= j0 - T + half up to
    // floor (p) <= j1 - 1 + half - 1, which on the doubles is p >= j0 - T + half up to p < j1 + half - 1
    if (tid < 2) s_range [tid] = sample_first_not_below (it.pos, it.gy_frames, tid ? (double)(j1 + half - 1) : (double)(j0 - T + half));
    __syncthreads ();

    art_s acc [CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) acc [c] = 0;

    const SampleGrid grid = { N, T, it.F };
    adj_walk<CG, INTERP, BAND> (acc, it, grid, curve, ch0, tid, j, j < N, 0u, s_range [0], s_range [1], s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_rung, s_lam);

    if (j < N)
#pragma unroll
        for (int c = 0; c < CG; ++c)
            if (ch0 + c < it.C) {
                if (it.out_pitch) it.out [(size_t)(ch0 + c) * it.out_pitch + j] = acc [c];
                else it.out [(size_t) j * it.C + ch0 + c] = acc [c];
            }
}

// the item of an adjoint's task, its tile and the first channel of its group
__device__ __forceinline__ const ArtSampleItem &sample_adjoint_task (const ArtSampleItem *items, int count, int &cg, int &tile, int &ch0)
{
    const unsigned int task = blockIdx.x;
    const ArtSampleItem &it = items [sample_item_of (items, count, task)];
    cg = sample_group (it.C);
    const int groups = (it.C + cg - 1) / cg, local = (int)(task - it.task0);
    tile = local / groups; ch0 = (local - tile * groups) * cg;
    return it;
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

    int cg, tile, ch0;
    const ArtSampleItem &it = sample_adjoint_task (items, count, cg, tile, ch0);

    // (the same branch for the whole workgroup: the item's)
    const SampleCurve curve = { it.pos };
    if (it.interpolate) {
        if (cg == 4) sample_adjoint_tile<4, true, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
        else if (cg == 2) sample_adjoint_tile<2, true, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
        else sample_adjoint_tile<1, true, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
    }
    else {
        if (cg == 4) sample_adjoint_tile<4, false, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
        else if (cg == 2) sample_adjoint_tile<2, false, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
        else sample_adjoint_tile<1, false, false> (it, curve, tile, ch0, s_w, s_row, s_pass, s_f0, s_f1, s_gy, s_range);
    }
}

__global__ __launch_bounds__ (ADJ_TILE)
void fir_band_adjoint_kernel (const ArtSampleItem *items, int count)
{
    __shared__ int s_w [ADJ_CHUNK];                   // window start of each output of the chunk
    __shared__ int s_row [ADJ_CHUNK];                 // its filter row's offset in a bank, in taps
    __shared__ int s_rung [ADJ_CHUNK];                // its rung L
    __shared__ double s_f0 [ADJ_CHUNK], s_f1 [ADJ_CHUNK];      // 1.0 - frac, frac
    __shared__ double s_lam [ADJ_CHUNK];              // its blend with rung L + 1 (0: that rung is not read)
    __shared__ art_s s_gy [ADJ_CHUNK * 4];
    __shared__ int s_range [2];                       // first output of the range, one past its last

    int cg, tile, ch0;
    const ArtSampleItem &it = sample_adjoint_task (items, count, cg, tile, ch0);
    BandCurve curve;
    curve.pos = it.pos; curve.level = it.level; curve.K = it.rungs;

    // (the same branch for the whole workgroup: the item's)
    if (cg == 4) sample_adjoint_tile<4, true, true> (it, curve, tile, ch0, s_w, s_row, nullptr, s_f0, s_f1, s_gy, s_range, s_rung, s_lam);
    else if (cg == 2) sample_adjoint_tile<2, true, true> (it, curve, tile, ch0, s_w, s_row, nullptr, s_f0, s_f1, s_gy, s_range, s_rung, s_lam);
    else sample_adjoint_tile<1, true, true> (it, curve, tile, ch0, s_w, s_row, nullptr, s_f0, s_f1, s_gy, s_range, s_rung, s_lam);
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

int arthip_fir_sample (const ArtSampleItem *items, int n, int what, int band, void *d_table, void *stream)
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
    void (*const kernels [3][2]) (const ArtSampleItem *, int) = {          // [ART_SAMPLE_*][band]; SM_TILE = ADJ_TILE threads each
        { fir_sample_kernel, fir_band_kernel }, { fir_sample_adjoint_kernel, fir_band_adjoint_kernel }, { fir_sample_slope_kernel, fir_band_slope_kernel } };
    const int which = what == ART_SAMPLE_FORWARD ? 0 : what == ART_SAMPLE_ADJOINT ? 1 : 2;
    hipLaunchKernelGGL (kernels [which][band != 0], dim3 ((unsigned int) next), dim3 (SM_TILE), 0, st, d_items, n);
    bool ok = hipGetLastError () == hipSuccess;
    if (staging_give (sg, st)) ok = false;
    return ok ? 1 : -1;
}

} // extern "C"
