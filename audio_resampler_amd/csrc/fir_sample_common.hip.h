#pragma once
// fir_sample_common.hip.h — what the kernels of a position curve share (gfx950): fir_sample.hip's three and fir_band.hip's three use this one
// copy of the position arithmetic, the bisections, the stores and the adjoint's tile.  Compiled with -ffp-contract=off, as both files are.
#include "fir_common.hip.h"
#include "fir_adjoint_walk.hip.h"

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

// adj_walk's position source: what the positions are laid over, and the curve
struct SampleGrid { int N, T, F; };
struct SampleCurve { const double *pos; };

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

// the task's item: the last whose first task is <= task (every item of a launch has a task at least)
template <typename Item>
__device__ __forceinline__ int sample_item_of (const Item *items, int count, unsigned int task)
{
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items [mid].task0 <= task) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <typename Item>
__device__ __forceinline__ void sample_store (const Item &it, int c, unsigned int m, art_s v)
{
    if (it.out_pitch) it.out [(size_t) c * it.out_pitch + m] = v;
    else it.out [(size_t) m * it.C + c] = v;
}

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
template <int CG, bool INTERP, bool BAND = false, typename Item, typename Curve>
__device__ __forceinline__ void sample_adjoint_tile (const Item &it, const Curve &curve, int tile, int ch0, int *s_w, int *s_row, int *s_pass,
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

} // namespace
