// fir_rate_grad.hip — the gradient of a clip made block by block with respect to its blocks' RATIOS (gfx950):
// resampleRateGradientScheduleClipsPlanarDevice's two kernels.
//
// On an interpolating context output n of phase k (the blocks' process calls in turn, then the flush) sits at p = o_k + n / rho_k and is
// the lerp of the dot products with bank rows fi and fi + 1, fi = floor (frac (p) F): piecewise linear in p with the slope
// D = F sum_t (bank [fi + 1][t] - bank [fi][t]) x [ip + t] of the cell the forward's own locate () picked (on a filter boundary: that
// cell's, no average).  With the output counts n_k held fixed, o_{k+1} = o_k + n_k / rho_k, so per phase
//     S0_k = sum gy D,   S1_k = sum n gy D   (over the channels and the phase's outputs)
//     dL/d rho_k = -(S1_k + n_k sum_{m > k} S0_m) / rho_k^2
// and a block's gradient is its phase's; the last block's is its own plus the flush's, which runs at its ratio.
//
// First launch: a task is a tile of ART_RATE_TILE consecutive outputs of one phase of one clip, in one flattened space over the call; a
// workgroup finds its phase (and through it its clip) by bisection over the phases' first tasks, so one long clip and a thousand short
// ones both spread over the chip, and a phase without outputs has no task.  A lane owns one output: its position by locate (), the taps
// the phase may read as one range of t (input frame j at linear index H + j - start; nothing at or past `end`, below `floor` or before
// the clip: such taps are LEFT OUT, not multiplied by zero), then per channel one fp64 chain of explicit fused multiply-adds, t
// ascending — RG_CH channels' chains in flight together — D = F * chain, v = gy * D, and the lane's pair (sum_ch v, n * sum_ch v), the
// channels in order.  Outputs at or past gy_frames have no terms and their gy is not read.  The samples are read from global memory as
// they lie (consecutive lanes read overlapping windows 1 / ratio frames apart: the caches' work), so the LDS holds the reduction's eight
// doubles and nothing that depends on the ratio, the block count or the clip.  The pairs are folded by a butterfly over the wave and the
// four waves added in wave order (lag_products.hip's tree); the tile's pair goes to scratch.
// Second launch: one wave per clip, 64 phases at a time from the last phase to the first.  A lane adds its phase's tile pairs in ascending
// tile order; the S0 of the phases behind are added one by one from the last phase down (every lane replays that one sequence up to its
// own phase), and the lane forms 0 - (S1 + n * behind) / (rho * rho).  The flush's is added to the last block's, in that order, and the
// clip's numBlocks doubles are SET.  No atomics, no counters: the launch boundary is the only hand-off, and every sum is one fixed tree
// of the clip's own terms whatever the batch, the clip's place in it, the layout, the pitch or the stream.
//
// Compiled with -ffp-contract=off: the only fused operation is the chains' explicit one.
#include <cstring>
#include "fir_common.hip.h"
#include "staging.hip.h"

namespace {

constexpr int RG_TILE = ART_RATE_TILE;   // outputs per task = the first launch's threads
constexpr int RG_WAVES = RG_TILE / 64;
constexpr int RG_CH = 4;                 // channels whose chains are in flight together
constexpr int RG_FINISH = 64;            // the second launch: one wave per clip, this many phases per trip

// per phase of the call's phase table: its first task, and the item it belongs to
struct RatePhaseTask { unsigned int task0; int item; };

__global__ __launch_bounds__ (RG_TILE)
void fir_rate_grad_tile_kernel (const ArtRateItem *items, const ArtAdjPhase *phases, const RatePhaseTask *tasks, int nphases,
                                const double *seg_base, const unsigned int *seg_first, const int *seg_lin_base, double *partials)
{
    __shared__ double red [RG_WAVES][2];

    const int tid = threadIdx.x;
    const unsigned int task = blockIdx.x;

    // the task's phase: the last whose first task is <= task (a phase without outputs shares its first task with the next one, which wins)
    int lo = 0, hi = nphases - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tasks [mid].task0 <= task) lo = mid; else hi = mid - 1;
    }
    const ArtAdjPhase &P = phases [lo];
    const ArtRateItem &it = items [tasks [lo].item];
    const unsigned int n = (task - tasks [lo].task0) * RG_TILE + (unsigned int) tid;
    const unsigned int g = P.first_output + n;                 // the output among the clip's

    double s = 0.0;
    if (n < P.outputs && g < it.gy_frames) {
        const int T = it.T, half = T / 2, H = T + half, C = it.C;
        const AdjRate rate = { P.ratio, it.F };
        const AdjSegs segs = { P.seg_count, seg_first + P.seg_first, seg_lin_base + P.seg_first, seg_base + P.seg_first };
        const Pos pos = locate<true> (rate, segs, n);
        const int w = pos.ip - half + 1;                       // linear index of tap 0
        // tap t reads linear index w + t = input frame w + t - off; the taps the phase may read are [t_lo, t_hi)
        const int off = H - P.start;
        const int t_lo = max (0, max (P.floor, off) - w);
        const int t_hi = min (T, (min (P.end, it.in_frames) - P.start) + H - w);
        const art_s *const row_lo = it.bank + (size_t) pos.fi * T, *const row_hi = row_lo + T;
        const long j0 = (long) w - off;                        // input frame of tap 0
        const long step = it.x_pitch ? 1 : C;

        for (int c0 = 0; c0 < C; c0 += RG_CH) {
            double acc [RG_CH];
            long at [RG_CH];
#pragma unroll
            for (int u = 0; u < RG_CH; ++u) {                  // (a chain past the last channel repeats it, and is dropped)
                const int c = min (c0 + u, C - 1);
                acc [u] = 0.0;
                at [u] = it.x_pitch ? (long) c * it.x_pitch + j0 : j0 * C + c;
            }
            for (int t = t_lo; t < t_hi; ++t) {
                const double d = (double) row_hi [t] - (double) row_lo [t];
#pragma unroll
                for (int u = 0; u < RG_CH; ++u) acc [u] = fused (d, (double) it.x [at [u] + t * step], acc [u]);
            }
#pragma unroll
            for (int u = 0; u < RG_CH; ++u) {
                const int c = c0 + u;
                if (c < C) {
                    const double D = (double) it.F * acc [u];
                    const art_s gy = it.gy_pitch ? it.gy [(size_t) c * it.gy_pitch + g] : it.gy [(size_t) g * C + c];
                    s += (double) gy * D;
                }
            }
        }
    }

    // the tile's tree: a butterfly over the wave's lanes (every lane ends with the same bits), then the waves in order
    double s0 = s, s1 = (double) n * s;
#pragma unroll
    for (int o = 32; o; o >>= 1) { s0 += __shfl_xor (s0, o, 64); s1 += __shfl_xor (s1, o, 64); }
    if (!(tid & 63)) { red [tid >> 6][0] = s0; red [tid >> 6][1] = s1; }
    __syncthreads ();
    if (tid < 2) {
        double r = red [0][tid];
#pragma unroll
        for (int wv = 1; wv < RG_WAVES; ++wv) r += red [wv][tid];
        partials [(size_t) task * 2 + tid] = r;
    }
}

__global__ __launch_bounds__ (RG_FINISH)
void fir_rate_grad_finish_kernel (const ArtRateItem *items, const ArtAdjPhase *phases, const RatePhaseTask *tasks, const double *partials)
{
    __shared__ double s_s0 [RG_FINISH], s_g [RG_FINISH];

    const int lane = threadIdx.x;
    const ArtRateItem &it = items [blockIdx.x];
    const int np = it.phase_count, K = np - 1;                 // (K >= 1 blocks; phase K is the flush)
    double behind = 0.0;                                       // S0 of the phases behind this trip's, added from the last phase down

    for (int top = np - 1; top >= 0; top -= RG_FINISH) {
        const int p = top - lane;                              // lane 0 has the trip's last phase
        double S0 = 0.0, S1 = 0.0, rho = 1.0, count = 0.0;
        if (p >= 0) {
            const ArtAdjPhase &P = phases [it.phase_first + p];
            const unsigned int tiles = (P.outputs + RG_TILE - 1) / RG_TILE;
            const double *const q = partials + (size_t) tasks [it.phase_first + p].task0 * 2;
            for (unsigned int i = 0; i < tiles; ++i) { S0 += q [2 * (size_t) i]; S1 += q [2 * (size_t) i + 1]; }
            rho = P.ratio; count = (double) P.outputs;
        }
        __syncthreads ();                                      // (the trip before is done with both tables)
        s_s0 [lane] = S0;
        __syncthreads ();
        double c = behind;
        for (int q = 0; q < lane; ++q) c += s_s0 [q];
        double gr = 0.0 - (S1 + count * c) / (rho * rho);
        s_g [lane] = gr;
        __syncthreads ();
        if (p >= 0 && p < K) {
            if (p == K - 1) gr = gr + s_g [lane - 1];          // (the first trip's lane 1: the last block, and the flush at its ratio)
            it.grad [p] = gr;
        }
        behind = __shfl (c + S0, RG_FINISH - 1, 64);
    }
}

inline size_t rg_items_bytes (int n) { return (sizeof (ArtRateItem) * (size_t) n + 7) & ~(size_t) 7; }
static_assert (sizeof (ArtAdjPhase) % 8 == 0 && sizeof (RatePhaseTask) == 8, "the segments' doubles follow the phases and their tasks");

// the table: the items, the phases, their first tasks, then the segments as three arrays (doubles first); rounded up to the partials' alignment
inline size_t rg_table_bytes (int nitems, int nphases, int nsegs)
{
    const size_t bytes = rg_items_bytes (nitems) + (sizeof (ArtAdjPhase) + sizeof (RatePhaseTask)) * (size_t) nphases +
                         (sizeof (double) + sizeof (unsigned int) + sizeof (int)) * (size_t) nsegs;
    return (bytes + 7) & ~(size_t) 7;
}

} // namespace

extern "C" {

unsigned long arthip_fir_rate_grad_tiles (const ArtAdjPhase *phases, int nphases)
{
    unsigned long tiles = 0;
    for (int p = 0; p < nphases; ++p) tiles += ((unsigned long) phases [p].outputs + RG_TILE - 1) / RG_TILE;
    return tiles;
}

size_t arthip_fir_rate_grad_bytes (int nitems, int nphases, int nsegs, unsigned long tiles)
{
    return rg_table_bytes (nitems, nphases, nsegs) + sizeof (double) * 2 * (size_t) tiles;
}

int arthip_fir_rate_grad (const ArtRateItem *items, int n, const ArtAdjPhase *phases, int nphases, const ArtamdSegment *segs, int nsegs,
                          void *d_table, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    if (n <= 0) return 0;
    const unsigned long tiles = arthip_fir_rate_grad_tiles (phases, nphases);
    if (tiles > 0x7fffffffUL) return -1;
    const size_t bytes = rg_table_bytes (n, nphases, nsegs), at_phases = rg_items_bytes (n), at_tasks = at_phases + sizeof (ArtAdjPhase) * (size_t) nphases,
                 at_segs = at_tasks + sizeof (RatePhaseTask) * (size_t) nphases;
    Staging *sg = staging_take (bytes);
    if (!sg) return -1;

    memcpy (sg->host, items, sizeof (ArtRateItem) * (size_t) n);
    memcpy ((char *) sg->host + at_phases, phases, sizeof (ArtAdjPhase) * (size_t) nphases);
    RatePhaseTask *tasks = (RatePhaseTask *)((char *) sg->host + at_tasks);
    unsigned int next = 0;
    for (int i = 0; i < n; ++i)                                // (the items' phases lie one after the other, in the items' order)
        for (int p = items [i].phase_first; p < items [i].phase_first + items [i].phase_count; ++p) {
            tasks [p].task0 = next; tasks [p].item = i;
            next += (phases [p].outputs + RG_TILE - 1) / RG_TILE;
        }
    double *base = (double *)((char *) sg->host + at_segs);
    unsigned int *first = (unsigned int *)(base + nsegs);
    int *lin_base = (int *)(first + nsegs);
    for (int q = 0; q < nsegs; ++q) { base [q] = segs [q].base_offset; first [q] = segs [q].first_output; lin_base [q] = segs [q].lin_base; }

    if (hipMemcpyAsync (d_table, sg->host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { (void) staging_give (sg, st); return -1; }
    const ArtRateItem *d_items = (const ArtRateItem *) d_table;
    const ArtAdjPhase *d_phases = (const ArtAdjPhase *)((const char *) d_table + at_phases);
    const RatePhaseTask *d_tasks = (const RatePhaseTask *)((const char *) d_table + at_tasks);
    const double *d_base = (const double *)((const char *) d_table + at_segs);
    const unsigned int *d_first = (const unsigned int *)(d_base + nsegs);
    const int *d_lin_base = (const int *)(d_first + nsegs);
    double *d_part = (double *)((char *) d_table + bytes);

    int launches = 0;
    bool ok = true;
    if (next) {
        hipLaunchKernelGGL (fir_rate_grad_tile_kernel, dim3 (next), dim3 (RG_TILE), 0, st, d_items, d_phases, d_tasks, nphases, d_base, d_first, d_lin_base, d_part);
        ok = hipGetLastError () == hipSuccess;
        if (ok) ++launches;
    }
    if (ok) {
        hipLaunchKernelGGL (fir_rate_grad_finish_kernel, dim3 ((unsigned int) n), dim3 (RG_FINISH), 0, st, d_items, d_phases, d_tasks, (const double *) d_part);
        ok = hipGetLastError () == hipSuccess;
        if (ok) ++launches;
    }
    if (staging_give (sg, st)) ok = false;
    return ok ? launches : -1;
}

} // extern "C"
