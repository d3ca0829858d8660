// fir_adjoint.hip — the transpose of the whole-clip windowed-sinc interpolator (gfx950): resampleAdjointClipsPlanarDevice's kernel, and
// resampleAdjointScheduleClipsPlanarDevice's for clips made block by block (fir_adjoint_blocks_kernel, further down).
//
// The forward kernels gather input taps for an output; this one gathers output gradients for an input, with the same coefficients
// read across the rows of the bank.  A workgroup owns ADJ_TILE consecutive INPUT frames of one clip and one channel group, a lane one
// frame j.  The outputs whose windows touch the tile are one contiguous range per phase (the process call's outputs, then the
// flush's: ip (n) is monotone), found by bisection over n with the forward's own locate (), so the range cannot disagree with the
// positions the sums use.  The range is walked in chunks of ADJ_CHUNK outputs through the LDS — each output's position once, then
// gy for the channel group — so the LDS does not depend on the ratio or the tap count.  For one output consecutive lanes read
// consecutive taps of one bank row (coalesced); its position and gy are the same address for every lane (LDS broadcasts).
// Every lane adds its terms in ascending output order, one fused multiply-add each: gx [j] does not depend on the tile, the chunk,
// the batch or the layout.  No atomics.
//
// Compiled with -ffp-contract=off: the weight's fp64 lerp rounds where the strict forward's does; the only fused operation is the
// accumulation's explicit one.
#include <cstring>
#include "fir_common.hip.h"
#include "fir_adjoint_walk.hip.h"        // ADJ_TILE, ADJ_CHUNK, ADJ_UNROLL and adj_walk: the blocks kernel's walk, shared with fir_sample.hip
#include "staging.hip.h"

namespace {

// window start of output n (linear index of its first tap)
template <bool INTERP>
__device__ __forceinline__ int adj_window (const AdjRate &r, const AdjSegs &s, unsigned int n, int half)
{
    return locate<INTERP> (r, s, n).ip - half + 1;
}

// first n in [0, count) whose window start exceeds `bound` (count: none)
template <bool INTERP>
__device__ int adj_first_above (const AdjRate &r, const AdjSegs &s, unsigned int count, int half, int bound)
{
    unsigned int lo = 0, hi = count;
    while (lo < hi) {
        const unsigned int mid = lo + (hi - lo) / 2;
        if (adj_window<INTERP> (r, s, mid, half) > bound) hi = mid; else lo = mid + 1;
    }
    return (int) lo;
}

template <int CG, bool INTERP>
__global__ __launch_bounds__ (ADJ_TILE)
void fir_adjoint_kernel (const ArtAdjItem *items, int count, const double *seg_base, const unsigned int *seg_first, const int *seg_lin_base)
{
    __shared__ int s_w [ADJ_CHUNK];                   // window start of each output of the chunk
    __shared__ int s_row [ADJ_CHUNK];                 // its filter row's offset in the bank, in taps
    __shared__ int s_pass [ADJ_CHUNK];                // nearest filter: the tap of the pass-through (-1: an ordinary row)
    __shared__ double s_f0 [INTERP ? ADJ_CHUNK : 1], s_f1 [INTERP ? ADJ_CHUNK : 1];      // 1.0 - frac, frac
    __shared__ art_s s_gy [ADJ_CHUNK * CG];
    __shared__ int s_range [2][2];                    // per phase: first output of the range, one past its last

    const int tid = threadIdx.x;

    // the tile's item: the last whose first tile is <= blockIdx.x (every item has a tile at least)
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items [mid].tile0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ArtAdjItem &it = items [lo];
    const int ch0 = (int) blockIdx.y * CG;
    if (ch0 >= it.C) return;

    const art_s *const bank = it.bank;
    const int T = it.T, half = T / 2, H = T + half, nin = it.in_frames;
    const int j0 = (int)(blockIdx.x - it.tile0) * ADJ_TILE;
    const int j1 = min (j0 + ADJ_TILE, nin);           // (j0 < nin: the item has ceil (nin / ADJ_TILE) tiles)
    const int j = j0 + tid;
    const AdjRate rate = { it.ratio, it.F };

    // input frame j in the linear space of each phase; the flush sees the rolled history, nothing below its floor (or below 0)
    const int off [2] = { H, H - nin };
    const int floor1 = max (0, it.lin_floor);

    if (tid < 4) {
        const int p = tid >> 1;
        const AdjSegs segs = { it.seg_count [p], seg_first + it.seg_first [p], seg_lin_base + it.seg_first [p], seg_base + it.seg_first [p] };
        // windows [w, w + T - 1] that meet the tile's frames [j0 + off, j1 - 1 + off]: w > j0 + off - T  up to  w <= j1 - 1 + off
        const int bound = (tid & 1) ? j1 - 1 + off [p] : j0 + off [p] - T;
        s_range [p][tid & 1] = adj_first_above<INTERP> (rate, segs, it.outputs [p], half, bound);
    }
    __syncthreads ();

    art_s acc [CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) acc [c] = 0;

    for (int p = 0; p < 2; ++p) {
        const AdjSegs segs = { it.seg_count [p], seg_first + it.seg_first [p], seg_lin_base + it.seg_first [p], seg_base + it.seg_first [p] };
        const int lin = j + off [p];
        const bool live = j < nin && (p == 0 || lin >= floor1);
        const unsigned int g0 = p ? it.outputs [0] : 0u;           // the phase's first output among the clip's
        const int n_end = s_range [p][1];

        for (int n0 = s_range [p][0]; n0 < n_end; n0 += ADJ_CHUNK) {
            const int cnt = min (ADJ_CHUNK, n_end - n0);
            __syncthreads ();                          // (the chunk before is done with)
            if (tid < cnt) {
                const Pos pos = locate<INTERP> (rate, segs, (unsigned int)(n0 + tid));
                s_w [tid] = pos.ip - half + 1;
                s_row [tid] = pos.fi * T;
                if (INTERP) { s_f0 [tid] = 1.0 - pos.frac; s_f1 [tid] = pos.frac; }
                else s_pass [tid] = (!it.lowpass && (pos.fi % it.F) == 0) ? half - 1 + pos.fi / it.F : -1;
            }
            // gy of the chunk for the channel group: zero past the frames handed in, past the item's channels and — the loop below takes whole
            // groups of ADJ_UNROLL outputs — past the chunk's last output up to the end of its group
            const int cntu = (cnt + ADJ_UNROLL - 1) / ADJ_UNROLL * ADJ_UNROLL;
            for (int e = tid; e < cntu * CG; e += ADJ_TILE) {
                int i, c;
                if (it.gy_pitch) { c = e / cntu; i = e - c * cntu; } else { i = e / CG; c = e - i * CG; }
                const unsigned int g = g0 + (unsigned int)(n0 + i);
                art_s v = 0;
                if (i < cnt && ch0 + c < it.C && g < it.gy_frames)
                    v = it.gy_pitch ? it.gy [(size_t)(ch0 + c) * it.gy_pitch + g] : it.gy [(size_t) g * it.C + ch0 + c];
                s_gy [i * CG + c] = v;
            }
            __syncthreads ();

            // ADJ_UNROLL outputs at a time, without a branch inside a group: which of them this lane has a term for, their coefficient loads all
            // in flight together, then one fused multiply-add per output in order — with the weight, or with a weight of zero where the lane has
            // no term, which leaves a sum of finite terms exactly as it was (w * gy = +-0, and s + +-0 = s, +0 for s = +0).  A lane's chain is
            // serial by definition: a lone clip has little else to hide a trip to the LDS or the cache behind.  A lane without a term reads tap 0
            // of row 0; a group no lane of the wave has a term for is skipped (short filters: most of a chunk lies outside a wave's 64 frames).
            for (int i0 = 0; i0 < cnt; i0 += ADJ_UNROLL) {    // (i0 + u < ADJ_CHUNK; positions past cnt are stale, and masked)
                bool ok [ADJ_UNROLL];
                int at [ADJ_UNROLL];
                bool any = false;
#pragma unroll
                for (int u = 0; u < ADJ_UNROLL; ++u) {
                    const int k = lin - s_w [i0 + u], row = s_row [i0 + u];
                    ok [u] = live && i0 + u < cnt && (unsigned int) k < (unsigned int) T;
                    if constexpr (!INTERP) { const int pass = s_pass [i0 + u]; if (pass >= 0 && k != pass) ok [u] = false; }
                    at [u] = ok [u] ? row + k : 0;
                    any = any || ok [u];
                }
                if (!__any (any)) continue;
                art_s w [ADJ_UNROLL];
#pragma unroll
                for (int u = 0; u < ADJ_UNROLL; ++u) {
                    const art_s *h = bank + at [u];
                    art_s v;
                    if constexpr (INTERP) {
                        const double left = (double) h [0] * s_f0 [i0 + u], right = (double) h [T] * s_f1 [i0 + u];
                        v = (art_s)(left + right);
                    }
                    else v = s_pass [i0 + u] >= 0 ? (art_s) 1 : h [0];
                    w [u] = ok [u] ? v : (art_s) 0;
                }
#pragma unroll
                for (int u = 0; u < ADJ_UNROLL; ++u)
#pragma unroll
                    for (int c = 0; c < CG; ++c) acc [c] = fused (w [u], s_gy [(i0 + u) * CG + c], acc [c]);
            }
        }
    }

    if (j < nin)
#pragma unroll
        for (int c = 0; c < CG; ++c)
            if (ch0 + c < it.C) {
                if (it.gx_pitch) it.gx [(size_t)(ch0 + c) * it.gx_pitch + j] = acc [c];
                else it.gx [(size_t) j * it.C + ch0 + c] = acc [c];
            }
}

// The same tiles for a clip made block by block (resampleAdjointScheduleClipsPlanarDevice): any number of phases — a process call per block, each at
// its own ratio, then the flush — where fir_adjoint_kernel has two.  Phase k holds input frame j at linear index H + j - start_k and reads
// nothing below its floor or at or past end_k.  start and end do not decrease from phase to phase, so the phases that can touch the tile
// (end > j0, start - H <= j1 - 1) are one contiguous range, found by bisection.  They are taken ADJ_GROUP at a time: two lanes per phase
// bisect its output range into a table of fixed size, so the LDS does not depend on the block count; a phase without outputs (a tiny
// block) or without an output on the tile costs its two bisections and is skipped.  Inside a phase the walk is adj_walk (fir_adjoint_walk.hip.h: the chunk loop above, shared with fir_sample.hip); the
// phases in order give the lane's terms in ascending output order.
constexpr int ADJ_GROUP = 32;            // phases whose ranges are bisected together
static_assert (2 * ADJ_GROUP <= ADJ_TILE, "two lanes per phase of a group");

template <int CG, bool INTERP>
__global__ __launch_bounds__ (ADJ_TILE)
void fir_adjoint_blocks_kernel (const ArtAdjBlocksItem *items, int count, const ArtAdjPhase *phases, const double *seg_base, const unsigned int *seg_first,
                                const int *seg_lin_base)
{
    __shared__ int s_w [ADJ_CHUNK];
    __shared__ int s_row [ADJ_CHUNK];
    __shared__ int s_pass [ADJ_CHUNK];
    __shared__ double s_f0 [INTERP ? ADJ_CHUNK : 1], s_f1 [INTERP ? ADJ_CHUNK : 1];
    __shared__ art_s s_gy [ADJ_CHUNK * CG];
    __shared__ int s_range [ADJ_GROUP][2];            // per phase of the group: first output of the range, one past its last

    const int tid = threadIdx.x;

    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items [mid].tile0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ArtAdjBlocksItem &it = items [lo];
    const int ch0 = (int) blockIdx.y * CG;
    if (ch0 >= it.C) return;

    const int T = it.T, half = T / 2, H = T + half, nin = it.in_frames;
    const int j0 = (int)(blockIdx.x - it.tile0) * ADJ_TILE;
    const int j1 = min (j0 + ADJ_TILE, nin);
    const int j = j0 + tid;
    const ArtAdjPhase *const ph = phases + it.phase_first;
    const int np = it.phase_count;                     // (>= 2: a block at least, and the flush, whose end = nin > j0)

    // [p_first, p_end): the first phase that ends past j0, up to the first that starts more than a history past the tile's last frame
    lo = 0; hi = np - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ph [mid].end > j0) hi = mid; else lo = mid + 1;
    }
    const int p_first = lo;
    lo = p_first; hi = np;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ph [mid].start - H > j1 - 1) hi = mid; else lo = mid + 1;
    }
    const int p_end = lo;

    art_s acc [CG];
#pragma unroll
    for (int c = 0; c < CG; ++c) acc [c] = 0;

    for (int pg = p_first; pg < p_end; pg += ADJ_GROUP) {
        const int in_group = min (ADJ_GROUP, p_end - pg);
        __syncthreads ();                              // (the group before is done with the table)
        if (tid < 2 * in_group) {
            const ArtAdjPhase &P = ph [pg + (tid >> 1)];
            int at = 0;
            if (P.outputs) {
                const AdjRate rate = { P.ratio, it.F };
                const AdjSegs segs = { P.seg_count, seg_first + P.seg_first, seg_lin_base + P.seg_first, seg_base + P.seg_first };
                // windows [w, w + T - 1] that meet the tile's frames [j0 + off, j1 - 1 + off], off = H - start
                const int off = H - P.start;
                const int bound = (tid & 1) ? j1 - 1 + off : j0 + off - T;
                at = adj_first_above<INTERP> (rate, segs, P.outputs, half, bound);
            }
            s_range [tid >> 1][tid & 1] = at;
        }
        __syncthreads ();

        for (int q = 0; q < in_group; ++q) {
            const int n_begin = s_range [q][0], n_end = s_range [q][1];
            if (n_begin >= n_end) continue;            // (the same for every thread)
            const ArtAdjPhase &P = ph [pg + q];
            const AdjRate rate = { P.ratio, it.F };
            const AdjSegs segs = { P.seg_count, seg_first + P.seg_first, seg_lin_base + P.seg_first, seg_base + P.seg_first };
            const int lin = j + (H - P.start);
            const bool live = j < nin && j < P.end && lin >= P.floor;
            adj_walk<CG, INTERP> (acc, it, rate, segs, ch0, tid, lin, live, P.first_output, n_begin, n_end, s_w, s_row, s_pass, s_f0, s_f1, s_gy);
        }
    }

    if (j < nin)
#pragma unroll
        for (int c = 0; c < CG; ++c)
            if (ch0 + c < it.C) {
                if (it.gx_pitch) it.gx [(size_t)(ch0 + c) * it.gx_pitch + j] = acc [c];
                else it.gx [(size_t) j * it.C + ch0 + c] = acc [c];
            }
}

template <typename Item>
inline int adj_variant (const Item &it)
{
    return (it.C > 4 ? 3 : it.C > 2 ? 2 : it.C == 2 ? 1 : 0) * 2 + (it.interpolate ? 1 : 0);
}

// a variant's launch, for either kernel: adj_enqueue calls both overloads the same way, so the two-phase kernel's takes the phase table
// (the blocks kernel's; NULL for it) and leaves it unnamed
template <int CG>
void adj_launch (bool interp, dim3 grid, hipStream_t st, const ArtAdjItem *d_items, int count, const ArtAdjPhase *, const double *b, const unsigned int *f, const int *l)
{
    if (interp) hipLaunchKernelGGL ((fir_adjoint_kernel<CG, true>), grid, dim3 (ADJ_TILE), 0, st, d_items, count, b, f, l);
    else hipLaunchKernelGGL ((fir_adjoint_kernel<CG, false>), grid, dim3 (ADJ_TILE), 0, st, d_items, count, b, f, l);
}

template <int CG>
void adj_launch (bool interp, dim3 grid, hipStream_t st, const ArtAdjBlocksItem *d_items, int count, const ArtAdjPhase *p, const double *b, const unsigned int *f, const int *l)
{
    if (interp) hipLaunchKernelGGL ((fir_adjoint_blocks_kernel<CG, true>), grid, dim3 (ADJ_TILE), 0, st, d_items, count, p, b, f, l);
    else hipLaunchKernelGGL ((fir_adjoint_blocks_kernel<CG, false>), grid, dim3 (ADJ_TILE), 0, st, d_items, count, p, b, f, l);
}

// the table: the items, the phases (the blocks kernel's), then the segments as three arrays (doubles first: every array keeps its alignment)
template <typename Item>
inline size_t adj_items_bytes (int n) { return (sizeof (Item) * (size_t) n + 7) & ~(size_t) 7; }
static_assert (sizeof (ArtAdjPhase) % 8 == 0, "the segments' doubles follow the phases");

template <typename Item>
inline size_t adj_table_bytes (int nitems, int nphases, int nsegs)
{
    return adj_items_bytes<Item> (nitems) + sizeof (ArtAdjPhase) * (size_t) nphases + (sizeof (double) + sizeof (unsigned int) + sizeof (int)) * (size_t) nsegs;
}

template <typename Item>
int adj_enqueue (const Item *items, int n, const ArtAdjPhase *phases, int nphases, const ArtamdSegment *segs, int nsegs, void *d_table, hipStream_t st)
{
    if (n <= 0) return 0;
    const size_t bytes = adj_table_bytes<Item> (n, nphases, nsegs), at_phases = adj_items_bytes<Item> (n), at_segs = at_phases + sizeof (ArtAdjPhase) * (size_t) nphases;
    Staging *sg = staging_take (bytes);
    if (!sg) return -1;

    Item *host = (Item *) sg->host;
    if (nphases) memcpy ((char *) sg->host + at_phases, phases, sizeof (ArtAdjPhase) * (size_t) nphases);
    double *base = (double *)((char *) sg->host + at_segs);
    unsigned int *first = (unsigned int *)(base + nsegs);
    int *lin_base = (int *)(first + nsegs);
    for (int q = 0; q < nsegs; ++q) { base [q] = segs [q].base_offset; first [q] = segs [q].first_output; lin_base [q] = segs [q].lin_base; }

    // the items by variant, each variant's one after another: a launch gets its slice
    struct { int first, count; unsigned int tiles, groups; } slice [8];
    int done = 0;
    for (int v = 0; v < 8; ++v) {
        slice [v].first = done; slice [v].count = 0; slice [v].tiles = 0; slice [v].groups = 1;
        const int cg = 1 << (v >> 1);
        for (int i = 0; i < n; ++i) {
            if (adj_variant (items [i]) != v) continue;
            Item &it = host [done++];
            it = items [i];
            it.tile0 = slice [v].tiles;
            slice [v].tiles += (unsigned int)((it.in_frames + ADJ_TILE - 1) / ADJ_TILE);
            const unsigned int groups = (unsigned int)((it.C + cg - 1) / cg);
            if (groups > slice [v].groups) slice [v].groups = groups;
            ++slice [v].count;
        }
    }

    if (hipMemcpyAsync (d_table, sg->host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { (void) staging_give (sg, st); return -1; }
    const Item *d_items = (const Item *) d_table;
    const ArtAdjPhase *d_phases = (const ArtAdjPhase *)((const char *) d_table + at_phases);
    const double *d_base = (const double *)((const char *) d_table + at_segs);
    const unsigned int *d_first = (const unsigned int *)(d_base + nsegs);
    const int *d_lin_base = (const int *)(d_first + nsegs);

    int launches = 0;
    bool ok = true;
    for (int v = 0; v < 8 && ok; ++v) {
        if (!slice [v].count) continue;
        const dim3 grid (slice [v].tiles, slice [v].groups);
        const Item *d = d_items + slice [v].first;
        const bool interp = (v & 1) != 0;
        switch (v >> 1) {
            case 3: adj_launch<8> (interp, grid, st, d, slice [v].count, d_phases, d_base, d_first, d_lin_base); break;
            case 2: adj_launch<4> (interp, grid, st, d, slice [v].count, d_phases, d_base, d_first, d_lin_base); break;
            case 1: adj_launch<2> (interp, grid, st, d, slice [v].count, d_phases, d_base, d_first, d_lin_base); break;
            default: adj_launch<1> (interp, grid, st, d, slice [v].count, d_phases, d_base, d_first, d_lin_base); break;
        }
        ok = hipGetLastError () == hipSuccess;
        if (ok) ++launches;
    }
    if (staging_give (sg, st)) ok = false;
    return ok ? launches : -1;
}

} // namespace

extern "C" {

size_t arthip_fir_adjoint_bytes (int nitems, int nsegs) { return adj_table_bytes<ArtAdjItem> (nitems, 0, nsegs); }

int arthip_fir_adjoint (const ArtAdjItem *items, int n, const ArtamdSegment *segs, int nsegs, void *d_table, void *stream)
{
    return adj_enqueue (items, n, (const ArtAdjPhase *) 0, 0, segs, nsegs, d_table, (hipStream_t) stream);
}

size_t arthip_fir_adjoint_blocks_bytes (int nitems, int nphases, int nsegs) { return adj_table_bytes<ArtAdjBlocksItem> (nitems, nphases, nsegs); }

int arthip_fir_adjoint_blocks (const ArtAdjBlocksItem *items, int n, const ArtAdjPhase *phases, int nphases, const ArtamdSegment *segs, int nsegs,
                               void *d_table, void *stream)
{
    return adj_enqueue (items, n, phases, nphases, segs, nsegs, d_table, (hipStream_t) stream);
}

} // extern "C"
