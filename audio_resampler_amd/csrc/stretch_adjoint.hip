// stretch_adjoint.hip — the transpose of a logged stage of the time stretcher (gfx950): stretchAdjointClipsPlanarDevice's kernel.
//
// With the period search's choices held fixed a stage is the sparse map its splice log spells out (art_hip.h): every output value a
// copy of one input value or a fade of two.  The forward is a chain of decisions, one workgroup per clip; the transpose has no chain.
// A workgroup owns SADJ_TILE consecutive INPUT values of one clip, a lane one value v, and gathers: for every segment that reads v,
// the term of the output it goes to.  `from` never falls along the log, and a segment reads only [from - back, from + ahead) (a
// longest period behind — the 2:1 step's second source, the 3:2 step's — and no more than the ring in front), so the segments that can
// touch the tile are ONE contiguous range of the log, whose ends two lanes find by bisection over `from`.  The range goes through the
// LDS SADJ_CHUNK records at a time, so the LDS does not depend on the clip or the periods; every lane walks the chunk, all lanes
// reading one record (an LDS broadcast), and consecutive lanes read consecutive gy (coalesced).  A lane adds its terms in log order,
// which is ascending output order, so gx [v] does not depend on the tile, the chunk, the batch or the layout.  No atomics.
//
// Compiled with -ffp-contract=off: a term is a product, a quotient and a sum, each rounded.
#include <hip/hip_runtime.h>
#include "art_internal.h"

namespace {

constexpr int SADJ_TILE = 256;           // input values per workgroup = its threads
constexpr int SADJ_CHUNK = 256;          // segments per trip through the LDS (4 KiB)

// value v of a clip's rows: channel v & shift of frame v >> shift (channels 1 or 2), as stretch_kernels.hip's Rows
__device__ __forceinline__ long value_at (int v, long pitch, int shift)
{
    return pitch ? (long)(v & shift) * pitch + (long)(v >> shift) : (long) v;
}

// first segment of [0, count) whose `from` is at least `bound` (count: none)
__device__ int first_from_at_least (const ArtamdStretchSegment *log, int count, long bound)
{
    int lo = 0, hi = count;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if ((long) log [mid].from >= bound) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__ (SADJ_TILE)
void stretch_adjoint_kernel (const ArtStretchAdjItem *items, int count)
{
    __shared__ ArtamdStretchSegment s_seg [SADJ_CHUNK];
    __shared__ int s_range [2];

    const int tid = threadIdx.x;

    // the tile's item: the last whose first tile is <= blockIdx.x (every item has a tile at least)
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items [mid].tile0 <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ArtStretchAdjItem &it = items [lo];

    // a pair's intermediate stream is as long as stage 1's log says: this stage's input (stage 2) or output (stage 1)
    int gx_values = it.gx_values, gy_values = it.gy_values;
    if (it.mid) {
        int made = 0;
        if (it.mid_count > 0) { const ArtamdStretchSegment last = it.mid [it.mid_count - 1]; made = last.out + last.count; }
        if (it.mid_is_gx) gx_values = min (gx_values, made); else gy_values = made;
    }

    const int v0 = (int)(blockIdx.x - it.tile0) * SADJ_TILE;
    if (v0 >= gx_values) return;                   // (the tiles were laid out for the host's bound)
    const int v1 = min (v0 + SADJ_TILE, gx_values);
    const int v = v0 + tid;
    const int shift = it.channels - 1;

    // segments with  from - back < v1  and  from + ahead > v0
    if (tid < 2)
        s_range [tid] = first_from_at_least (it.log, it.count, tid ? (long) v1 + it.back : (long) v0 - it.ahead + 1);
    __syncthreads ();
    const int q_end = s_range [1];

    const art_s *const gy = it.gy;
    const long gy_pitch = it.gy_pitch;
    art_s acc = 0;

    for (int q0 = s_range [0]; q0 < q_end; q0 += SADJ_CHUNK) {
        const int cnt = min (SADJ_CHUNK, q_end - q0);
        __syncthreads ();                          // (the chunk before is done with)
        if (tid < cnt) s_seg [tid] = it.log [q0 + tid];
        __syncthreads ();

        for (int q = 0; q < cnt; ++q) {
            const ArtamdStretchSegment s = s_seg [q];
            const unsigned int n = (unsigned int) s.count;
            const unsigned int i = (unsigned int)(v - s.from);          // (a wrapped difference is out of range either way)
            if (s.to == ARTAMD_STRETCH_COPY) {
                if (i < n && s.out + (int) i < gy_values) acc = acc + gy [value_at (s.out + (int) i, gy_pitch, shift)];
                continue;
            }
            // a fade: the term through `from` (weight count - i) and the term through `to` (weight i), the lower output first
            const unsigned int k = (unsigned int)(v - s.to);
            const bool hit_from = i < n && s.out + (int) i < gy_values, hit_to = k < n && s.out + (int) k < gy_values;
            if (!hit_from && !hit_to) continue;
            const art_s cnt_s = (art_s) s.count;
            art_s t_from = 0, t_to = 0;
            if (hit_from) t_from = (gy [value_at (s.out + (int) i, gy_pitch, shift)] * (art_s)(s.count - (int) i)) / cnt_s;
            if (hit_to) t_to = (gy [value_at (s.out + (int) k, gy_pitch, shift)] * (art_s)(int) k) / cnt_s;
            const bool from_first = s.from > s.to;                      // i < k
            if (hit_from && from_first) acc = acc + t_from;
            if (hit_to) acc = acc + t_to;
            if (hit_from && !from_first) acc = acc + t_from;
        }
    }

    if (v < v1) it.gx [value_at (v, it.gx_pitch, shift)] = acc;
}

} // namespace

extern "C" int arthip_stretch_adjoint (ArtStretchAdjItem *items, int n, void *d_table, void *stream)
{
    if (n <= 0) return 0;
    unsigned int tiles = 0;
    for (int i = 0; i < n; ++i) {
        items [i].tile0 = tiles;
        const unsigned int own = (unsigned int)((items [i].gx_values + SADJ_TILE - 1) / SADJ_TILE);
        tiles += own ? own : 1;
    }
    if (arthip_table_upload (items, sizeof (ArtStretchAdjItem) * (size_t) n, d_table, stream)) return -1;
    hipLaunchKernelGGL (stretch_adjoint_kernel, dim3 (tiles), dim3 (SADJ_TILE), 0, (hipStream_t) stream, (const ArtStretchAdjItem *) d_table, n);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}
