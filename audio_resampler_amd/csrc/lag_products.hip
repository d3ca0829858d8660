// lag_products.hip — lagged inner products of whole rows (gfx950): artamdLagProductsBatchDevice's kernels.
//
// Row i asks for sums [q] = sum_{t = k}^{frames - 1} (double) u [t] * (double) v [t - k], k = first + q, q = 0 .. lags - 1 (at most
// ART_LAG_MAX lags below ART_LAG_MAX): what the coefficient gradient of a biquad section is made of.  A row is cut into tiles of
// ART_LAG_TILE frames; a workgroup owns one (row, tile) task of the call's flattened task space and finds its row by bisection over
// the rows' first tasks, so 2 rows of a million frames and 4,096 rows of 700 both spread over the chip.
//
// A tile goes through the LDS in passes of LP_PASS frames: u [p0 ..] and v [p0 - ART_LAG_MAX ..], loaded 16 bytes at a time where
// the row's own address allows (single accesses at the head and the tail) and, from there on, addressed by FRAME: thread j takes
// the frames p0 + j + 256 i in ascending order, one explicit fma per lag, then the 64 lanes of a wave are folded by a butterfly and
// the four waves added in wave order.  So a tile's partial is one fixed tree of the row's frames, whatever the base alignment of
// u and v, the other rows of the call, the row's place in the list or the stream.  The partials go to scratch; a second, small
// launch (one wave per row) adds a row's partials in ascending tile order and SETS the row's sums.  No atomics, no counters: the
// launch boundary is the reduction's only hand-off.
//
// Products and sums are fp64 in both builds (exact products in the 4-byte build).  Compiled with -ffp-contract=off: the only fused
// operation is the accumulation's explicit fma.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <mutex>
#include "art_internal.h"

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_PASS = 2048;                        // frames in the LDS at a time
constexpr int LP_VEC = (int)(16 / sizeof (art_s));   // samples per 16-byte load
constexpr int LP_FINISH = 64;                        // the finishing launch: one wave per row, this many partials per trip
static_assert (ART_LAG_TILE % LP_PASS == 0 && LP_PASS % LP_THREADS == 0, "whole passes per tile, whole rounds per pass");
static_assert (ART_LAG_MAX % LP_VEC == 0, "the look-back keeps 16-byte groups whole");

// the row a task belongs to: the last whose first task is <= task (rows [0].task0 == 0, ascending)
__device__ __forceinline__ const ArtLagRow &lag_row_of (const ArtLagRow *rows, int n, long task)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (rows [mid].task0 <= task) lo = mid; else hi = mid - 1; }
    return rows [lo];
}

// dst [j] = src [base + j] for j = 0 .. count - 1 where 0 <= base + j < frames, else 0.  Groups of LP_VEC samples are cut where the
// ADDRESS of src is a multiple of 16 (src is aligned to its sample size); a group that lies whole inside both ranges is one load.
__device__ __forceinline__ void lag_stage (art_s *dst, const art_s *src, long base, int count, long frames, int tid)
{
    typedef art_s vec_t __attribute__ ((ext_vector_type (LP_VEC)));
    const int m = (int)((((uintptr_t) src / sizeof (art_s)) + (uintptr_t)(base & (LP_VEC - 1))) & (LP_VEC - 1));
    const int groups = (count + m + LP_VEC - 1) / LP_VEC;
    for (int g = tid; g < groups; g += LP_THREADS) {
        const int j0 = g * LP_VEC - m;
        const long f0 = base + j0;
        if (j0 >= 0 && j0 + LP_VEC <= count && f0 >= 0 && f0 + LP_VEC <= frames) {
            const vec_t x = *reinterpret_cast<const vec_t *> (src + f0);
#pragma unroll
            for (int e = 0; e < LP_VEC; ++e) dst [j0 + e] = x [e];
            continue;
        }
#pragma unroll
        for (int e = 0; e < LP_VEC; ++e) {
            const int j = j0 + e;
            if (j >= 0 && j < count) dst [j] = (f0 + e >= 0 && f0 + e < frames) ? src [f0 + e] : (art_s) 0;
        }
    }
}

// one pass's terms of this thread, frames p0 + tid + 256 i ascending.  GUARD: the pass touches frame `first + q` > t or frames >= n
// (the first and the last pass of a row); such terms are left out, not multiplied by zero (a non-finite neighbour stays out).
template <bool GUARD>
__device__ __forceinline__ void lag_pass (double (&acc) [ART_LAG_MAX], const art_s *su, const art_s *sv, long p0, long frames,
                                          int first, int lags, int tid)
{
#pragma unroll
    for (int i = 0; i < LP_PASS / LP_THREADS; ++i) {
        const int idx = tid + LP_THREADS * i;
        const long t = p0 + idx;
        if (GUARD && p0 + LP_THREADS * i >= frames) break;          // (the same for every thread: a round past the row's end adds nothing)
        const double uu = (double) su [idx];
        const art_s *const vp = sv + ART_LAG_MAX + idx - first;
#pragma unroll
        for (int q = 0; q < ART_LAG_MAX; ++q) {
            if (q >= lags) break;
            const double sum = fma (uu, (double) vp [-q], acc [q]);
            acc [q] = !GUARD || (t < frames && t >= first + q) ? sum : acc [q];
        }
    }
}

__global__ __launch_bounds__ (LP_THREADS)
void lag_products_tile_kernel (const ArtLagRow *rows, int n, double *partials)
{
    __shared__ art_s su [LP_PASS];
    __shared__ art_s sv [LP_PASS + ART_LAG_MAX];                    // sv [j]: v [p0 - ART_LAG_MAX + j]
    __shared__ double red [LP_WAVES][ART_LAG_MAX];

    const int tid = threadIdx.x;
    const long task = blockIdx.x;
    const ArtLagRow &a = lag_row_of (rows, n, task);
    const long frames = a.frames, t0 = (task - a.task0) * ART_LAG_TILE;
    const int first = a.first, lags = a.lags;
    const art_s *const u = a.u, *const v = a.v;

    double acc [ART_LAG_MAX];
#pragma unroll
    for (int q = 0; q < ART_LAG_MAX; ++q) acc [q] = 0.0;

    for (int pass = 0; pass < ART_LAG_TILE / LP_PASS; ++pass) {
        const long p0 = t0 + (long) pass * LP_PASS;
        if (p0 >= frames) break;                                    // (the same for every thread)
        if (pass) __syncthreads ();
        // (a short last pass stages only the rounds that have frames: lag_pass stops where they end)
        const int staged = frames - p0 < LP_PASS ? (int)((frames - p0 + LP_THREADS - 1) / LP_THREADS) * LP_THREADS : LP_PASS;
        lag_stage (su, u, p0, staged, frames, tid);
        lag_stage (sv, v, p0 - ART_LAG_MAX, staged + ART_LAG_MAX, frames, tid);
        __syncthreads ();
        if (p0 < ART_LAG_MAX || p0 + LP_PASS > frames) lag_pass<true> (acc, su, sv, p0, frames, first, lags, tid);
        else lag_pass<false> (acc, su, sv, p0, frames, first, lags, tid);
    }

    // the tile's tree: a butterfly over the wave's lanes (every lane ends with the same bits), then the waves in order
#pragma unroll
    for (int q = 0; q < ART_LAG_MAX; ++q) {
        if (q >= lags) break;
        double s = acc [q];
#pragma unroll
        for (int off = 32; off; off >>= 1) s += __shfl_xor (s, off, 64);
        if (!(tid & 63)) red [tid >> 6][q] = s;
    }
    __syncthreads ();
    if (tid < lags) {
        double s = red [0][tid];
#pragma unroll
        for (int w = 1; w < LP_WAVES; ++w) s += red [w][tid];
        partials [task * ART_LAG_MAX + tid] = s;
    }
}

// one wave per row: the row's partials in ascending tile order, LP_FINISH tiles' loads in flight per trip; lane q adds lag first + q
__global__ __launch_bounds__ (LP_FINISH)
void lag_products_finish_kernel (const ArtLagRow *rows, int n, const double *partials)
{
    __shared__ double sp [LP_FINISH][ART_LAG_MAX];
    const int tid = threadIdx.x;
    const ArtLagRow &a = rows [blockIdx.x];
    const int lags = a.lags;
    const long tiles = ((long) a.frames + ART_LAG_TILE - 1) / ART_LAG_TILE;
    const double *const p = partials + a.task0 * ART_LAG_MAX;
    double s = 0.0;
    for (long c0 = 0; c0 < tiles; c0 += LP_FINISH) {
        const int cnt = tiles - c0 < LP_FINISH ? (int)(tiles - c0) : LP_FINISH;
        if (c0) __syncthreads ();
        if (tid < cnt)
            for (int q = 0; q < lags; ++q) sp [tid][q] = p [(c0 + tid) * ART_LAG_MAX + q];
        __syncthreads ();
        if (tid < lags)
            for (int l = 0; l < cnt; ++l) s += sp [l][tid];
    }
    if (tid < lags) a.sums [tid] = s;
}

// The call has no context to keep its table and partials in: one scratch per device for the process, grown under `lag_lock`.  `ev`
// marks the last launch that used it; a call on another stream waits for it on the device before the scratch is rewritten, and
// growing waits for it on the host.  Like the pinned staging (device_rt.hip) it lives as long as the process.
struct LagScratch { ArtLagRow *h_rows; size_t h_cap; void *d_rows; size_t rows_cap; void *d_part; size_t part_cap; hipEvent_t ev; hipStream_t last; bool used; };
LagScratch lag_scratch [ART_MAX_DEVICES];
std::mutex lag_lock;

// a device buffer of `need` bytes at least (content lost when it grows); false when out of memory
bool lag_reserve (LagScratch &s, void *&dev, size_t &cap, size_t need)
{
    if (need <= cap) return true;
    if (s.used) { (void) hipEventSynchronize (s.ev); s.used = false; }
    if (dev) (void) hipFree (dev);
    dev = nullptr; cap = 0;
    const size_t want = need + need / 2 + 4096;
    if (hipMalloc (&dev, want) != hipSuccess) { dev = nullptr; (void) hipGetLastError (); return false; }
    cap = want;
    return true;
}

} // namespace

extern "C" {

int arthip_lag_products (const art_s *const *d_u, const art_s *const *d_v, const int *frames, const int *first, const int *lags,
                         double *const *d_sums, int n, int live, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    int device = 0;
    if (live <= 0) return 0;
    if (hipGetDevice (&device) != hipSuccess || device < 0 || device >= ART_MAX_DEVICES) return -1;
    std::lock_guard<std::mutex> hold (lag_lock);
    LagScratch &s = lag_scratch [device];
    if ((size_t) live > s.h_cap) {
        const size_t want = (size_t) live + (size_t) live / 2 + 64;
        ArtLagRow *h = (ArtLagRow *) std::realloc (s.h_rows, want * sizeof (ArtLagRow));
        if (!h) return -1;
        s.h_rows = h; s.h_cap = want;
    }
    long tasks = 0;
    int j = 0;
    for (int i = 0; i < n; ++i) {
        if (frames [i] <= 0) continue;
        ArtLagRow &r = s.h_rows [j++];
        r.u = d_u [i]; r.v = d_v [i]; r.sums = d_sums [i];
        r.task0 = tasks;
        r.frames = frames [i]; r.first = first [i]; r.lags = lags [i]; r.pad = 0;
        tasks += ((long) frames [i] + ART_LAG_TILE - 1) / ART_LAG_TILE;
    }
    if (j != live || tasks > 0x7fffffffL) return -1;
    if (!s.ev && hipEventCreateWithFlags (&s.ev, hipEventDisableTiming) != hipSuccess) { s.ev = nullptr; return -1; }
    const size_t table = sizeof (ArtLagRow) * (size_t) live;
    if (!lag_reserve (s, s.d_rows, s.rows_cap, table) || !lag_reserve (s, s.d_part, s.part_cap, sizeof (double) * ART_LAG_MAX * (size_t) tasks)) return -1;
    if (s.used && s.last != st && hipStreamWaitEvent (st, s.ev, 0) != hipSuccess) return -1;
    if (arthip_table_upload (s.h_rows, table, s.d_rows, st)) return -1;
    hipLaunchKernelGGL (lag_products_tile_kernel, dim3 ((unsigned int) tasks), dim3 (LP_THREADS), 0, st, (const ArtLagRow *) s.d_rows, live, (double *) s.d_part);
    if (hipGetLastError () != hipSuccess) return -1;
    hipLaunchKernelGGL (lag_products_finish_kernel, dim3 ((unsigned int) live), dim3 (LP_FINISH), 0, st, (const ArtLagRow *) s.d_rows, live, (const double *) s.d_part);
    const bool ok = hipGetLastError () == hipSuccess;
    // (the scratch may be rewritten only after these launches: if the event cannot be recorded, wait for the stream instead)
    if (hipEventRecord (s.ev, st) != hipSuccess) { s.used = false; if (hipStreamSynchronize (st) != hipSuccess) return -1; }
    else { s.last = st; s.used = true; }
    return ok ? 2 : -1;
}

}
