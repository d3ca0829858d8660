// fir_band.hip — whole clips at a position curve, band-limited per output from a LADDER of banks (gfx950): the kernels of
// resampleSampleBandClipsPlanarDevice, resampleSampleBandAdjointClipsPlanarDevice and resampleSampleBandGradientsClipsPlanarDevice.  What a mip
// chain is to a texture sampler: an item holds K banks of one shape at descending cut-offs (rung 0 the widest) and, beside its positions, a
// curve of levels — doubles in device memory.  An output's level l picks two neighbouring rungs and blends them:
//     !(l > 0) (a NaN, -0.0, a negative): L = 0, lam = 0;   l >= K - 1: L = K - 1, lam = 0;   else L = floor (l), lam = l - L.
// The position arithmetic is fir_sample.hip's (sample_locate<true>, fir_sample_common.hip.h: the one copy), and so are the task spaces, the
// bisections and the summation trees.  With a_k = s0 (1 - frac) + s1 frac the value of rung k in double — fir_sample_kernel's chains and its
// lerp before the rounding —
//   fir_band_kernel          y = (art_s) a_L where lam == 0: rung L + 1 is not read, and the bits are fir_sample_kernel's on rung L's bank;
//                            elsewhere y = (art_s)(a_L (1.0 - lam) + a_{L+1} lam), the two rungs' chains side by side over one pass of the
//                            samples.  Lanes of a wave may sit on different rungs: their rows come from L2, as the sampler's do.
//   fir_band_adjoint_kernel  the transpose: fir_sample_adjoint_kernel's tiles, range and walk (adj_walk's BAND form) with the weight
//                            (art_s)(w_L (1.0 - lam) + w_{L+1} lam), w_k = h0 f0 + h1 f1 unrounded, and rung L's own weight where lam == 0.
//                            PRECONDITION: the positions do not decrease; the levels may be anything.
//   fir_band_slope_kernel    gp [m] = sum_c gy D with D = D_L where lam == 0 (fir_sample_slope_kernel's bits) and D_L (1.0 - lam) + D_{L+1} lam
//                            elsewhere; gl [m] = sum_c gy (a_{j+1} - a_j), j = min (L, K - 2), for 0 <= l <= K - 1 (-0.0 among them: the
//                            closed ends pass the gradient, as a clamp's do) and exactly 0 elsewhere, for a NaN, for K = 1 and without a
//                            window.  An item asks for either or both; the value chains are run only where gl is asked for.
// No atomics, no counters; every value is one fixed tree of its own clip's terms.  Compiled with -ffp-contract=off.
#include <cstring>
#include "fir_sample_common.hip.h"
#include "staging.hip.h"

namespace {

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

// adj_walk's position source of a banded item: the sampler's curve, and the levels beside it
struct BandCurve : SampleCurve { const double *level; int K; };

__device__ __forceinline__ void adj_level (const BandCurve &c, unsigned int n, int &rung, double &lam) { band_level (c.level [n], c.K, rung, lam); }

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
__device__ __forceinline__ void band_group (const ArtBandItem &it, int c0, int j0, long (&at) [SM_CH])
{
#pragma unroll
    for (int u = 0; u < SM_CH; ++u) {
        const int c = min (c0 + u, it.C - 1);
        at [u] = it.in_pitch ? (long) c * it.in_pitch + j0 : (long) j0 * it.C + c;
    }
}

__global__ __launch_bounds__ (SM_TILE)
void fir_band_kernel (const ArtBandItem *items, int count)
{
    const unsigned int task = blockIdx.x;
    const ArtBandItem &it = items [sample_item_of (items, count, task)];
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

__device__ __forceinline__ double band_gy (const ArtBandItem &it, int c, unsigned int m)
{
    return (double)(it.gy_pitch ? it.gy [(size_t) c * it.gy_pitch + m] : it.gy [(size_t) m * it.C + c]);
}

// one output of the gradients: WANT_P: gp, WANT_L: gl (one of them at least)
template <bool WANT_P, bool WANT_L>
__device__ __forceinline__ void band_gradients (const ArtBandItem &it, unsigned int m)
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
void fir_band_slope_kernel (const ArtBandItem *items, int count)
{
    const unsigned int task = blockIdx.x;
    const ArtBandItem &it = items [sample_item_of (items, count, task)];
    const unsigned int m = (task - it.task0) * SM_TILE + threadIdx.x;
    if (m >= it.gy_frames) return;
    // (the same branch for the whole launch: the entry's lists)
    if (it.gp && it.gl) band_gradients<true, true> (it, m);
    else if (it.gp) band_gradients<true, false> (it, m);
    else band_gradients<false, true> (it, m);
}

__global__ __launch_bounds__ (ADJ_TILE)
void fir_band_adjoint_kernel (const ArtBandItem *items, int count)
{
    __shared__ int s_w [ADJ_CHUNK];                   // window start of each output of the chunk
    __shared__ int s_row [ADJ_CHUNK];                 // its filter row's offset in a bank, in taps
    __shared__ int s_rung [ADJ_CHUNK];                // its rung L
    __shared__ double s_f0 [ADJ_CHUNK], s_f1 [ADJ_CHUNK];      // 1.0 - frac, frac
    __shared__ double s_lam [ADJ_CHUNK];              // its blend with rung L + 1 (0: that rung is not read)
    __shared__ art_s s_gy [ADJ_CHUNK * 4];
    __shared__ int s_range [2];                       // first output of the range, one past its last

    const unsigned int task = blockIdx.x;
    const ArtBandItem &it = items [sample_item_of (items, count, task)];
    const int cg = sample_group (it.C), groups = (it.C + cg - 1) / cg;
    const int local = (int)(task - it.task0), tile = local / groups, ch0 = (local - tile * groups) * cg;
    BandCurve curve;
    curve.pos = it.pos; curve.level = it.level; curve.K = it.rungs;

    // (the same branch for the whole workgroup: the item's)
    if (cg == 4) sample_adjoint_tile<4, true, true> (it, curve, tile, ch0, s_w, s_row, nullptr, s_f0, s_f1, s_gy, s_range, s_rung, s_lam);
    else if (cg == 2) sample_adjoint_tile<2, true, true> (it, curve, tile, ch0, s_w, s_row, nullptr, s_f0, s_f1, s_gy, s_range, s_rung, s_lam);
    else sample_adjoint_tile<1, true, true> (it, curve, tile, ch0, s_w, s_row, nullptr, s_f0, s_f1, s_gy, s_range, s_rung, s_lam);
}

} // namespace

extern "C" {

unsigned long arthip_fir_band_tasks (const ArtBandItem *it, int what)
{
    if (what != ART_SAMPLE_ADJOINT) return ((unsigned long) it->gy_frames + SM_TILE - 1) / SM_TILE;
    const int cg = sample_group (it->C);
    return (((unsigned long) it->in_frames + ADJ_TILE - 1) / ADJ_TILE) * (unsigned long)((it->C + cg - 1) / cg);
}

size_t arthip_fir_band_bytes (int nitems) { return sizeof (ArtBandItem) * (size_t) nitems; }

int arthip_fir_band (const ArtBandItem *items, int n, int what, void *d_table, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    if (n <= 0) return 0;
    const size_t bytes = arthip_fir_band_bytes (n);
    Staging *sg = staging_take (bytes);
    if (!sg) return -1;

    ArtBandItem *host = (ArtBandItem *) sg->host;
    unsigned long next = 0;
    for (int i = 0; i < n; ++i) {
        host [i] = items [i];
        host [i].task0 = (unsigned int) next;
        next += arthip_fir_band_tasks (&items [i], what);
    }
    if (next > 0x7fffffffUL) { (void) staging_give (sg, st); return -1; }

    if (hipMemcpyAsync (d_table, sg->host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { (void) staging_give (sg, st); return -1; }
    const ArtBandItem *d_items = (const ArtBandItem *) d_table;
    const dim3 grid ((unsigned int) next);
    switch (what) {
        case ART_SAMPLE_FORWARD: hipLaunchKernelGGL (fir_band_kernel, grid, dim3 (SM_TILE), 0, st, d_items, n); break;
        case ART_SAMPLE_ADJOINT: hipLaunchKernelGGL (fir_band_adjoint_kernel, grid, dim3 (ADJ_TILE), 0, st, d_items, n); break;
        default: hipLaunchKernelGGL (fir_band_slope_kernel, grid, dim3 (SM_TILE), 0, st, d_items, n); break;
    }
    bool ok = hipGetLastError () == hipSuccess;
    if (staging_give (sg, st)) ok = false;
    return ok ? 1 : -1;
}

} // extern "C"
