// layout_kernels.hip — planar <-> interleaved copies of MANY buffers in one launch (the planar batch entries' staging, resampler_host.c).
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include "art_internal.h"
#include "staging.hip.h"

namespace {

// A task is (item, tile of `tile` consecutive frames x all C channels) and one workgroup; the item is found by binary search over the items'
// first tasks, as ingest_batch_kernel finds its own.  The tile passes through the LDS as [channel][frame], so that both sides of the copy are
// runs of consecutive addresses: a plane's frames on one side, frames x C interleaved samples on the other.  Streams of more than
// LAYOUT_CH channels pass in chunks of LAYOUT_CH channels (their interleaved side is then rows of LAYOUT_CH samples, C apart).
constexpr int LAYOUT_THREADS = 256;
constexpr int LAYOUT_CH = 256 / (int) sizeof (art_s);           // channels of a chunk: 64 (4-byte samples), 32 (8-byte)
constexpr int LAYOUT_MIN_TILE = 64;                              // frames of a tile, at least ...
constexpr int LAYOUT_TARGET = 2048;                              // ... and about this many samples (a stereo clip of 102,400 frames: 100 workgroups)
constexpr int LAYOUT_LDS = LAYOUT_CH * 2 * LAYOUT_MIN_TILE;      // samples: 32 KB in either build — every tile with its padding fits (layout_tile)
constexpr int VEC = 16 / (int) sizeof (art_s);                   // samples of a 16-byte access
typedef art_s vec_t __attribute__ ((ext_vector_type (VEC)));

// frames of a tile of a C-channel item, a multiple of 4.  With cc = min (C, LAYOUT_CH) channels in the LDS at a pitch below tile + 32:
// cc <= 32: cc * (2048 / cc + 32) <= 4096; above (4-byte build): cc * (64 + 32) < 8192.
__host__ __device__ inline int layout_tile (int C)
{
    const int cc = C < LAYOUT_CH ? C : LAYOUT_CH;
    const int tile = (LAYOUT_TARGET / cc) & ~3;
    return tile < LAYOUT_MIN_TILE ? LAYOUT_MIN_TILE : tile;
}

// The LDS pitch of a channel's frames, in samples.  The interleaved side walks the tile frame by frame: the 32 lanes of a half wave touch
// channels 0 .. cc-1 of ceil (32 / cc) consecutive frames, sample (c, f) at c * pitch + f.  A sample of either width is one bank of its
// access (ds_read_b32 / ds_write_b32: 32 banks per half wave; ds_read_b64: 64 dwords, two per sample), so with pitch = ceil (32 / cc) mod 32
// the lanes fall on c * ceil (32 / cc) + f: distinct banks (a plain pitch of `tile`, a multiple of 32 for the common widths, would put all
// channels of a frame on one bank).  The planar side walks along f: conflict-free at any pitch.
__device__ inline int layout_pitch (int tile, int cc)
{
    const int c = cc < 32 ? cc : 32, s = (32 + c - 1) / c;
    return tile + ((s - tile) & 31);
}

// One side of the copy where a channel's frames are consecutive in memory: channel c of the chunk, frames [0, nf), at g + c * pitch.
// A channel's run is cut at the 16-byte boundaries of its own address: the part in front of the first (quad 0) and the part behind the last
// move sample by sample, every whole quad as one 16-byte access — whatever base and pitch are (an odd pitch: every plane its own head).
template <bool TO_LDS>
__device__ inline void pass_planes (art_s *lds, int lp, art_s *g, long pitch, int nf, int cc)
{
    const int qmax = (nf + VEC - 1) / VEC + 1, total = cc * qmax;
    for (int idx = threadIdx.x; idx < total; idx += LAYOUT_THREADS) {
        const int c = idx / qmax, q = idx - c * qmax;
        art_s *const p = g + (size_t) c * pitch;
        art_s *const l = lds + c * lp;
        const int head = (int)(((16u - (unsigned int)((uintptr_t) p & 15u)) & 15u) / sizeof (art_s));
        const int b = q ? head + (q - 1) * VEC : 0;
        int e = q ? b + VEC : head;
        if (e > nf) e = nf;
        if (b >= e) continue;
        if (q && e - b == VEC) {
            if (TO_LDS) {
                const vec_t v = *(const vec_t *)(p + b);
#pragma unroll
                for (int j = 0; j < VEC; ++j) l [b + j] = v [j];
            }
            else {
                vec_t v;
#pragma unroll
                for (int j = 0; j < VEC; ++j) v [j] = l [b + j];
                *(vec_t *)(p + b) = v;
            }
        }
        else
            for (int j = b; j < e; ++j) { if (TO_LDS) l [j] = p [j]; else p [j] = l [j]; }
    }
}

// The other side, all C channels of the item in the chunk: the tile's nf x C interleaved samples are ONE run of consecutive addresses at g,
// cut at its 16-byte boundaries in the same way.  Sample j of the run is channel j % C of frame j / C.
template <bool TO_LDS>
__device__ inline void pass_frames (art_s *lds, int lp, art_s *g, int nf, int C)
{
    const int len = nf * C, total = (len + VEC - 1) / VEC + 1;
    const int head = (int)(((16u - (unsigned int)((uintptr_t) g & 15u)) & 15u) / sizeof (art_s));
    for (int q = threadIdx.x; q < total; q += LAYOUT_THREADS) {
        const int b = q ? head + (q - 1) * VEC : 0;
        int e = q ? b + VEC : head;
        if (e > len) e = len;
        if (b >= e) continue;
        int f = b / C, c = b - f * C;
        if (q && e - b == VEC) {
            vec_t v;
            if (TO_LDS) v = *(const vec_t *)(g + b);
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                if (TO_LDS) lds [c * lp + f] = v [j]; else v [j] = lds [c * lp + f];
                if (++c == C) { c = 0; ++f; }
            }
            if (!TO_LDS) *(vec_t *)(g + b) = v;
        }
        else
            for (int j = b; j < e; ++j) {
                if (TO_LDS) lds [c * lp + f] = g [j]; else g [j] = lds [c * lp + f];
                if (++c == C) { c = 0; ++f; }
            }
    }
}

// ... and a chunk of cc < C channels: rows of cc consecutive samples, C apart (g: the chunk's first channel in the tile's first frame)
template <bool TO_LDS>
__device__ inline void pass_rows (art_s *lds, int lp, art_s *g, int nf, int cc, int C)
{
    const int total = nf * cc;
    for (int j = threadIdx.x; j < total; j += LAYOUT_THREADS) {
        const int f = j / cc, c = j - f * cc;
        art_s *const p = g + (size_t) f * C + c;
        if (TO_LDS) lds [c * lp + f] = *p; else *p = lds [c * lp + f];
    }
}

// TO_PLANAR: interleaved frames -> planes; otherwise planes -> interleaved frames
template <bool TO_PLANAR>
__global__ __launch_bounds__ (LAYOUT_THREADS)
void transpose_group_kernel (const ArtLayoutItem *items, int n)
{
    __shared__ __attribute__ ((aligned (16))) art_s lds [LAYOUT_LDS];
    const long task = blockIdx.x;
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items [mid].task0 <= task) lo = mid; else hi = mid - 1; }
    const ArtLayoutItem &it = items [lo];
    const int C = it.C, tile = it.tile;
    const long f0 = (task - it.task0) * tile;
    if (f0 >= it.count) return;
    const int nf = it.count - f0 < tile ? (int)(it.count - f0) : tile;
    art_s *const frames = it.frames + (size_t) f0 * C;

    for (int c0 = 0; c0 < C; c0 += LAYOUT_CH) {
        const int cc = C - c0 < LAYOUT_CH ? C - c0 : LAYOUT_CH;
        const int lp = layout_pitch (tile, cc);
        art_s *const planes = it.planes + (size_t) c0 * it.pitch + f0;
        if (c0) __syncthreads ();                          // (the chunk before has left the LDS)
        if (!TO_PLANAR) pass_planes<true> (lds, lp, planes, it.pitch, nf, cc);
        else if (cc == C) pass_frames<true> (lds, lp, frames, nf, C);
        else pass_rows<true> (lds, lp, frames + c0, nf, cc, C);
        __syncthreads ();
        if (TO_PLANAR) pass_planes<false> (lds, lp, planes, it.pitch, nf, cc);
        else if (cc == C) pass_frames<false> (lds, lp, frames, nf, C);
        else pass_rows<false> (lds, lp, frames + c0, nf, cc, C);
    }
}

// Many runs of device memory cleared in one launch (resampleProcessAndFlushClipsPlanarDevice: both history buffers of every context of a
// batch, where resampleReset issues two memsets per context).  A task is one 16-byte group counted from the boundary before its run:
// whole aligned stores inside the run, single words at its ends; nothing outside [ptr, ptr + words) is written.
__global__ __launch_bounds__ (256)
void zero_runs_group_kernel (const ArtZeroRun *items, int n, long tasks)
{
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= tasks) return;
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items [mid].task0 <= task) lo = mid; else hi = mid - 1; }
    const ArtZeroRun &it = items [lo];
    const long w0 = (task - it.task0) * 4 - (long)(((uintptr_t) it.ptr >> 2) & 3), words = it.words;
    if (w0 >= 0 && w0 + 4 <= words) { *reinterpret_cast<uint4 *> (it.ptr + w0) = make_uint4 (0u, 0u, 0u, 0u); return; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (w0 + j >= 0 && w0 + j < words) it.ptr [w0 + j] = 0u;
}

} // namespace

extern "C" {

// items [k].task0 is filled here; d_table: device memory of n items (stream order protects it)
int arthip_zero_runs (ArtZeroRun *items, int n, void *d_table, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    long tasks = 0;
    for (int k = 0; k < n; ++k) {
        items [k].task0 = tasks;
        if (items [k].words > 0) tasks += (items [k].words + 3) / 4 + 1;
    }
    if (n <= 0 || tasks <= 0) return 0;
    if (arthip_table_upload (items, sizeof (ArtZeroRun) * (size_t) n, d_table, stream)) return -1;
    hipLaunchKernelGGL (zero_runs_group_kernel, dim3 ((unsigned int)((tasks + 255) / 256)), dim3 (256), 0, st, (const ArtZeroRun *) d_table, n, tasks);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

// items [k].tile and .task0 are filled here; d_table: device memory of n items (reused call after call: stream order protects it)
int arthip_transpose_group (ArtLayoutItem *items, int n, int to_planar, void *d_table, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    long tasks = 0;
    for (int k = 0; k < n; ++k) {
        items [k].tile = layout_tile (items [k].C);
        items [k].task0 = tasks;
        if (items [k].count > 0) tasks += (items [k].count + items [k].tile - 1) / items [k].tile;
    }
    if (n <= 0 || tasks <= 0) return 0;
    if (tasks > 0x7fffffffL) return -1;
    const size_t bytes = sizeof (ArtLayoutItem) * (size_t) n;
    Staging *sg = staging_take (bytes);
    if (!sg) return -1;
    std::memcpy (sg->host, items, bytes);
    if (hipMemcpyAsync (d_table, sg->host, bytes, hipMemcpyHostToDevice, st) != hipSuccess) { (void) staging_give (sg, st); return -1; }
    if (to_planar) hipLaunchKernelGGL (transpose_group_kernel<true>, dim3 ((unsigned int) tasks), dim3 (LAYOUT_THREADS), 0, st, (const ArtLayoutItem *) d_table, n);
    else hipLaunchKernelGGL (transpose_group_kernel<false>, dim3 ((unsigned int) tasks), dim3 (LAYOUT_THREADS), 0, st, (const ArtLayoutItem *) d_table, n);
    const bool ok = hipGetLastError () == hipSuccess;
    return staging_give (sg, st) || !ok ? -1 : 0;
}

}
