// pcm_kernels.hip — gfx950 kernels for the serial-recurrence parts of the path:
//   biquad section chains      reference biquad.c:106-163 (apply_buffer), :78-102 (apply_sample)
//   float -> integer decimator reference decimator.c:255-283, dither :370-382
//   integer -> float ingest    reference decimator.c:416-450
//
// Both recurrences feed each output back through float rounding (and, in the decimator, through
// floor()), so they cannot be re-associated or scanned in parallel without changing bits.  The
// bit-exact GPU form is one lane per channel walking time serially; channels run side by side in a
// wave.  Compiled with -ffp-contract=off: every multiply and add rounds separately, as in the
// reference.
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdlib>
#include <type_traits>
#include "art_internal.h"

namespace {

struct SectionRegs {
    art_s a [5], b [5];
    art_s x [4], y [4];       // x[0] = most recent input, x[1] the one before, ...
    int order;
};

__device__ __forceinline__ void load_section (SectionRegs &r, const Biquad &f)
{
    const int i = f.index;
#pragma unroll
    for (int k = 0; k < 5; ++k) { r.a [k] = f.a [k]; r.b [k] = f.b [k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { r.x [k] = f.x [(i - k) & 3]; r.y [k] = f.y [(i - k) & 3]; }
    r.order = f.order;
}

__device__ __forceinline__ void store_section (Biquad &f, const SectionRegs &r, int steps, bool mask_index)
{
    int i = f.index;
    if (mask_index) i &= 3;
    i += steps;
    if (mask_index) i &= 3;
#pragma unroll
    for (int k = 0; k < 4; ++k) { f.x [(i - k) & 3] = r.x [k]; f.y [(i - k) & 3] = r.y [k]; }
    f.index = i;
}

__device__ __forceinline__ void push (SectionRegs &r, art_s in, art_s out)
{
    r.x [3] = r.x [2]; r.x [2] = r.x [1]; r.x [1] = r.x [0]; r.x [0] = in;
    r.y [3] = r.y [2]; r.y [2] = r.y [1]; r.y [1] = r.y [0]; r.y [0] = out;
}

// buffer form: in*a0, then for k = 1..order: + x_k*a_k, - b_k*y_k, strictly left to right
__device__ __forceinline__ art_s step_buffer_order (SectionRegs &r, art_s in)
{
    art_s acc = in * r.a [0];
#pragma unroll
    for (int k = 1; k <= 4; ++k)
        if (k <= r.order) {
            art_s fwd = r.x [k - 1] * r.a [k];
            acc = acc + fwd;
            art_s back = r.b [k] * r.y [k - 1];
            acc = acc - back;
        }
    push (r, in, acc);
    return acc;
}

// per-sample form: in*a0, then for k = order..1: += (x_k*a_k - b_k*y_k)
__device__ __forceinline__ art_s step_sample_order (SectionRegs &r, art_s in)
{
    art_s acc = in * r.a [0];
#pragma unroll
    for (int k = 4; k >= 1; --k)
        if (k <= r.order) {
            art_s fwd = r.x [k - 1] * r.a [k];
            art_s back = r.b [k] * r.y [k - 1];
            art_s term = fwd - back;
            acc = acc + term;
        }
    push (r, in, acc);
    return acc;
}

constexpr int MAX_CHAIN = 4;

__global__ void biquad_chain_kernel (Biquad *sections, int C, int S, art_s *buf, int frames, int stride, int sample_form)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;

    SectionRegs r [MAX_CHAIN];
#pragma unroll
    for (int s = 0; s < MAX_CHAIN; ++s)
        if (s < S) load_section (r [s], sections [(size_t) c * S + s]);

    art_s *p = buf + c;
    for (int i = 0; i < frames; ++i, p += stride) {
        art_s v = *p;
#pragma unroll
        for (int s = 0; s < MAX_CHAIN; ++s)
            if (s < S) v = sample_form ? step_sample_order (r [s], v) : step_buffer_order (r [s], v);
        *p = v;
    }

#pragma unroll
    for (int s = 0; s < MAX_CHAIN; ++s)
        if (s < S) store_section (sections [(size_t) c * S + s], r [s], frames, sample_form != 0);
}

// ---------------------------------------------------------------------------------------------------
// Bit-exact biquad cascade, parallel over TIME (biquad_spec_kernel + biquad_commit_kernel).
//
// The recurrence rounds after every operation (reference biquad.c:138-146), so it cannot be re-associated; but a
// STABLE filter forgets its state: two runs over the same input that start from different states converge
// geometrically, and once their rounded states coincide at one sample they coincide for ever.  So every chunk of L
// frames is computed by its own lane in the reference's exact operation order, started WARM-UP frames early from a
// zero state (section s starts (S - s) W frames early, so that it is fed converged outputs of section s - 1), and
// records the state it reached at its chunk's first frame and the state it left at its last.  Chunk 0 starts from the
// carried-in state and is exact; chunk k is exact iff chunk k - 1 is exact and the state chunk k reached after its
// warm-up equals, bit for bit, the state chunk k - 1 left.  The commit kernel checks every boundary in parallel; in the
// (rare) case of a mismatch one lane recomputes from the exact state until it rejoins a speculative trajectory — in the
// worst case everything, serially, so the result is exact whatever the filter.  W comes from the decay of the
// recursive part (host side); filters too narrow to forget within the cap take the serial kernels instead.
// Input and output are separate buffers (a chunk's warm-up reads frames its predecessor writes).
// ---------------------------------------------------------------------------------------------------
struct SpecState { art_s x [4], y [4]; };           // one section's delay lines, newest first

template <int S>
__device__ __forceinline__ bool same_state (const SpecState *a, const SpecState *b)
{
    bool same = true;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // bit patterns, not values: -0.0 and 0.0 carry on differently through a multiply by a negative coefficient
            same = same && __builtin_bit_cast (typename std::conditional<sizeof (art_s) == 4, uint32_t, uint64_t>::type, a [s].x [k]) ==
                           __builtin_bit_cast (typename std::conditional<sizeof (art_s) == 4, uint32_t, uint64_t>::type, b [s].x [k]);
            same = same && __builtin_bit_cast (typename std::conditional<sizeof (art_s) == 4, uint32_t, uint64_t>::type, a [s].y [k]) ==
                           __builtin_bit_cast (typename std::conditional<sizeof (art_s) == 4, uint32_t, uint64_t>::type, b [s].y [k]);
        }
    return same;
}

template <int S>
__device__ __forceinline__ void get_state (SpecState *dst, const SectionRegs *r)
{
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) { dst [s].x [k] = r [s].x [k]; dst [s].y [k] = r [s].y [k]; }
}

template <int S>
__device__ __forceinline__ void put_state (SectionRegs *r, const SpecState *src)
{
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) { r [s].x [k] = src [s].x [k]; r [s].y [k] = src [s].y [k]; }
}

// PLANAR instantiations take pitches (samples between planes) where the interleaved ones take strides
template <bool PLANAR> using spec_stride = typename std::conditional<PLANAR, long, int>::type;

// A run over a plane, the one copy for every time-parallel kernel: the addresses [lo, hi) of `in` (and `out`) taken upwards from
// lo, or REV: DOWNWARDS from hi - 1.  The run is cut at the 16-byte boundaries of its own address: single frames up (down) to the
// first boundary, batches of U frames by 16-byte loads from there (two batches in flight, as below), single frames behind the last
// whole batch.  Stores are 16 bytes too where `out` is aligned as `in` is.  Within a batch the frames are taken in the run's
// direction; the arithmetic is the interleaved form's, frame by frame in the same order.
template <int ACTIVE, bool STORE, bool REV = false>
__device__ __forceinline__ void run_plane (SectionRegs *r, const art_s *in, art_s *out, int lo, int hi)
{
    constexpr int U = 8, Q = 16 / (int) sizeof (art_s);                   // Q frames to 16 bytes
    typedef art_s vecq __attribute__ ((ext_vector_type (Q)));
    auto one = [&] (int a) {
        art_s v = in [a];
#pragma unroll
        for (int s = 0; s < ACTIVE; ++s) v = step_buffer_order (r [s], v);
        if constexpr (STORE) out [a] = v;
    };
    auto past = [&] (int a) { return (int)(((uintptr_t)(in + a) / sizeof (art_s)) & (Q - 1)); };        // samples of in + a beyond a boundary
    int n = REV ? hi : lo;                                                // done: everything below n, REV: everything from n up
    const int head = min (hi - lo, REV ? past (hi) : (Q - past (lo)) & (Q - 1));
    if constexpr (REV) for (const int e = n - head; n > e; ) { --n; one (n); }
    else for (const int e = n + head; n < e; ++n) one (n);
    bool whole = false;                                                   // (in + n is on a boundary now, or the run is over)
    if constexpr (STORE) whole = !((uintptr_t)(out + n) & 15);
    auto fetch = [&] (art_s (&v) [U], int at) {                           // the U frames from address `at` up
#pragma unroll
        for (int q = 0; q < U / Q; ++q) {
            const vecq t = *reinterpret_cast<const vecq *> (in + at + q * Q);
#pragma unroll
            for (int j = 0; j < Q; ++j) v [q * Q + j] = t [j];
        }
    };
    auto work = [&] (art_s (&v) [U], int at) {
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int u = REV ? U - 1 - i : i;
#pragma unroll
            for (int s = 0; s < ACTIVE; ++s) v [u] = step_buffer_order (r [s], v [u]);
        }
        if constexpr (STORE) {
            if (whole) {
#pragma unroll
                for (int q = 0; q < U / Q; ++q) {
                    vecq t;
#pragma unroll
                    for (int j = 0; j < Q; ++j) t [j] = v [q * Q + j];
                    *reinterpret_cast<vecq *> (out + at + q * Q) = t;
                }
            }
            else {
#pragma unroll
                for (int u = 0; u < U; ++u) out [at + u] = v [u];
            }
        }
    };
    constexpr int STEP = REV ? -U : U, LOW = REV ? -U : 0;                // a batch at n: the addresses from n + LOW up
    const int batches = (REV ? n - lo : hi - n) / U;
    if (batches > 0) {
        art_s cur [U], nxt [U];
        fetch (cur, n + LOW);
        for (int b = 0; b < batches; ++b, n += STEP) {
            const bool more = b + 1 < batches;
            if (more) fetch (nxt, n + STEP + LOW);         // in flight while this batch's dependent chain runs
            work (cur, n + LOW);
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) cur [u] = nxt [u];
            }
        }
    }
    if constexpr (REV) while (n > lo) { --n; one (n); }
    else for (; n < hi; ++n) one (n);
}

// frames [from, to) of channel c through sections 0 .. ACTIVE-1, exact order; STORE: the results go to `out`.  The one forward run
// of every time-parallel kernel, single or gathered.
// The recurrence is latency-bound and a lane's loads are independent of it: two batches of U frames are kept in flight
// (the next batch's loads are issued before the current batch's dependent chain starts).
template <int S, int ACTIVE, bool STORE, bool PLANAR = false>
__device__ __forceinline__ void spec_run (SectionRegs *r, const art_s *in, spec_stride<PLANAR> stride, art_s *out, spec_stride<PLANAR> out_stride,
                                          int c, int from, int to)
{
    if constexpr (PLANAR) {
        run_plane<ACTIVE, STORE> (r, in + (size_t) c * stride, STORE ? out + (size_t) c * out_stride : nullptr, from, to);
        return;
    }
    else {
    constexpr int U = 8;
    auto fetch = [&] (art_s (&v) [U], int n) {
#pragma unroll
        for (int u = 0; u < U; ++u) v [u] = in [(size_t)(n + u) * stride + c];
    };
    auto work = [&] (art_s (&v) [U], int n) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int s = 0; s < ACTIVE; ++s) v [u] = step_buffer_order (r [s], v [u]);
        }
        if (STORE) {
#pragma unroll
            for (int u = 0; u < U; ++u) out [(size_t)(n + u) * out_stride + c] = v [u];
        }
    };
    int n = from;
    const int batches = (to - from) / U;
    if (batches > 0) {
        art_s cur [U], nxt [U];
        fetch (cur, n);
        for (int b = 0; b < batches; ++b, n += U) {
            const bool more = b + 1 < batches;
            if (more) fetch (nxt, n + U);                  // in flight while this batch's dependent chain runs
            work (cur, n);
            if (more) {
#pragma unroll
                for (int u = 0; u < U; ++u) cur [u] = nxt [u];
            }
        }
    }
    for (; n < to; ++n) {
        art_s v = in [(size_t) n * stride + c];
#pragma unroll
        for (int s = 0; s < ACTIVE; ++s) v = step_buffer_order (r [s], v);
        if (STORE) out [(size_t) n * out_stride + c] = v;
    }
    }
}

// spec_run with a direction, for the gathered kernels: frames [from, to) of the recurrence of channel c of a call of `frames` frames.
// Forwards it IS spec_run, and a reversed plane is run_plane downwards.  The reversed INTERLEAVED run is a COPY of spec_run's
// interleaved branch, frame n at row frames - 1 - n: a change to one goes into the other.  With REV as a parameter of spec_run
// itself (three formulations of the row: frames - 1 - n, top - n - u, a pointer walked down) the single kernels kept their
// instructions, but the reversed interleaved kernels of four sections needed more registers: 4-byte bq_filter_commit_kernel<4,
// false, true> 162 -> 169 VGPRs, 8-byte 225 -> 258 with 2 AGPRs, 8-byte bq_filter_spec_kernel<4, false, true> 250 -> 262 with 6
// AGPRs (profiles/biquad_one_body.txt).
template <int S, int ACTIVE, bool STORE, bool PLANAR, bool REV>
__device__ __forceinline__ void dir_run (SectionRegs *r, const art_s *in, spec_stride<PLANAR> stride, art_s *out, spec_stride<PLANAR> out_stride,
                                         int c, int from, int to, int frames)
{
    if constexpr (!REV) spec_run<S, ACTIVE, STORE, PLANAR> (r, in, stride, out, out_stride, c, from, to);
    else if constexpr (PLANAR)
        run_plane<ACTIVE, STORE, true> (r, in + (size_t) c * stride, STORE ? out + (size_t) c * out_stride : nullptr, frames - to, frames - from);
    else {
        // the interleaved form of spec_run, frame n at row frames - 1 - n
        constexpr int U = 8;
        const int top = frames - 1;
        auto fetch = [&] (art_s (&v) [U], int n) {
#pragma unroll
            for (int u = 0; u < U; ++u) v [u] = in [(size_t)(top - n - u) * stride + c];
        };
        auto work = [&] (art_s (&v) [U], int n) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int s = 0; s < ACTIVE; ++s) v [u] = step_buffer_order (r [s], v [u]);
            }
            if (STORE) {
#pragma unroll
                for (int u = 0; u < U; ++u) out [(size_t)(top - n - u) * out_stride + c] = v [u];
            }
        };
        int n = from;
        const int batches = (to - from) / U;
        if (batches > 0) {
            art_s cur [U], nxt [U];
            fetch (cur, n);
            for (int b = 0; b < batches; ++b, n += U) {
                const bool more = b + 1 < batches;
                if (more) fetch (nxt, n + U);              // in flight while this batch's dependent chain runs
                work (cur, n);
                if (more) {
#pragma unroll
                    for (int u = 0; u < U; ++u) cur [u] = nxt [u];
                }
            }
        }
        for (; n < to; ++n) {
            art_s v = in [(size_t)(top - n) * stride + c];
#pragma unroll
            for (int s = 0; s < ACTIVE; ++s) v = step_buffer_order (r [s], v);
            if (STORE) out [(size_t)(top - n) * out_stride + c] = v;
        }
    }
}

// the warm-up of a speculative chunk: W frames with section 0 alone, W more with sections 0-1, ... (section s joins (S - s) W
// frames before the chunk's first frame, fed by sections that have already converged)
template <int S, bool PLANAR, bool REV = false, int J = 0>
__device__ __forceinline__ void spec_warm_up (SectionRegs *r, const art_s *in, spec_stride<PLANAR> stride, int c, int begin, int W, int frames = 0)
{
    if constexpr (J < S) {
        dir_run<S, J + 1, false, PLANAR, REV> (r, in, stride, nullptr, 0, c, begin + J * W, begin + (J + 1) * W, frames);
        spec_warm_up<S, PLANAR, REV, J + 1> (r, in, stride, c, begin, W, frames);
    }
}

// task = (chunk k, channel c), c fastest: the lanes of a wave read neighbouring channels of a few chunks.  PLANAR: k fastest —
// consecutive lanes walk consecutive chunks of ONE plane, so a wave touches one contiguous stretch of it.
template <int S, bool PLANAR = false>
__global__ __launch_bounds__ (256)
void biquad_spec_kernel (const Biquad *sections, int C, int K, int L, int W, const art_s *in, spec_stride<PLANAR> stride, art_s *out,
                         spec_stride<PLANAR> out_stride, int frames, SpecState *starts, SpecState *ends)
{
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= (long) C * K) return;
    const int c = PLANAR ? (int)(task / K) : (int)(task % C), k = PLANAR ? (int)(task % K) : (int)(task / C);
    const int first = k * L, last = min (first + L, frames);

    SectionRegs r [S];
#pragma unroll
    for (int s = 0; s < S; ++s) load_section (r [s], sections [(size_t) c * S + s]);

    const int begin = first - S * W;
    if (begin > 0) {
        // speculative start: silence behind every section
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) { r [s].x [q] = 0; r [s].y [q] = 0; }
        spec_warm_up<S, PLANAR> (r, in, stride, c, begin, W);
    }
    else if (first > 0)
        // close to the start of the call: from the carried-in state through frames [0, first) — exact, nothing stored
        spec_run<S, S, false, PLANAR> (r, in, stride, nullptr, 0, c, 0, first);

    SpecState st [S];
    get_state<S> (st, r);
#pragma unroll
    for (int s = 0; s < S; ++s) starts [((size_t) c * K + k) * S + s] = st [s];

    spec_run<S, S, true, PLANAR> (r, in, stride, out, out_stride, c, first, last);

    get_state<S> (st, r);
#pragma unroll
    for (int s = 0; s < S; ++s) ends [((size_t) c * K + k) * S + s] = st [s];
}

// Every chunk boundary checked, one thread each: flags [c][k] = chunk k did not start from the state chunk k-1 left;
// first_bad [c] = the first such k of the channel (stays at its armed value, beyond any chunk count, when there is none).
template <int S>
__global__ __launch_bounds__ (256)
void biquad_check_kernel (int C, int K, const SpecState *starts, const SpecState *ends, unsigned char *bad, int *first_bad)
{
    const long t = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long) C * K) return;
    const int c = (int)(t / K), k = (int)(t % K);
    if (k == 0) return;
    const bool ok = same_state<S> (starts + ((size_t) c * K + k) * S, ends + ((size_t) c * K + k - 1) * S);
    bad [(size_t) c * K + k] = ok ? 0 : 1;
    if (!ok) atomicMin (first_bad + c, k);
}

// One thread per channel: repairs from the first mismatch (rare: recomputes from the exact state until it rejoins a
// speculative trajectory — in the worst case everything, serially), then the channel's final state goes back into
// `sections`.  repairs: running count of chunks recomputed (diagnostics).  first_bad is re-armed for the next call.
template <int S, bool PLANAR = false>
__global__ __launch_bounds__ (64)
void biquad_commit_kernel (Biquad *sections, int C, int K, int L, const art_s *in, spec_stride<PLANAR> stride, art_s *out,
                           spec_stride<PLANAR> out_stride, int frames,
                           const SpecState *starts, SpecState *ends, const unsigned char *bad, int *first_bad, unsigned int *repairs)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const SpecState *st = starts + (size_t) c * K * S;
    SpecState *en = ends + (size_t) c * K * S;
    const unsigned char *flags = bad + (size_t) c * K;

    SectionRegs r [S];
#pragma unroll
    for (int s = 0; s < S; ++s) load_section (r [s], sections [(size_t) c * S + s]);

    int k = first_bad [c];
    first_bad [c] = INT_MAX;
    unsigned int redone = 0;
    while (k < K) {
        // chunk k again, from the exact state its predecessor left
        put_state<S> (r, en + (size_t)(k - 1) * S);
        const int first = k * L, last = min (first + L, frames);
        spec_run<S, S, true, PLANAR> (r, in, stride, out, out_stride, c, first, last);
        SpecState now [S];
        get_state<S> (now, r);
#pragma unroll
        for (int s = 0; s < S; ++s) en [(size_t) k * S + s] = now [s];
        ++redone;
        if (k + 1 >= K) break;
        if (same_state<S> (now, st + (size_t)(k + 1) * S)) {
            // rejoined the speculative trajectory: everything up to the next recorded mismatch stands
            int next = k + 2;
            while (next < K && !flags [next]) ++next;
            k = next;
        }
        else ++k;
    }
    if (redone) atomicAdd (repairs, redone);

    put_state<S> (r, en + (size_t)(K - 1) * S);
#pragma unroll
    for (int s = 0; s < S; ++s) store_section (sections [(size_t) c * S + s], r [s], frames, false);
}

__device__ __forceinline__ uint32_t lcg (uint32_t r) { return ((r << 4) - r) ^ 1u; }

// One draw of the TPDF dither (reference decimator.c:370-382): five generator steps, and u = (first >> 1) + (r >> 1); the dither
// is u / 2^31 - 1.0.
__device__ __forceinline__ uint32_t tpdf_step (uint32_t &g, int dither_type)
{
    const uint32_t start = g;
    uint32_t r = lcg (lcg (start));
    const uint32_t first = dither_type < 0 ? ~start : dither_type > 0 ? start : ~r;
    r = lcg (lcg (lcg (r)));
    g = r;
    return (first >> 1) + (r >> 1);
}

// u / 2^31 - 1.0, converted to the sample type, is exactly this (power-of-two scale)
__device__ __forceinline__ art_s tpdf_value (uint32_t u) { return (art_s)(int)(u ^ 0x80000000u) * (art_s) 4.656612873077392578125e-10; }

// ---------------------------------------------------------------------------------------------------
// The output format, once for every decimator kernel (reference decimator.c:266-283): a code value is clipped to the format's range,
// shifted up to whole bytes (8-bit codes are offset binary: + 128), and leaves as `pad` zero bytes and then its `width` value bytes,
// least significant first.  Every kernel but decimate_kernel builds a DecFmt once, clips with DEC_CLIP and stores with DEC_STORE_BYTES (interleaved
// bytes, one at a time) or packs dec_word (planar bytes, in whole units).
// DEC_FMT, DEC_CLIP and DEC_STORE_BYTES are TEXT, not functions: as __forceinline__ functions (the clip returning bool, or taking the
// count as a callable; the format returned by value) each moved the register rows of the interleaved serial kernels, which must
// stay the parent's (profiles/pcm_shared_parts.txt has the table of every form tried).
// ---------------------------------------------------------------------------------------------------
struct DecFmt { int nbytes, width, pad, hi, lo, shift; uint32_t bias; };
// the fields of a DecFmt in order: nbytes, width, pad, hi, lo, shift, bias
#define DEC_FMT(bits, bytes) { (bytes), ((bits) + 7) / 8, (bytes) - ((bits) + 7) / 8, (1 << ((bits) - 1)) - 1, ~((1 << ((bits) - 1)) - 1), (24 - (bits)) % 8, (bits) <= 8 ? 128u : 0u }
__device__ __forceinline__ DecFmt dec_fmt (int bits, int bytes) { const DecFmt f = DEC_FMT (bits, bytes); return f; }
// q into the format's range; COUNT is the statement that counts a clip (a register, or the batch's LDS counter per lane)
#define DEC_CLIP(fm, q, COUNT) do { if ((q) > (fm).hi) { (q) = (fm).hi; COUNT; } else if ((q) < (fm).lo) { (q) = (fm).lo; COUNT; } } while (0)
__device__ __forceinline__ uint32_t dec_value (const DecFmt &f, int q) { return ((uint32_t) q << f.shift) + f.bias; }
// a clipped code value's nbytes output bytes at `at`, byte by byte (an interleaved sample has no alignment to speak of)
#define DEC_STORE_BYTES(at, fm, q) do { const uint32_t v_ = ((uint32_t)(q) << (fm).shift) + (fm).bias; unsigned char *o_ = (at); \
        for (int j_ = 0; j_ < (fm).pad; ++j_) *o_++ = 0; \
        *o_++ = (unsigned char) v_; \
        if ((fm).width > 1) { *o_++ = (unsigned char)(v_ >> 8); if ((fm).width > 2) *o_++ = (unsigned char)(v_ >> 16); } } while (0)
// ... and the same bytes as one little-endian word (the planar sides' packers)
__device__ __forceinline__ uint32_t dec_word (const DecFmt &f, int q)
{
    return (dec_value (f, q) & (0xffffffffu >> (32 - 8 * f.width))) << (8 * f.pad);
}

// the one-lane form: calls under 64 frames, and the host-pointer planar call.  Its dither and rounding are written as the reference
// writes them (through double), where the chunked kernels below use tpdf_value and round_half_up.  Its clip and store are written out
// too, NOT through DEC_CLIP / DEC_STORE_BYTES: with them its registers were the same and its code two scalar instructions other, and
// 63-frame calls measured 2-4 % slower in two alternating runs (profiles/pcm_shared_parts.txt), so by the rule of that change it stays.
__global__ void decimate_kernel (ArtDecArgs a, const art_s *in, long in_pitch, int frames, unsigned char *out, long out_pitch)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C) return;

    art_s fb = a.feedback [c];
    uint32_t gen = a.dither_on ? a.gens [c] : 0u;
    SectionRegs sh;
    if (a.shaping_on) load_section (sh, a.shapers [c]);

    const int pad = a.bytes - ((a.bits + 7) / 8);
    const int hi = (1 << (a.bits - 1)) - 1, lo = ~hi;
    const int shift = (24 - a.bits) % 8;
    const uint32_t bias = a.bits <= 8 ? 128u : 0u;
    unsigned long long clips = 0;

    for (int i = 0; i < frames; ++i) {
        const art_s s = in_pitch ? in [(size_t) c * in_pitch + i] : in [(size_t) i * a.C + c];
        art_s dither = 0.0f;

        if (a.dither_on) {
            const double tri = ((double) tpdf_step (gen, a.dither_type) / 2147483648.0) - 1.0;     // the reference's order
            dither = (art_s) tri;
        }

        const art_s scaled = s * a.scale;
        const art_s code = scaled - fb;
        const art_s dithered = code + dither;
        int q = (int) floor ((double) dithered + 0.5);

        if (a.shaping_on) {
            const art_s err = (art_s) q - code;
            fb = step_sample_order (sh, err);
        }

        if (q > hi) { q = hi; clips++; }
        else if (q < lo) { q = lo; clips++; }

        const uint32_t v = ((uint32_t) q << shift) + bias;
        unsigned char *o = out_pitch ? out + (size_t) c * out_pitch + (size_t) i * a.bytes
                                     : out + ((size_t) i * a.C + c) * a.bytes;
        for (int j = 0; j < pad; ++j) *o++ = 0;
        *o++ = (unsigned char) v;
        if (a.bits > 8) { *o++ = (unsigned char)(v >> 8); if (a.bits > 16) *o++ = (unsigned char)(v >> 16); }
    }

    a.feedback [c] = fb;
    if (a.dither_on) a.gens [c] = gen;
    if (a.shaping_on) store_section (a.shapers [c], sh, frames, true);
    if (clips) atomicAdd (a.clipped, clips);
}


// ---------------------------------------------------------------------------------------------------
// LDS-staged forms (interleaved frames, stride == channel count).  The recurrences stay one lane per
// channel — that is what bit-exactness costs — but memory traffic is taken off the serial path: the whole
// workgroup moves a chunk of frames HBM <-> LDS with coalesced 16-byte accesses, then lanes 0..Cg-1 of
// wave 0 run the chunk out of LDS (inputs are known ahead of the recurrence, so the LDS reads pipeline).
// Algorithmic HBM bytes per sample: biquad 8 (in-place), decimator 4 + output bytes.
// ---------------------------------------------------------------------------------------------------
constexpr int ST_THREADS = 256;
constexpr int ST_CHUNK_FLOATS = ART_WIDE ? 4096 : 8192;   // 32 KiB of samples per chunk

__global__ __launch_bounds__ (ST_THREADS)
void biquad_chain_lds_kernel (Biquad *sections, int C, int S, art_s *buf, int frames)
{
    __shared__ __attribute__ ((aligned (16))) art_s tile [ST_CHUNK_FLOATS];
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * 64, Cg = min (64, C - c0);          // this block's channel group
    const int chunk_frames = ST_CHUNK_FLOATS / Cg;

    SectionRegs r [MAX_CHAIN];
    if (tid < Cg) {
#pragma unroll
        for (int s = 0; s < MAX_CHAIN; ++s)
            if (s < S) load_section (r [s], sections [(size_t)(c0 + tid) * S + s]);
    }

    for (int f0 = 0; f0 < frames; f0 += chunk_frames) {
        const int nf = min (chunk_frames, frames - f0);
        // HBM -> LDS (coalesced when the group is the whole frame)
        for (int e = tid; e < nf * Cg; e += ST_THREADS) {
            const int f = e / Cg, c = e - f * Cg;
            tile [e] = buf [(size_t)(f0 + f) * C + c0 + c];
        }
        __syncthreads ();
        if (tid < Cg) {
            art_s *p = tile + tid;
            for (int f = 0; f < nf; ++f, p += Cg) {
                art_s v = *p;
#pragma unroll
                for (int s = 0; s < MAX_CHAIN; ++s)
                    if (s < S) v = step_buffer_order (r [s], v);
                *p = v;
            }
        }
        __syncthreads ();
        for (int e = tid; e < nf * Cg; e += ST_THREADS) {
            const int f = e / Cg, c = e - f * Cg;
            buf [(size_t)(f0 + f) * C + c0 + c] = tile [e];
        }
        __syncthreads ();
    }

    if (tid < Cg) {
#pragma unroll
        for (int s = 0; s < MAX_CHAIN; ++s)
            if (s < S) store_section (sections [(size_t)(c0 + tid) * S + s], r [s], frames, false);
    }
}


// ---- order-2 cascade, feed-forward split + section pipeline -----------------------------------------
// A lone wave issues one instruction every ~4 cycles whatever the number of active lanes, so with 8 channels
// the serial lanes are issue- and latency-bound: what counts is instructions (and dependent operations) per
// sample in the recurrence.  Of the nine operations of a section only five depend on earlier outputs; the rest is
// feed-forward and is done for a whole chunk at once by helper waves (same operations, same order, same
// roundings):
//
//     helpers       u[n]  = (x[n]*a0) + (x[n-1]*a1)          p[n] = x[n-2]*a2
//     serial lane   y[n]  = ((u[n] - (b1*y[n-1])) + p[n]) - (b2*y[n-2])
//
// u/p/y live in LDS per channel (time-contiguous: one ds_read_b128 feeds four samples, fetched one block of
// eight samples ahead of the recurrence; row pitch = 4 mod 32 words keeps the channels of a wave on different
// banks).  The workgroup is a four-stage pipeline over chunks, one barrier per step `it`, all stages of a step
// running concurrently on different waves (different SIMDs of the CU):
//
//     wave 2      feed-forward 1 of chunk it+1 (inputs fetched from HBM one step earlier) | fetch chunk it+2
//     wave 3      store chunk it-3 | feed-forward 2 of chunk it-1
//     wave 0      section 1 of chunk it
//     wave 1      section 2 of chunk it-2
//
// The first chunk takes the remainder, every later chunk has the same length (a multiple of 4).
constexpr int FF_CAP = ART_WIDE ? 1536 : 3072;      // samples per LDS array (12 KiB); 9 arrays
constexpr int FF_HELPERS = 64;                     // threads per helper role (one wave each)
constexpr int FF_RUN = 48;                         // frames per helper lane and chunk (upper bound)
constexpr int FF_GROUP = 16;                       // frames wave 3 holds in registers at a time (divides FF_RUN)

// Raw buffer accesses with hardware bounds checking (word 3 = 0x00020000: raw, 32-bit): an out-of-range load
// returns 0 and an out-of-range store is dropped, so the helper loops carry no per-element predicates.
typedef unsigned int ffu2 __attribute__ ((ext_vector_type (2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t ff_rsrc (const void *base, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc (const_cast<void *> (base), 0, (int) (bytes > 0x7fffffffu ? 0x7fffffffu : bytes), 0x00020000);
}
__attribute__ ((unused)) __device__ __forceinline__ float ff_load (__amdgpu_buffer_rsrc_t r, int off, float) { return __uint_as_float (__builtin_amdgcn_raw_buffer_load_b32 (r, off, 0, 0)); }
__attribute__ ((unused)) __device__ __forceinline__ double ff_load (__amdgpu_buffer_rsrc_t r, int off, double)
{
    const ffu2 v = __builtin_amdgcn_raw_buffer_load_b64 (r, off, 0, 0);
    return __hiloint2double ((int) v.y, (int) v.x);
}
__attribute__ ((unused)) __device__ __forceinline__ void ff_store (__amdgpu_buffer_rsrc_t r, int off, float v) { __builtin_amdgcn_raw_buffer_store_b32 (__float_as_uint (v), r, off, 0, 0); }
__attribute__ ((unused)) __device__ __forceinline__ void ff_store (__amdgpu_buffer_rsrc_t r, int off, double v)
{
    ffu2 w; w.x = (unsigned int) __double2loint (v); w.y = (unsigned int) __double2hiint (v);
    __builtin_amdgcn_raw_buffer_store_b64 (w, r, off, 0, 0);
}

__device__ __forceinline__ void ff_serial (art_s *row, const art_s *prow, int len, art_s b1, art_s b2, art_s &y1, art_s &y2)
{
    typedef art_s vec4 __attribute__ ((ext_vector_type (4)));
    auto four = [&] (const vec4 u, const vec4 p) -> vec4 {
        vec4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const art_s m = b1 * y1;
            const art_s t2 = u [j] - m;
            const art_s t3 = t2 + p [j];
            const art_s q = b2 * y2;
            const art_s v = t3 - q;
            y [j] = v; y2 = y1; y1 = v;
        }
        return y;
    };
    // blocks of eight samples, two register sets: the reads of the next block are issued before the recurrence of
    // the current one starts (sched_barrier keeps the compiler from sinking them), so LDS latency never sits on
    // the serial path.  The look-ahead may read up to one block past `len` (inside the LDS allocation, unused).
    const int nblk = len >> 3;
    if (nblk > 0) {
        vec4 ua0 = *(const vec4 *)(row), ua1 = *(const vec4 *)(row + 4), pa0 = *(const vec4 *)(prow), pa1 = *(const vec4 *)(prow + 4);
        int blk = 0;
        for (; blk + 2 <= nblk; blk += 2) {
            art_s *r = row + 8 * blk; const art_s *pr = prow + 8 * blk;
            const vec4 ub0 = *(const vec4 *)(r + 8), ub1 = *(const vec4 *)(r + 12), pb0 = *(const vec4 *)(pr + 8), pb1 = *(const vec4 *)(pr + 12);
            __builtin_amdgcn_sched_barrier (0);
            const vec4 ya0 = four (ua0, pa0), ya1 = four (ua1, pa1);
            *(vec4 *)(r) = ya0; *(vec4 *)(r + 4) = ya1;
            __builtin_amdgcn_sched_barrier (0);
            ua0 = *(const vec4 *)(r + 16); ua1 = *(const vec4 *)(r + 20); pa0 = *(const vec4 *)(pr + 16); pa1 = *(const vec4 *)(pr + 20);
            __builtin_amdgcn_sched_barrier (0);
            const vec4 yb0 = four (ub0, pb0), yb1 = four (ub1, pb1);
            *(vec4 *)(r + 8) = yb0; *(vec4 *)(r + 12) = yb1;
            __builtin_amdgcn_sched_barrier (0);
        }
        if (blk < nblk) {
            const vec4 ya0 = four (ua0, pa0), ya1 = four (ua1, pa1);
            *(vec4 *)(row + 8 * blk) = ya0; *(vec4 *)(row + 8 * blk + 4) = ya1;
        }
    }
    int f = 8 * nblk;
    for (; f < len; ++f) {
        const art_s m = b1 * y1;
        const art_s t2 = row [f] - m;
        const art_s t3 = t2 + prow [f];
        const art_s q = b2 * y2;
        const art_s v = t3 - q;
        row [f] = v; y2 = y1; y1 = v;
    }
}

template <int S>                                   // S = 1 or 2 order-2 sections per channel
__global__ __launch_bounds__ (ST_THREADS)
void biquad_order2_ff_kernel (Biquad *sections, int C, int stride, art_s *buf, int frames, int cpw)   // stride: values between frames (>= C); cpw: channels per workgroup (<= 64)
{
    extern __shared__ __attribute__ ((aligned (32))) unsigned char ff_lds [];
    art_s *const A1 = (art_s *) ff_lds;            // [3][FF_CAP]  u1 -> y1, by chunk % 3
    art_s *const B1 = A1 + 3 * FF_CAP;             // [2][FF_CAP]  p1, by chunk parity
    art_s *const A2 = B1 + 2 * FF_CAP;             // [2][FF_CAP]  u2 -> y2
    art_s *const B2 = A2 + 2 * FF_CAP;             // [2][FF_CAP]  p2
    __shared__ art_s ffc [2][64][3];               // a0, a1, a2 per section and channel
    __shared__ art_s xtail [2][64][2];             // the two inputs preceding a chunk, by chunk parity: [0] nearest
    __shared__ art_s mtail [3][64][2];             // the two section-1 outputs preceding a chunk (chunk % 3)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = blockIdx.x * cpw, Cg = min (cpw, C - c0);

    // Chunk geometry.  A helper lane owns `run` consecutive frames of one channel (hc) in every chunk, `runs` lanes
    // per channel; a chunk is exactly runs*run frames (run a multiple of 4), the first chunk takes the remainder.
    int pitch = FF_CAP / Cg;
    pitch = pitch >= 36 ? ((pitch - 4) / 32) * 32 + 4 : pitch & ~3;
    const int runs = FF_HELPERS / Cg;
    const int hc = lane % Cg, hr = lane / Cg;
    int run = min (FF_RUN, ((pitch >= 36 ? pitch - 4 : pitch) / runs) & ~3);
    {   // no more chunk than the call has frames (short calls: several short chunks keep all four stages busy)
        const int want = (((frames + 3) / 4 + runs - 1) / runs + 3) & ~3;
        run = max (4, min (run, want));
    }
    const int len = runs * run;                                     // every chunk but the first
    const int nchunks = (frames + len - 1) / len;
    const int len0 = frames - (nchunks - 1) * len;                  // 1 .. len
    auto chunk_start = [&] (int k) { return k == 0 ? 0 : len0 + (k - 1) * len; };
    auto chunk_len = [&] (int k) { return k == 0 ? len0 : len; };
    const int f0 = hr * run;

    // per-lane recurrence state: wave 0 owns section 1, wave 1 section 2
    art_s b1 = 0, b2 = 0, y1 = 0, y2 = 0;
    art_s xt [4] = { 0, 0, 0, 0 };                 // the call's last four inputs (section 1's x history afterwards)
    if (tid < Cg) {
        const Biquad &f1 = sections [(size_t)(c0 + tid) * S];
        ffc [0][tid][0] = f1.a [0]; ffc [0][tid][1] = f1.a [1]; ffc [0][tid][2] = f1.a [2];
        xtail [0][tid][0] = f1.x [f1.index & 3]; xtail [0][tid][1] = f1.x [(f1.index - 1) & 3];
        b1 = f1.b [1]; b2 = f1.b [2]; y1 = f1.y [f1.index & 3]; y2 = f1.y [(f1.index - 1) & 3];
#pragma unroll
        for (int k = 0; k < 4; ++k) xt [k] = buf [(size_t)(frames - 1 - k) * stride + c0 + tid];     // frames >= 4 (launcher)
        if (S == 2) {
            const Biquad &f2 = sections [(size_t)(c0 + tid) * S + 1];
            ffc [1][tid][0] = f2.a [0]; ffc [1][tid][1] = f2.a [1]; ffc [1][tid][2] = f2.a [2];
            mtail [0][tid][0] = f2.x [f2.index & 3]; mtail [0][tid][1] = f2.x [(f2.index - 1) & 3];
        }
    }
    else if (S == 2 && wave == 1 && lane < Cg) {
        const Biquad &f2 = sections [(size_t)(c0 + lane) * S + 1];
        b1 = f2.b [1]; b2 = f2.b [2]; y1 = f2.y [f2.index & 3]; y2 = f2.y [(f2.index - 1) & 3];
    }
    __syncthreads ();

    const int store_lag = S == 2 ? 3 : 1;          // chunk k leaves the last section in step k + store_lag - 1
    const int esz = (int) sizeof (art_s);
    art_s xr [FF_RUN + 2];                         // wave 2: its run of the next chunk's inputs (+ the two before it)
    art_s xl0 = 0, xl1 = 0;                        //         and that chunk's last two inputs (hr == 0 lanes)
    auto fetch = [&] (int k) {
        if (wave != 2 || hr >= runs || k >= nchunks) return;
        const int L = chunk_len (k);
        const __amdgpu_buffer_rsrc_t rs = ff_rsrc (buf + (size_t) chunk_start (k) * stride + c0, ((size_t) L * stride - c0) * esz);
        // the two frames before the chunk (f0 == 0: patched from xtail later) are forced out of range by a select — a
        // negative offset is not left to wrap, the hardware's range check does not wrap register + immediate to 32 bits
#pragma unroll
        for (int j = 0; j < FF_RUN + 2; ++j) {     // (guards, not a break: constant trip counts keep the arrays in registers; run is a multiple of 4)
            const int f = f0 + j - 2;
            if (j < 2 || ((j - 2) & ~3) < run) xr [j] = ff_load (rs, f >= 0 ? (f * stride + hc) * esz : (int) 0xfffffff0u, art_s ());
        }
        xl0 = ff_load (rs, ((L - 1) * stride + hc) * esz, art_s ());
        xl1 = ff_load (rs, L >= 2 ? ((L - 2) * stride + hc) * esz : (int) 0xfffffff0u, art_s ());
    };
    fetch (0);

    for (int it = -1; it < nchunks + store_lag; ++it) {
        // Wave 2 only ever has loads in flight and wave 3 only stores, so neither waits for the other's memory
        // latency; the same (channel, frame) always belongs to the same lane, so wave 3 may store a buffer and
        // refill it without a barrier in between.
        if (wave == 2) {
            if (hr < runs) {
                if (it + 1 < nchunks) {                    // section 1's feed-forward part of chunk it+1, from the
                    const int k = it + 1, L = chunk_len (k), par = k & 1;      // inputs fetched during the previous step
                    art_s *ud = A1 + (k % 3) * FF_CAP + hc * pitch + f0, *pd = B1 + par * FF_CAP + hc * pitch + f0;
                    // the two frames before the chunk may already hold outputs (in-place): they come from xtail
                    if (hr == 0) {
                        xr [0] = xtail [par][hc][1]; xr [1] = xtail [par][hc][0];
                        xtail [par ^ 1][hc][0] = xl0; xtail [par ^ 1][hc][1] = L >= 2 ? xl1 : xr [1];
                    }
                    const art_s a0 = ffc [0][hc][0], a1 = ffc [0][hc][1], a2 = ffc [0][hc][2];
#pragma unroll
                    for (int j = 0; j < FF_RUN; ++j) {     // frames past a short first chunk land in row slack
                        if ((j & ~3) < run) {
                            const art_s p0 = xr [j + 2] * a0, p1 = xr [j + 1] * a1;
                            ud [j] = p0 + p1;
                            pd [j] = xr [j] * a2;
                        }
                    }
                }
                fetch (it + 2);                            // in flight across the barrier
            }
        }
        else if (wave == 3) {
            if (hr < runs) {
                {   // store the chunk that left the last section
                    const int k = it - store_lag;
                    if (k >= 0) {
                        const int L = chunk_len (k);
                        const art_s *src = (S == 2 ? A2 + (k & 1) * FF_CAP : A1 + (k % 3) * FF_CAP) + hc * pitch + f0;
                        const __amdgpu_buffer_rsrc_t rs = ff_rsrc (buf + (size_t) chunk_start (k) * stride + c0, ((size_t) L * stride - c0) * esz);
                        const int base = (f0 * stride + hc) * esz;
#pragma unroll
                        for (int g = 0; g < FF_RUN; g += FF_GROUP) {       // FF_GROUP frames at a time: reads first, then stores
                            art_s v [FF_GROUP];
#pragma unroll
                            for (int j = 0; j < FF_GROUP; ++j) { if (g + (j & ~3) < run) v [j] = src [g + j]; }
#pragma unroll
                            for (int j = 0; j < FF_GROUP; ++j) { if (g + (j & ~3) < run) ff_store (rs, base + (g + j) * stride * esz, v [j]); }
                        }
                    }
                }
                if (S == 2 && it >= 1 && it <= nchunks) {  // section 2's feed-forward part from section 1's outputs
                    const int k = it - 1;
                    const art_s *row = A1 + (k % 3) * FF_CAP + hc * pitch + f0;
                    art_s *ud = A2 + (k & 1) * FF_CAP + hc * pitch + f0, *pd = B2 + (k & 1) * FF_CAP + hc * pitch + f0;
                    const art_s a0 = ffc [1][hc][0], a1 = ffc [1][hc][1], a2 = ffc [1][hc][2];
#pragma unroll
                    for (int g = 0; g < FF_RUN; g += FF_GROUP) {           // FF_GROUP frames at a time (+ the two before them)
                        art_s x [FF_GROUP + 2];
#pragma unroll
                        for (int j = 0; j < FF_GROUP + 2; ++j) {
                            if (g + (j < 2 ? 0 : (j - 2) & ~3) < run) x [j] = row [hr == 0 && g + j < 2 ? 0 : g + j - 2];
                        }
                        if (g == 0 && hr == 0) { x [0] = mtail [k % 3][hc][1]; x [1] = mtail [k % 3][hc][0]; }
#pragma unroll
                        for (int j = 0; j < FF_GROUP; ++j) {
                            if (g + (j & ~3) < run) {
                                const art_s p0 = x [j + 2] * a0, p1 = x [j + 1] * a1;
                                ud [g + j] = p0 + p1;
                                pd [g + j] = x [j] * a2;
                            }
                        }
                    }
                }
            }
        }
        else if (wave == 0) {
            if (lane < Cg && it >= 0 && it < nchunks) {
                ff_serial (A1 + (it % 3) * FF_CAP + lane * pitch, B1 + (it & 1) * FF_CAP + lane * pitch, chunk_len (it), b1, b2, y1, y2);
                if (S == 2) { mtail [(it + 1) % 3][lane][0] = y1; mtail [(it + 1) % 3][lane][1] = y2; }
            }
        }
        else if (S == 2) {
            const int k = it - 2;
            if (lane < Cg && k >= 0 && k < nchunks)
                ff_serial (A2 + (k & 1) * FF_CAP + lane * pitch, B2 + (k & 1) * FF_CAP + lane * pitch, chunk_len (k), b1, b2, y1, y2);
        }
        // LDS-only barrier: wave 2's global loads (consumed next step) and wave 3's stores stay in flight across it;
        // no thread reads global memory another thread of this launch wrote
        asm volatile ("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    __syncthreads ();

    // ---- state write-back: the four most recent inputs / outputs of each section ----------------------
    if (tid < Cg) {
        // the last chunk (>= 4 frames whenever frames >= 4) is still in LDS as section outputs
        const int kl = nchunks - 1, L = chunk_len (kl);
        const art_s *r1 = A1 + (kl % 3) * FF_CAP + tid * pitch + L, *r2 = A2 + (kl & 1) * FF_CAP + tid * pitch + L;
        Biquad &f1 = sections [(size_t)(c0 + tid) * S];
        {
            const int i = f1.index + frames;
#pragma unroll
            for (int k = 0; k < 4; ++k) { f1.x [(i - k) & 3] = xt [k]; f1.y [(i - k) & 3] = r1 [-1 - k]; }
            f1.index = i;
        }
        if (S == 2) {
            Biquad &f2 = sections [(size_t)(c0 + tid) * S + 1];
            const int i = f2.index + frames;
#pragma unroll
            for (int k = 0; k < 4; ++k) { f2.x [(i - k) & 3] = r1 [-1 - k]; f2.y [(i - k) & 3] = r2 [-1 - k]; }
            f2.index = i;
        }
    }
}

// error-feedback filter with a compile-time order (per-sample association, reference biquad.c:83-95):
//     acc = in*a0;  for k = ORDER..1:  acc += (x_k*a_k) - (b_k*y_k)
// x_k / y_k for k >= 2 do not depend on the newest output, so those terms are formed ahead of the chain.
template <int ORDER>
__device__ __forceinline__ art_s shaper_step (SectionRegs &r, art_s in)
{
    art_s term [4];
#pragma unroll
    for (int k = 1; k <= 4; ++k)
        if (k <= ORDER) { const art_s fwd = r.x [k - 1] * r.a [k]; const art_s back = r.b [k] * r.y [k - 1]; term [k - 1] = fwd - back; }
    art_s acc = in * r.a [0];
#pragma unroll
    for (int k = 4; k >= 1; --k)
        if (k <= ORDER) acc = acc + term [k - 1];
    push (r, in, acc);
    return acc;
}

// The dither generator (decimator.c:370-382) steps r <- 15 r ^ 1 five times per sample.  15 r keeps the
// parity of r and "^ 1" flips it, so a step is 15 r + 1 on even r and 15 r - 1 on odd r and the parity
// alternates every step: five steps are one of two affine maps (chosen by the parity of the start state),
// the parity alternates every SAMPLE, and two samples are a single fixed affine map.  That gives an
// O(log n) jump-ahead, so a chunk's dither can be produced by all threads at once.
struct Affine { uint32_t a, b; };                  // r -> a r + b  (mod 2^32)
__device__ __forceinline__ Affine compose (Affine second, Affine first) { return { second.a * first.a, second.a * first.b + second.b }; }

__device__ __forceinline__ Affine five_steps (bool even_start)
{
    Affine m = { 1u, 0u };
    bool even = even_start;
#pragma unroll
    for (int i = 0; i < 5; ++i) { m = compose (Affine { 15u, even ? 1u : 0xffffffffu }, m); even = !even; }
    return m;
}

__device__ __forceinline__ uint32_t jump_pairs (uint32_t g, unsigned int pairs)     // advance by 2*pairs samples
{
    const bool even = (g & 1u) == 0;
    Affine two = compose (five_steps (!even), five_steps (even));                   // parity returns after two samples
    Affine acc = { 1u, 0u };
    while (pairs) {
        if (pairs & 1u) acc = compose (two, acc);
        two = compose (two, two);
        pairs >>= 1;
    }
    return acc.a * g + acc.b;
}

constexpr int DEC_CHUNK = ART_WIDE ? 2048 : 4096;                    // samples per chunk (16 KiB each for data and dither)
// floor (d + 0.5) as the reference evaluates it (decimator.c:262).  4-byte samples: the reference widens d to double
// first, so the sum is exact; v_cvt_rpi_i32_f32 ("round to nearest, ties towards +infinity") is exactly that function,
// computed without an intermediate rounding — verified on the hardware against floor ((double) d + 0.5) over 5M random
// and adversarial inputs (tools/micro/rpi_check.hip) — and puts two dependent operations on the serial path instead of
// four (floorf, subtract, compare, select).  Beyond +-2^31 it saturates where the reference's conversion is undefined.
// 8-byte samples: the reference's own sum rounds (e.g. d = 0.5 - 2^-54 gives 1), so it is evaluated literally.
__device__ __forceinline__ art_s round_half_up (art_s d)
{
#if ART_WIDE
    return floor (d + 0.5);
#else
    int q;
    asm ("v_cvt_rpi_i32_f32 %0, %1" : "=v" (q) : "v" (d));
    return (float) q;
#endif
}

constexpr int DEC_SEG = ART_DEC_SEG;               // consecutive samples of one channel per dither task (even; the batch host counts tasks with it)

// ---------------------------------------------------------------------------------------------------
// Channels-first (planar) sides: channel c of a buffer is a plane, c * pitch away from the first.  The arithmetic of every kernel
// below is untouched; a planar side only changes where a lane's or a task's samples are fetched and where its bytes land.  A
// plane's frames are consecutive, so a run of them is moved in whole aligned units cut at the boundaries of the run's OWN address
// (layout_kernels.hip does the same for samples): element by element before the first boundary and after the last, one access per
// unit between — 16-byte loads, 16-byte stores in the time-parallel kernels, 4-byte stores in the serial kernels' helper waves
// (dec_store_unit_of says why).  A pitch or a base of any alignment costs a run a head and a tail and nothing else.
// The kernels take a template parameter PITCHED: false is the interleaved kernel as it always was, true takes a pitch per side
// (0: that side interleaved).  The single-call kernels branch on it uniformly; in the batch kernels a side belongs to a lane
// (serial class) or an item (time-parallel class), which share workgroups whatever their layout, so there the branch is per lane
// or per task and a wave that holds both layouts pays for both.
// ---------------------------------------------------------------------------------------------------
constexpr int DEC_VEC = 16 / (int) sizeof (art_s);
typedef art_s dec_vec_t __attribute__ ((ext_vector_type (DEC_VEC)));

// w's bytes at byte `pos` (0..15) of the 16-byte image hi:lo; bytes past the image are dropped
__device__ __forceinline__ void dec_place (uint64_t &lo, uint64_t &hi, uint32_t w, int pos)
{
    const int sh = pos * 8;
    if (sh < 64) { lo |= (uint64_t) w << sh; if (sh > 32) hi |= (uint64_t) w >> (64 - sh); }
    else hi |= (uint64_t) w << (sh - 64);
}
__device__ __forceinline__ void dec_put_bytes (unsigned char *unit, uint64_t lo, uint64_t hi, int from, int to)     // bytes [from, to) of the image
{
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j >= from && j < to) unit [j] = (unsigned char)(j < 8 ? lo >> (8 * j) : hi >> (8 * (j - 8)));
}
__device__ __forceinline__ void dec_put_unit (unsigned char *unit, uint64_t lo, uint64_t hi)                        // unit: 16-byte aligned
{
    *reinterpret_cast<uint4 *> (unit) = make_uint4 ((uint32_t) lo, (uint32_t)(lo >> 32), (uint32_t) hi, (uint32_t)(hi >> 32));
}

// f (i, x) for the cnt consecutive samples at p, in order
template <typename F>
__device__ __forceinline__ void dec_for_run (const art_s *p, int cnt, F f)
{
    const int head = min (cnt, (int)(((16u - (unsigned int)((uintptr_t) p & 15u)) & 15u) / sizeof (art_s)));
    int i = 0;
    for (; i < head; ++i) f (i, p [i]);
    for (; i + DEC_VEC <= cnt; i += DEC_VEC) {
        const dec_vec_t v = *reinterpret_cast<const dec_vec_t *> (p + i);
#pragma unroll
        for (int j = 0; j < DEC_VEC; ++j) f (i + j, v [j]);
    }
    for (; i < cnt; ++i) f (i, p [i]);
}

// A thread's consecutive output bytes, in order: whole 16-byte units are one store each, the run's first and last unit go byte by byte
struct DecPacker {
    unsigned char *unit; uint64_t lo, hi; int pos, first;        // the unit being filled, its image, the next byte and the first valid one
    __device__ __forceinline__ void begin (unsigned char *p)
    {
        const int a = (int)((uintptr_t) p & 15u);
        unit = p - a; pos = first = a; lo = hi = 0;
    }
    __device__ __forceinline__ void put (uint32_t w, int nb)      // w: nb bytes (1..4), the rest zero
    {
        dec_place (lo, hi, w, pos);
        const int np = pos + nb;
        if (np < 16) { pos = np; return; }
        if (first == 0) dec_put_unit (unit, lo, hi); else dec_put_bytes (unit, lo, hi, first, 16);
        const int over = np - 16;                                 // bytes of w that belong to the next unit (0..3)
        lo = over ? (uint64_t)(w >> (8 * (nb - over))) : 0; hi = 0;
        unit += 16; first = 0; pos = over;
    }
    __device__ __forceinline__ void end () { if (pos > first) dec_put_bytes (unit, lo, hi, first, pos); }
};

// Unit u of a run of n consecutive samples at p (units are the 16-byte lines of the run's own address; at most
// dec_load_units (n) of them): store (i, x) for its samples
__device__ __forceinline__ int dec_load_units (int n) { return (n + 2 * DEC_VEC - 2) / DEC_VEC; }
template <typename F>
__device__ __forceinline__ void dec_load_unit (const art_s *p, int n, int u, F store)
{
    const int a = (int)(((uintptr_t) p & 15u) / sizeof (art_s));
    const int b = u * DEC_VEC - a, e = b + DEC_VEC;
    if (b >= 0 && e <= n) {
        const dec_vec_t v = *reinterpret_cast<const dec_vec_t *> (p + b);
#pragma unroll
        for (int j = 0; j < DEC_VEC; ++j) store (b + j, v [j]);
    }
    else
        for (int i = max (b, 0); i < min (e, n); ++i) store (i, p [i]);
}

// Unit u of the n * NB consecutive output bytes at p, a unit being UB = 4 aligned bytes of the run's own address (at most
// dec_store_units (n * NB) of them): word (f, counted) is frame f's bytes (dec_word); `counted` is true in exactly one unit per
// frame — the one that holds the frame's first byte — for the clip count.  Every frame that touches the unit is fetched (their number
// is bounded by NB and UB alone, so the fetches are independent of each other and of the unit's offset), laid out from the first
// one's first byte, and the image is then moved down by the bytes that lie before the unit.  A whole unit is one store, the run's
// first and last go byte by byte.
// UB: the serial kernels' helper waves have a few hundred bytes per lane and chunk to store and a chunk's step waits for the longest
// THREAD among them, so they take 4-byte units, not 16-byte ones (a quarter of the code per thread, four times the threads; a
// wave's stores still cover consecutive addresses); the 16-byte form's measurement is in profiles/decimate_planar.txt.
constexpr int DEC_STORE_UNIT = 4;
__device__ __forceinline__ int dec_store_units (int bytes) { return (bytes + 2 * DEC_STORE_UNIT - 2) / DEC_STORE_UNIT; }
template <int NB, typename F>
__device__ __forceinline__ void dec_store_unit_of (unsigned char *p, int n, int u, F word)
{
    constexpr int UB = DEC_STORE_UNIT;
    constexpr int MAXF = (UB + 2 * (NB - 1)) / NB;                 // frames a unit can touch (4, 3, 2, 2)
    constexpr int WORDS = (MAXF * NB + 7) / 8 + 1;
    const int a = (int)((uintptr_t) p & (UB - 1));
    const int b = max (u * UB - a, 0), e = min (u * UB - a + UB, n * NB);
    if (b >= e) return;
    const int f0 = b / NB, skip = b - f0 * NB;
    uint64_t im [WORDS] = {};
#pragma unroll
    for (int k = 0; k < MAXF; ++k) {
        const int f = f0 + k, at = k * NB;                         // (frames past the run or the unit: their bytes are never stored)
        const uint64_t w = word (min (f, n - 1), f < n && f * NB >= b && f * NB < e);
        im [at / 8] |= w << (8 * (at % 8));
        if (at % 8 + NB > 8) im [at / 8 + 1] |= w >> (64 - 8 * (at % 8));
    }
    const int sh = 8 * skip;
    const uint64_t lo = sh ? (im [0] >> sh) | (im [1] << (64 - sh)) : im [0];
    if (e - b == 4) *reinterpret_cast<uint32_t *> (p + b) = (uint32_t) lo;
    else
#pragma unroll
        for (int j = 0; j < 3; ++j) if (j < e - b) p [b + j] = (unsigned char)(lo >> (8 * j));
}
template <typename F>
__device__ __forceinline__ void dec_store_unit (unsigned char *p, int n, int nbytes, int u, F word)
{
    switch (nbytes) {
    case 1: dec_store_unit_of<1> (p, n, u, word); break;
    case 2: dec_store_unit_of<2> (p, n, u, word); break;
    case 3: dec_store_unit_of<3> (p, n, u, word); break;
    default: dec_store_unit_of<4> (p, n, u, word); break;
    }
}

// One task of the time-parallel kernels (no noise shaping, so no recurrence: the feedback term is a constant, decimator.c:264-265):
// frames [n0, n0 + DEC_SEG) of channel c of item `a`, the generator jumped to n0.  PITCHED: either side may be planar — a planar
// input is read as one run, a planar output packed into 16-byte stores; without it both sides are interleaved and the pitches are
// not looked at.  The channel's last task leaves the generator state in gens_next (the rest still read gens; the host swaps them).
// The clips entry's records (decimateProcessClipsPlanarLEDevice) carry the batch entry's and more; the kernel bodies are instantiated
// per record type, for kernels of their own, so the batch entry's kernels are the code they were.  What a body asks of its record:
__device__ __forceinline__ const ArtDecTask &dec_task (const ArtDecTask &t) { return t; }
__device__ __forceinline__ const ArtDecTask &dec_task (const ArtDecClipTask &t) { return t.task; }
__device__ __forceinline__ void dec_count_item (const ArtDecTask &, unsigned long long) {}
__device__ __forceinline__ void dec_count_item (const ArtDecClipTask &t, unsigned long long n) { if (t.item_clipped) atomicAdd (t.item_clipped, n); }
__device__ __forceinline__ const ArtDecLane &dec_lane (const ArtDecLane &l) { return l; }
__device__ __forceinline__ const ArtDecLane &dec_lane (const ArtDecClipLane &l) { return l.lane; }
__device__ __forceinline__ const art_s *dec_feedback_from (const ArtDecLane &l) { return l.feedback; }
__device__ __forceinline__ const art_s *dec_feedback_from (const ArtDecClipLane &l) { return l.feedback_from; }
__device__ __forceinline__ const uint32_t *dec_gen_from (const ArtDecLane &l) { return l.gen; }
__device__ __forceinline__ const uint32_t *dec_gen_from (const ArtDecClipLane &l) { return l.gen_from; }
__device__ __forceinline__ const Biquad *dec_shaper_from (const ArtDecLane &l) { return l.shaper; }
__device__ __forceinline__ const Biquad *dec_shaper_from (const ArtDecClipLane &l) { return l.shaper_from; }
__device__ __forceinline__ void dec_shaper_index (const ArtDecLane &) {}                 // (store_section steps the live record's index:
__device__ __forceinline__ void dec_shaper_index (const ArtDecClipLane &l) { l.lane.shaper->index = l.shaper_from->index; }   // the source's first)
__device__ __forceinline__ void dec_count_item (const ArtDecLane &, unsigned long long) {}
__device__ __forceinline__ void dec_count_item (const ArtDecClipLane &l, unsigned long long n) { if (l.item_clipped) atomicAdd (l.item_clipped, n); }

template <bool DITHER, bool PITCHED, typename Task = ArtDecTask>
__device__ __forceinline__ void dec_parallel_task (const Task &item, int c, long n0)
{
    const ArtDecTask &a = dec_task (item);
    const art_s *const in = a.in;
    unsigned char *const out = a.out;
    const long in_pitch = PITCHED ? a.in_pitch : 0, out_pitch = PITCHED ? a.out_pitch : 0;
    const int C = a.C, dtype = a.dither_type, cnt = (int) min ((long) DEC_SEG, a.frames - n0);
    const DecFmt fm = dec_fmt (a.bits, a.bytes);
    const art_s scale = a.scale, fb = a.feedback [c];
    uint32_t g = DITHER ? jump_pairs (a.gens [c], (unsigned int)(n0 / 2)) : 0u;
    unsigned int clips = 0;
    DecPacker pk;
    unsigned char *const rows = out + ((size_t) n0 * C + c) * fm.nbytes;        // interleaved output: frame i at rows + i * C * nbytes
    if (out_pitch) pk.begin (out + (long) c * out_pitch + n0 * fm.nbytes);
    auto one = [&] (int i, art_s smp) {
        const art_s dither = DITHER ? tpdf_value (tpdf_step (g, dtype)) : 0.0f;
        const art_s scaled = smp * scale;
        const art_s code = scaled - fb;
        const art_s dithered = code + dither;
        int q = (int) round_half_up (dithered);
        DEC_CLIP (fm, q, clips++);
        if (out_pitch) pk.put (dec_word (fm, q), fm.nbytes);
        else DEC_STORE_BYTES (rows + (size_t) i * C * fm.nbytes, fm, q);
    };
    if (in_pitch) dec_for_run (in + (long) c * in_pitch + n0, cnt, one);
    else for (int i = 0; i < cnt; ++i) one (i, in [(size_t)(n0 + i) * C + c]);
    if (out_pitch) pk.end ();
    if (DITHER && n0 + cnt == a.frames) a.gens_next [c] = g;
    if (clips) { atomicAdd (a.clipped, (unsigned long long) clips); dec_count_item (item, (unsigned long long) clips); }
}

template <int ORDER, bool DITHER, bool PITCHED = false>                  // ORDER 0 = no noise shaping
__global__ __launch_bounds__ (ST_THREADS)
void decimate_lds_kernel (ArtDecArgs a, const art_s *in, int frames, unsigned char *out, int cpw, long in_pitch, long out_pitch)     // cpw: channels per workgroup (<= 64)
{
    __shared__ __attribute__ ((aligned (16))) art_s tile [DEC_CHUNK];          // input, then the rounded code values
    __shared__ __attribute__ ((aligned (16))) art_s dth [DITHER ? DEC_CHUNK : 1];
    __shared__ uint32_t s_gen [64], s_next [64];   // generator state at the start of this / the next chunk
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * cpw, Cg = min (cpw, a.C - c0);
    const int chunk_frames = (DEC_CHUNK / Cg) & ~1;                            // even: chunk boundaries keep generator parity

    art_s fb = 0.0f; SectionRegs sh; unsigned long long clips = 0;
    if (tid < Cg) {
        fb = a.feedback [c0 + tid];
        if (DITHER) s_gen [tid] = a.gens [c0 + tid];
        if (ORDER) load_section (sh, a.shapers [c0 + tid]);
    }
    const DecFmt fm = dec_fmt (a.bits, a.bytes);
    const int nbytes = fm.nbytes, dtype = a.dither_type;
    const art_s scale = a.scale;
    __syncthreads ();

    for (int f0 = 0; f0 < frames; f0 += chunk_frames) {
        const int nf = min (chunk_frames, frames - f0);

        // ---- phase A (all threads): load the chunk; produce its dither by jump-ahead
        if (PITCHED && in_pitch) {                 // a channel's frames are one run of its plane
            const int units = dec_load_units (nf);
            for (int e = tid; e < units * Cg; e += ST_THREADS) {
                const int c = e / units, u = e - c * units;
                dec_load_unit (in + (long)(c0 + c) * in_pitch + f0, nf, u, [&] (int f, art_s x) { tile [f * Cg + c] = x; });
            }
        }
        else
        for (int e = tid; e < nf * Cg; e += ST_THREADS) {
            const int f = e / Cg, c = e - f * Cg;
            tile [e] = in [(size_t)(f0 + f) * a.C + c0 + c];
        }
        if (DITHER) {
            const int segs_per_ch = (nf + DEC_SEG - 1) / DEC_SEG;
            for (int task = tid; task < segs_per_ch * Cg; task += ST_THREADS) {
                const int c = task % Cg, k = task / Cg, n0 = k * DEC_SEG;
                uint32_t g = jump_pairs (s_gen [c], (unsigned int)(n0 / 2));
                const int cnt = min (DEC_SEG, nf - n0);
                for (int i = 0; i < cnt; ++i) dth [(n0 + i) * Cg + c] = tpdf_value (tpdf_step (g, dtype));
                if (n0 + cnt == nf) s_next [c] = g;          // the channel's last task publishes the next chunk's state
            }
        }
        __syncthreads ();

        // ---- phase B: rounding (round_half_up).  Without noise shaping the feedback term never changes, so there is
        // no recurrence and every thread rounds its own samples; with shaping one lane per channel walks time.
        if (!ORDER) {
            for (int e = tid; e < nf * Cg; e += ST_THREADS) {
                const int c = e % Cg;
                const art_s code = tile [e] * scale - a.feedback [c0 + c];
                const art_s dithered = code + (DITHER ? dth [e] : 0.0f);
                tile [e] = round_half_up (dithered);
            }
        }
        else if (tid < Cg) {
            if (DITHER) s_gen [tid] = s_next [tid];          // phase A of the next chunk is two barriers away
            auto one = [&] (art_s smp, art_s dither) -> art_s {
                const art_s scaled = smp * scale;
                const art_s code = scaled - fb;
                const art_s dithered = code + dither;
                const art_s qf = round_half_up (dithered);
                const art_s err = qf - code;
                fb = shaper_step<ORDER> (sh, err);
                return qf;
            };
            constexpr int UB = 8;
            int f = 0;
            for (; f + UB <= nf; f += UB) {
                art_s x [UB], d [UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) { x [u] = tile [(f + u) * Cg + tid]; d [u] = DITHER ? dth [(f + u) * Cg + tid] : 0.0f; }
#pragma unroll
                for (int u = 0; u < UB; ++u) x [u] = one (x [u], d [u]);
#pragma unroll
                for (int u = 0; u < UB; ++u) tile [(f + u) * Cg + tid] = x [u];
            }
            for (; f < nf; ++f) tile [f * Cg + tid] = one (tile [f * Cg + tid], DITHER ? dth [f * Cg + tid] : 0.0f);
        }
        if (!ORDER && DITHER && tid < Cg) s_gen [tid] = s_next [tid];   // (s_next was published before the barrier above)
        __syncthreads ();

        // ---- phase C (all threads): clip, pack little-endian, store
        if (PITCHED && out_pitch) {                // a channel's bytes are one run of its plane
            const int units = dec_store_units (nf * nbytes);
            for (int e = tid; e < units * Cg; e += ST_THREADS) {
                const int c = e / units, u = e - c * units;
                dec_store_unit (out + (long)(c0 + c) * out_pitch + (long) f0 * nbytes, nf, nbytes, u, [&] (int f, bool counted) {
                    int q = (int) tile [f * Cg + c];
                    DEC_CLIP (fm, q, if (counted) clips++);
                    return dec_word (fm, q);
                });
            }
        }
        else
        for (int e = tid; e < nf * Cg; e += ST_THREADS) {
            const int f = e / Cg, c = e - f * Cg;
            int q = (int) tile [e];
            DEC_CLIP (fm, q, clips++);
            DEC_STORE_BYTES (out + ((size_t)(f0 + f) * a.C + c0 + c) * nbytes, fm, q);
        }
        __syncthreads ();
    }

    if (tid < Cg) {
        a.feedback [c0 + tid] = fb;
        if (DITHER) a.gens [c0 + tid] = s_gen [tid];
        if (ORDER) store_section (a.shapers [c0 + tid], sh, frames, true);
    }
    if (clips) atomicAdd (a.clipped, clips);
}


// Noise-shaped decimator as a three-stage pipeline over chunks (the serial lane is latency-bound: a 10-deep dependent
// chain per sample — so everything that is not that chain runs beside it, on the other waves):
//     waves 1-3   phase A of chunk it+1 (load, dither by jump-ahead)   |   phase C of chunk it-1 (clip, pack, store)
//     wave 0      phase B of chunk it: one lane per channel through the error-feedback recurrence
// one LDS-only barrier per step; three sample tiles (by chunk % 3), two dither tiles and two generator-state rows.
template <int ORDER, bool DITHER, bool PITCHED = false>                  // ORDER >= 1
__global__ __launch_bounds__ (ST_THREADS)
void decimate_pipe_kernel (ArtDecArgs a, const art_s *in, int frames, unsigned char *out, int cpw, long in_pitch, long out_pitch)
{
    extern __shared__ __attribute__ ((aligned (16))) unsigned char dec_lds [];
    art_s *const tiles = (art_s *) dec_lds;                               // [3][DEC_CHUNK]
    art_s *const dths = tiles + 3 * DEC_CHUNK;                            // [2][DEC_CHUNK]
    __shared__ uint32_t s_gen [2][64];             // generator state at the start of a chunk, by chunk parity
    const int tid = threadIdx.x, wave = tid >> 6;
    const int c0 = blockIdx.x * cpw, Cg = min (cpw, a.C - c0);
    // LDS tiles are CHANNEL-major, [channel][frame] with a pitch of chunk_frames + 4 (the serial lane then moves four frames per
    // ds_read_b128 / ds_write_b128 instead of one per instruction — a lone wave's budget is instructions; the +4 keeps the
    // channels' rows on different banks)
    const int chunk_frames = ((DEC_CHUNK / Cg) - 4) & ~3;                 // multiple of 4 (vector alignment; even: chunk boundaries keep generator parity)
    const int pitch = chunk_frames + 4;
    const int nchunks = (frames + chunk_frames - 1) / chunk_frames;

    art_s fb = 0.0f; SectionRegs sh; unsigned long long clips = 0;
    if (tid < Cg) {
        fb = a.feedback [c0 + tid];
        if (DITHER) s_gen [0][tid] = a.gens [c0 + tid];
        load_section (sh, a.shapers [c0 + tid]);
    }
    const DecFmt fm = dec_fmt (a.bits, a.bytes);
    const int nbytes = fm.nbytes, dtype = a.dither_type;
    const art_s scale = a.scale;
    constexpr int HELPERS = ST_THREADS - 64;
    __syncthreads ();

    for (int it = -1; it <= nchunks; ++it) {
        if (wave >= 1) {
            const int ht = tid - 64;
            if (it + 1 < nchunks) {                // ---- phase A of chunk it+1
                const int k = it + 1, f0 = k * chunk_frames, nf = min (chunk_frames, frames - f0);
                art_s *tile = tiles + (k % 3) * DEC_CHUNK, *dth = dths + (k & 1) * DEC_CHUNK;
                if (PITCHED && in_pitch) {         // a channel's frames are one run of its plane
                    const int units = dec_load_units (nf);
                    for (int e = ht; e < units * Cg; e += HELPERS) {
                        const int c = e / units, u = e - c * units;
                        dec_load_unit (in + (long)(c0 + c) * in_pitch + f0, nf, u, [&] (int f, art_s x) { tile [c * pitch + f] = x * scale; });
                    }
                }
                else
                for (int e = ht; e < nf * Cg; e += HELPERS) {
                    const int f = e / Cg, c = e - f * Cg;
                    tile [c * pitch + f] = in [(size_t)(f0 + f) * a.C + c0 + c] * scale;     // (the serial wave's first operation, done here: same product)
                }
                if (DITHER) {
                    const int segs_per_ch = (nf + DEC_SEG - 1) / DEC_SEG;
                    for (int task = ht; task < segs_per_ch * Cg; task += HELPERS) {
                        const int c = task % Cg, sgm = task / Cg, n0 = sgm * DEC_SEG;
                        uint32_t g = jump_pairs (s_gen [k & 1][c], (unsigned int)(n0 / 2));
                        const int cnt = min (DEC_SEG, nf - n0);
                        for (int i = 0; i < cnt; ++i) dth [c * pitch + n0 + i] = tpdf_value (tpdf_step (g, dtype));
                        if (n0 + cnt == nf) s_gen [(k & 1) ^ 1][c] = g;      // start state of chunk k+1
                    }
                }
            }
            if (it >= 1) {                         // ---- phase C of chunk it-1
                const int k = it - 1, f0 = k * chunk_frames, nf = min (chunk_frames, frames - f0);
                const art_s *tile = tiles + (k % 3) * DEC_CHUNK;
                if (PITCHED && out_pitch) {        // a channel's bytes are one run of its plane
                    const int units = dec_store_units (nf * nbytes);
                    for (int e = ht; e < units * Cg; e += HELPERS) {
                        const int c = e / units, u = e - c * units;
                        dec_store_unit (out + (long)(c0 + c) * out_pitch + (long) f0 * nbytes, nf, nbytes, u, [&] (int f, bool counted) {
                            int q = (int) tile [c * pitch + f];
                            DEC_CLIP (fm, q, if (counted) clips++);
                            return dec_word (fm, q);
                        });
                    }
                }
                else
                for (int e = ht; e < nf * Cg; e += HELPERS) {
                    const int f = e / Cg, c = e - f * Cg;
                    int q = (int) tile [c * pitch + f];
                    DEC_CLIP (fm, q, clips++);
                    DEC_STORE_BYTES (out + ((size_t)(f0 + f) * a.C + c0 + c) * nbytes, fm, q);
                }
            }
        }
        else if (tid < Cg && it >= 0 && it < nchunks) {      // ---- phase B of chunk it
            const int f0 = it * chunk_frames, nf = min (chunk_frames, frames - f0);
            art_s *tile = tiles + (it % 3) * DEC_CHUNK;
            const art_s *dth = dths + (it & 1) * DEC_CHUNK;
#include "pcm_dec_serial_row.inc"
        }
        // LDS-only barrier: the helpers' stores (and loads already consumed) stay in flight; nobody reads global memory
        // that this launch writes
        asm volatile ("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    __syncthreads ();

    if (tid < Cg) {
        a.feedback [c0 + tid] = fb;
        if (DITHER) a.gens [c0 + tid] = s_gen [nchunks & 1][tid];
        store_section (a.shapers [c0 + tid], sh, frames, true);
    }
    if (clips) atomicAdd (a.clipped, clips);
}

// No noise shaping => no recurrence at all: the time axis is cut into segments of DEC_SEG frames, each thread
// jumps its channel's dither generator to its segment and converts it.  Adjacent threads are adjacent
// channels of the same frames.  The generator state after the call is written to a second array (the first
// is still being read by other threads); the host swaps them.
template <bool DITHER, bool PITCHED = false>
__global__ __launch_bounds__ (256)
void decimate_parallel_kernel (ArtDecTask a)       // one item, by value (task0 = 0)
{
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (PITCHED) {                                 // neighbouring threads are neighbouring segments of one plane
        const long segs = (a.frames + DEC_SEG - 1) / DEC_SEG;
        if (task >= segs * a.C) return;
        const int c = (int)(task / segs);
        dec_parallel_task<DITHER, true> (a, c, (task - c * segs) * DEC_SEG);
        return;
    }
    const long n0 = (task / a.C) * DEC_SEG;        // neighbouring threads are neighbouring channels of the same frames
    if (n0 < a.frames) dec_parallel_task<DITHER, false> (a, (int)(task % a.C), n0);
}

// ---------------------------------------------------------------------------------------------------
// Many contexts in one launch (decimateProcessBatchInterleavedLEDevice).  Phase B — the error-feedback recurrence — depends only
// on the shaper order and on whether dither is on; the gain, the dither type and the output format are applied by the helper
// waves.  So channels of different contexts share one serial wave, each lane reading its own descriptor, and the bits are those
// of the single call: the same operations in the same order, per lane.
// ---------------------------------------------------------------------------------------------------
constexpr int DEC_BATCH_RUN = 60;                  // frames per chunk at most: a service tick is a few hundred frames, and the
                                                   // pipeline's fill and drain cost two chunks of the serial lane's time

// decimate_pipe_kernel over `lanes` lanes of ArtDecLane descriptors per workgroup.  LDS tiles are [lane][frame] with a pitch of
// chunk_frames + 4 (a multiple of 4: the serial lane's 16-byte LDS accesses); the launcher sizes them by `lanes`, so small
// workgroups are small in LDS too.  A lane whose context has fewer frames than the workgroup's longest sits the rest out.
// PITCHED: a class with a planar side among its lanes.  A lane's side is a run of consecutive frames exactly when its stride there is 1
// (a plane, or a one-channel stream): the helper waves then move that lane's side of a chunk unit by unit, and every other lane's
// element by element as before.
// Lane: the record type (the kernels proper follow the body).  An ArtDecClipLane reads its first state from where the record says (the context's initial image, or the
// live state) and counts its clipped samples for its item as well.
template <int ORDER, bool DITHER, bool PITCHED, typename Lane>            // ORDER 0: no noise shaping (calls under 64 frames)
__device__ __forceinline__ void dec_batch_pipe_body (const Lane *table, int lanes, int chunk_frames)
{
    extern __shared__ __attribute__ ((aligned (16))) unsigned char dec_lds [];
    const int pitch = chunk_frames + 4, span = lanes * pitch;
    art_s *const tiles = (art_s *) dec_lds;                               // [3][lanes][pitch]
    art_s *const dths = tiles + 3 * span;                                 // [2][lanes][pitch]
    __shared__ uint32_t s_gen [2][64];             // generator state at the start of a chunk, by chunk parity
    __shared__ const art_s *s_in [64];
    __shared__ unsigned char *s_out [64];
    __shared__ art_s s_scale [64];
    __shared__ int s_stride [64], s_frames [64], s_fmt [64];            // fmt: bits | bytes << 8 | (dither type + 1) << 16
    __shared__ int s_ostride [PITCHED ? 64 : 1];                        // PITCHED: the output's stride in frames (s_stride: the input's)
    __shared__ unsigned int s_clips [64];
    const int tid = threadIdx.x, wave = tid >> 6;
    const Lane *const mine = table + (size_t) blockIdx.x * lanes;

    art_s fb = 0; SectionRegs sh; int my_frames = 0;
    if (tid < lanes) {
        const Lane &rec = mine [tid];
        const ArtDecLane &d = dec_lane (rec);
        s_in [tid] = d.in; s_out [tid] = d.out; s_scale [tid] = d.scale; s_stride [tid] = d.stride; s_frames [tid] = d.frames;
        s_fmt [tid] = d.bits | (d.bytes << 8) | ((d.dither_type + 1) << 16);
        s_clips [tid] = 0;
        if (PITCHED) s_ostride [tid] = d.out_stride;
        my_frames = d.frames;
        if (my_frames > 0) {
            fb = *dec_feedback_from (rec);
            if (DITHER) s_gen [0][tid] = *dec_gen_from (rec);
            if (ORDER) load_section (sh, *dec_shaper_from (rec));
        }
    }
    __syncthreads ();
    int frames = 0;
    for (int c = 0; c < lanes; ++c) frames = max (frames, s_frames [c]);
    const int nchunks = (frames + chunk_frames - 1) / chunk_frames;
    constexpr int HELPERS = ST_THREADS - 64;

    for (int it = -1; it <= nchunks; ++it) {
        if (wave >= 1) {
            const int ht = tid - 64;
            if (it + 1 < nchunks) {                // ---- phase A of chunk it+1 (a thread walks one lane's frames: its reads are
                const int k = it + 1, f0 = k * chunk_frames, nf = min (chunk_frames, frames - f0);    // that context's interleave)
                art_s *tile = tiles + (k % 3) * span, *dth = dths + (k & 1) * span;
                for (int e = ht; e < nf * lanes; e += HELPERS) {
                    const int c = e / nf, f = e - c * nf;
                    if (PITCHED && s_stride [c] == 1) {      // task f of the lane is unit f of its run (a run has at most nf units)
                        const int nfc = min (nf, s_frames [c] - f0);
                        const art_s sc = s_scale [c];
                        if (nfc > 0 && f < dec_load_units (nfc))
                            dec_load_unit (s_in [c] + f0, nfc, f, [&] (int i, art_s x) { tile [c * pitch + i] = x * sc; });
                        continue;
                    }
                    if (f0 + f < s_frames [c]) tile [c * pitch + f] = s_in [c][(size_t)(f0 + f) * s_stride [c]] * s_scale [c];
                }
                if (DITHER) {
                    const int segs = (nf + DEC_SEG - 1) / DEC_SEG;
                    for (int task = ht; task < segs * lanes; task += HELPERS) {
                        const int c = task / segs, sgm = task - c * segs, n0 = sgm * DEC_SEG;
                        const int nfc = min (nf, s_frames [c] - f0);                 // this lane's frames in the chunk (may be <= 0)
                        if (n0 >= nfc) continue;
                        const int dtype = (s_fmt [c] >> 16) - 1;
                        uint32_t g = jump_pairs (s_gen [k & 1][c], (unsigned int)(n0 / 2));
                        const int cnt = min (DEC_SEG, nfc - n0);
                        for (int i = 0; i < cnt; ++i) dth [c * pitch + n0 + i] = tpdf_value (tpdf_step (g, dtype));
                        if (n0 + cnt == nfc) s_gen [(k & 1) ^ 1][c] = g;    // start state of the lane's chunk k+1 (or its final state)
                    }
                }
            }
            if (it >= 1) {                         // ---- phase C of chunk it-1
                const int k = it - 1, f0 = k * chunk_frames, nf = min (chunk_frames, frames - f0);
                const art_s *tile = tiles + (k % 3) * span;
                const int per = PITCHED ? max (nf, dec_store_units (nf * 4)) : nf;     // tasks per lane: its frames, or the units of a 4-byte format's run
                for (int e = ht; e < per * lanes; e += HELPERS) {
                    const int c = e / per, f = e - c * per;
                    if (PITCHED && s_ostride [c] == 1) {     // task f of the lane is unit f of its run of bytes
                        const int nfc = min (nf, s_frames [c] - f0);
                        const DecFmt fm = dec_fmt (s_fmt [c] & 255, (s_fmt [c] >> 8) & 255);
                        if (nfc > 0 && f < dec_store_units (nfc * fm.nbytes))
                            dec_store_unit (s_out [c] + (size_t) f0 * fm.nbytes, nfc, fm.nbytes, f, [&] (int i, bool counted) {
                                int q = (int) tile [c * pitch + i];
                                DEC_CLIP (fm, q, if (counted) atomicAdd (&s_clips [c], 1u));
                                return dec_word (fm, q);
                            });
                        continue;
                    }
                    if ((PITCHED && f >= nf) || f0 + f >= s_frames [c]) continue;
                    const int fmt = s_fmt [c], bits = fmt & 255, nbytes = (fmt >> 8) & 255;
                    const DecFmt fm = DEC_FMT (bits, nbytes);
                    int q = (int) tile [c * pitch + f];
                    DEC_CLIP (fm, q, atomicAdd (&s_clips [c], 1u));
                    DEC_STORE_BYTES (s_out [c] + (size_t)(f0 + f) * (PITCHED ? s_ostride [c] : s_stride [c]) * fm.nbytes, fm, q);
                }
            }
        }
        else if (tid < lanes && it >= 0 && it < nchunks && it * chunk_frames < my_frames) {     // ---- phase B of chunk it
            const int f0 = it * chunk_frames, nf = min (chunk_frames, my_frames - f0);
            art_s *tile = tiles + (it % 3) * span;
            const art_s *dth = dths + (it & 1) * span;
#include "pcm_dec_serial_row.inc"
        }
        // LDS-only barrier, as in decimate_pipe_kernel: nobody reads global memory that this launch writes
        asm volatile ("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
    __syncthreads ();

    if (tid < lanes && my_frames > 0) {
        const Lane &rec = mine [tid];
        const ArtDecLane &d = dec_lane (rec);
        *d.feedback = fb;
        if (DITHER) *d.gen = s_gen [((my_frames + chunk_frames - 1) / chunk_frames) & 1][tid];
        if (ORDER) { dec_shaper_index (rec); store_section (*d.shaper, sh, my_frames, true); }
        if (s_clips [tid]) { atomicAdd (d.clipped, (unsigned long long) s_clips [tid]); dec_count_item (rec, (unsigned long long) s_clips [tid]); }
    }
}

template <int ORDER, bool DITHER, bool PITCHED = false>
__global__ __launch_bounds__ (ST_THREADS)
void decimate_batch_pipe_kernel (const ArtDecLane *table, int lanes, int chunk_frames)
{
    dec_batch_pipe_body<ORDER, DITHER, PITCHED> (table, lanes, chunk_frames);
}

// ... over the clips entry's records; always PITCHED, which takes interleaved lanes as well
template <int ORDER, bool DITHER>
__global__ __launch_bounds__ (ST_THREADS)
void decimate_clips_pipe_kernel (const ArtDecClipLane *table, int lanes, int chunk_frames)
{
    dec_batch_pipe_body<ORDER, DITHER, true> (table, lanes, chunk_frames);
}

// the item a task of a flattened task space belongs to: the last whose first task is <= task (items [0].task0 == 0, ascending)
template <typename Item>
__device__ __forceinline__ const Item &item_of (const Item *items, int n, long task)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items [mid].task0 <= task) lo = mid; else hi = mid - 1; }
    return items [lo];
}

// decimate_parallel_kernel over a flattened task space: (context, channel, DEC_SEG-frame segment).  A thread finds its context by
// binary search over the contexts' first tasks (item_of).
template <bool DITHER, bool PITCHED, typename Task>
__device__ __forceinline__ void dec_batch_parallel_body (const Task *items, int n, long tasks)
{
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= tasks) return;
    const Task &item = item_of (items, n, task);
    const ArtDecTask &a = dec_task (item);
    const long t = task - a.task0;
    if (PITCHED && (a.in_pitch || a.out_pitch)) {  // neighbouring threads are neighbouring segments of one plane
        const long segs = (a.frames + DEC_SEG - 1) / DEC_SEG;
        const int c = (int)(t / segs);
        dec_parallel_task<DITHER, true> (item, c, (t - c * segs) * DEC_SEG);
        return;
    }
    const long n0 = (t / a.C) * DEC_SEG;           // (an interleaved item of a PITCHED class as well) neighbouring threads are
    if (n0 < a.frames) dec_parallel_task<DITHER, false> (item, (int)(t % a.C), n0);    // neighbouring channels of the same frames
}

template <bool DITHER, bool PITCHED = false>      // PITCHED: a class with a planar side among its items
__global__ __launch_bounds__ (256)
void decimate_batch_parallel_kernel (const ArtDecTask *items, int n, long tasks)
{
    dec_batch_parallel_body<DITHER, PITCHED> (items, n, tasks);
}

template <bool DITHER>                             // ... over the clips entry's records; always PITCHED
__global__ __launch_bounds__ (256)
void decimate_clips_parallel_kernel (const ArtDecClipTask *items, int n, long tasks)
{
    dec_batch_parallel_body<DITHER, true> (items, n, tasks);
}

// ---------------------------------------------------------------------------------------------------
// Many biquad banks in one launch (biquadBankApplyBatchInterleavedDevice): the serial cascade of biquad_chain_kernel, one lane per
// channel of any bank, S sections per lane (each section's own order at run time), in the three-phase pipeline of
// decimate_batch_pipe_kernel.  Waves 1-3 load chunk it+1 into LDS and store chunk it-1 back in place while lanes 0..lanes-1 of wave 0
// run chunk it; one LDS-only barrier per step.  Every lane makes the same operations in the same order as the single call's serial
// form (step_buffer_order, reference biquad.c:106-163), so the bits are the single call's.
// ---------------------------------------------------------------------------------------------------
constexpr int BQ_Q = 16 / (int) sizeof (art_s);    // frames to 16 bytes
typedef art_s bq_vecq __attribute__ ((ext_vector_type (BQ_Q)));
// a lane whose frames are consecutive (a plane, or a one-channel bank) from a 16-byte boundary: the helper waves move it 16 bytes at a time
__device__ __forceinline__ bool bq_plane_aligned (const art_s *buf, int stride) { return stride == 1 && !((uintptr_t) buf & 15); }

// The helper waves' move of one chunk (frames [f0, f0 + nf) of every lane) between one side of the lanes' buffers and an LDS tile,
// LOAD: into the tile; the one copy for both pipe kernels.  Task e = (lane c, frame f), a thread walks one lane's frames.  A plane
// on a 16-byte boundary (f0 is a multiple of 4) goes 16 bytes at a time: the first thread of every whole group of BQ_Q frames moves
// the group.  REV: frame n of a lane of `count` frames lives at address count - 1 - n, one sample at a time (the lanes of a
// workgroup differ in count, so a tile row and a plane share no 16-byte cut).
template <bool LOAD, bool REV>
__device__ __forceinline__ void bq_move_chunk (art_s *tile, int pitch, int lanes, int f0, int nf, int first, int step,
                                               typename std::conditional<LOAD, const art_s, art_s>::type *const *bufs, const int *strides, const int *counts)
{
    for (int e = first; e < nf * lanes; e += step) {
        const int c = e / nf, f = e - c * nf;
        const int left = counts [c] - (f0 + f);
        if (left <= 0) continue;
        const int stride = strides [c];
        art_s *const t = tile + c * pitch + f;
        const size_t at = (size_t)(REV ? left - 1 : f0 + f) * stride;
        if constexpr (!REV) {
            if (bq_plane_aligned (bufs [c], stride)) {
                if (left >= BQ_Q - (f & (BQ_Q - 1))) {
                    if (!(f & (BQ_Q - 1))) {
                        if constexpr (LOAD) *reinterpret_cast<bq_vecq *> (t) = *reinterpret_cast<const bq_vecq *> (bufs [c] + at);
                        else *reinterpret_cast<bq_vecq *> (bufs [c] + at) = *reinterpret_cast<const bq_vecq *> (t);
                    }
                    continue;
                }
            }
        }
        if constexpr (LOAD) *t = bufs [c][at]; else bufs [c][at] = *t;
    }
}

constexpr int BQ_BATCH_RUN = 60;                   // frames per chunk at most (the decimator batch's: fill and drain cost two chunks)

// The pipeline, the one copy for both pipe kernels: Lane = ArtBqLane filters in place and stores the state back, ArtBqFilterLane
// reads one side, writes the other (REV: with time reversed) and stores no state.
// LDS: three tiles [lanes][chunk_frames + 4] (the pitch is a multiple of 4: one ds_read_b128 feeds the serial lane 4 float frames),
// sized by the launcher from `lanes`.  A lane with fewer frames than the workgroup's longest sits the rest out.
template <int S, bool REV, typename Lane>
__device__ __forceinline__ void bq_pipe_body (const Lane *table, int lanes, int chunk_frames)
{
    constexpr bool IN_PLACE = std::is_same<Lane, ArtBqLane>::value;
    extern __shared__ __attribute__ ((aligned (16))) unsigned char bq_lds [];
    const int pitch = chunk_frames + 4, span = lanes * pitch;
    art_s *const tiles = (art_s *) bq_lds;                                // [3][lanes][pitch]
    __shared__ const art_s *s_in [64];                                    // (in place: the output side's arrays alone are used)
    __shared__ art_s *s_out [64];
    __shared__ int s_in_stride [64], s_out_stride [64], s_frames [64];
    const int tid = threadIdx.x, wave = tid >> 6;
    const Lane *const mine = table + (size_t) blockIdx.x * lanes;

    SectionRegs r [S];
    int my_frames = 0;
    if (tid < lanes) {
        const Lane &d = mine [tid];
        if constexpr (IN_PLACE) { s_out [tid] = d.buf; s_out_stride [tid] = d.stride; }
        else { s_in [tid] = d.in; s_out [tid] = d.out; s_in_stride [tid] = d.in_stride; s_out_stride [tid] = d.out_stride; }
        s_frames [tid] = d.frames;
        my_frames = d.frames;
        if (my_frames > 0) {
#pragma unroll
            for (int s = 0; s < S; ++s) load_section (r [s], d.sections [s]);
        }
    }
    __syncthreads ();
    int frames = 0;
    for (int c = 0; c < lanes; ++c) frames = max (frames, s_frames [c]);
    const int nchunks = (frames + chunk_frames - 1) / chunk_frames;
    constexpr int HELPERS = ST_THREADS - 64;

    for (int it = -1; it <= nchunks; ++it) {
        if (wave >= 1) {
            const int ht = tid - 64;
            if (it + 1 < nchunks) {                // ---- load chunk it+1
                const int k = it + 1, f0 = k * chunk_frames;
                if constexpr (IN_PLACE) bq_move_chunk<true, REV> (tiles + (k % 3) * span, pitch, lanes, f0, min (chunk_frames, frames - f0), ht, HELPERS, s_out, s_out_stride, s_frames);
                else bq_move_chunk<true, REV> (tiles + (k % 3) * span, pitch, lanes, f0, min (chunk_frames, frames - f0), ht, HELPERS, s_in, s_in_stride, s_frames);
            }
            if (it >= 1) {                         // ---- store chunk it-1
                const int k = it - 1, f0 = k * chunk_frames;
                bq_move_chunk<false, REV> (tiles + (k % 3) * span, pitch, lanes, f0, min (chunk_frames, frames - f0), ht, HELPERS, s_out, s_out_stride, s_frames);
            }
        }
        else if (tid < lanes && it >= 0 && it < nchunks && it * chunk_frames < my_frames) {     // ---- the cascade over chunk it
            const int f0 = it * chunk_frames, nf = min (chunk_frames, my_frames - f0);
            art_s *row = tiles + (it % 3) * span + tid * pitch;
            typedef art_s vec4 __attribute__ ((ext_vector_type (4)));
            int f = 0;
            for (; f + 4 <= nf; f += 4) {
                vec4 v = *reinterpret_cast<const vec4 *> (row + f);
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int s = 0; s < S; ++s) v [u] = step_buffer_order (r [s], v [u]);
                *reinterpret_cast<vec4 *> (row + f) = v;
            }
            for (; f < nf; ++f) {
                art_s v = row [f];
#pragma unroll
                for (int s = 0; s < S; ++s) v = step_buffer_order (r [s], v);
                row [f] = v;
            }
        }
        // LDS-only barrier, as in decimate_pipe_kernel: nobody reads global memory that this launch writes
        asm volatile ("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }

    if constexpr (IN_PLACE) {
        if (tid < lanes && my_frames > 0) {
            Biquad *const sections = mine [tid].sections;
#pragma unroll
            for (int s = 0; s < S; ++s) store_section (sections [s], r [s], my_frames, false);
        }
    }
}

template <int S>
__global__ __launch_bounds__ (ST_THREADS)
void biquad_batch_pipe_kernel (const ArtBqLane *table, int lanes, int chunk_frames)
{
    bq_pipe_body<S, false> (table, lanes, chunk_frames);
}

// The passes as functions of one task, for the gathered kernels (bq_clips_*_kernel and bq_filter_*_kernel).  The runs themselves
// (run_plane, spec_run, spec_warm_up) are shared with the single call's kernels.  spec_task and repair_chunks are the one place for
// the gathered family's speculative task and repair loop.  COPIES, exactly these: biquad_spec_kernel and biquad_commit_kernel keep
// bodies of their own with spec_task's and repair_chunks' text, and check_task (which feeds bq_clips_check_kernel) is a copy of
// biquad_check_kernel's: a change to one goes into the other.  With the single kernels calling these functions they
// compile to other code, and each was slower on an MI355X than as it stands (single call against the build with the copies,
// profiles/biquad_shared_body.txt): the 8-byte biquad_spec_kernel<4, interleaved> 308.8 -> 353.2 us and 318.8 -> 368.8 us at the
// same 254 VGPRs, biquad_check_kernel up to 0.5 us in nine of ten traced cases (S = 3: 4.98 -> 5.32 us), the 4-byte
// biquad_commit_kernel<2, interleaved> 174.4 -> 181.5 us in a call with 35 repaired chunks.  The gathered family under one body:
// profiles/biquad_one_body.txt.
//
// One task of the speculative pass: chunk k of channel c of a call (C channels, K chunks of L frames, warm-up W) from `sections`,
// forwards or (REV) over the reversed sequence.
template <int S, bool PLANAR, bool REV>
__device__ __forceinline__ void spec_task (const Biquad *sections, int c, int k, int K, int L, int W, const art_s *in, spec_stride<PLANAR> stride, art_s *out,
                                           spec_stride<PLANAR> out_stride, int frames, SpecState *starts, SpecState *ends)
{
    const int first = k * L, last = min (first + L, frames);

    SectionRegs r [S];
#pragma unroll
    for (int s = 0; s < S; ++s) load_section (r [s], sections [(size_t) c * S + s]);

    const int begin = first - S * W;
    if (begin > 0) {
        // speculative start: silence behind every section
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int q = 0; q < 4; ++q) { r [s].x [q] = 0; r [s].y [q] = 0; }
        spec_warm_up<S, PLANAR, REV> (r, in, stride, c, begin, W, frames);
    }
    else if (first > 0)
        // close to the start of the sequence: from the carried-in state through frames [0, first) — exact, nothing stored
        dir_run<S, S, false, PLANAR, REV> (r, in, stride, nullptr, 0, c, 0, first, frames);

    SpecState st [S];
    get_state<S> (st, r);
#pragma unroll
    for (int s = 0; s < S; ++s) starts [((size_t) c * K + k) * S + s] = st [s];

    dir_run<S, S, true, PLANAR, REV> (r, in, stride, out, out_stride, c, first, last, frames);

    get_state<S> (st, r);
#pragma unroll
    for (int s = 0; s < S; ++s) ends [((size_t) c * K + k) * S + s] = st [s];
}

// biquad_check_kernel's body (a copy): one chunk boundary checked.
template <int S>
__device__ __forceinline__ void check_task (int c, int k, int K, const SpecState *starts, const SpecState *ends, unsigned char *bad, int *first_bad)
{
    if (k == 0) return;
    const bool ok = same_state<S> (starts + ((size_t) c * K + k) * S, ends + ((size_t) c * K + k - 1) * S);
    bad [(size_t) c * K + k] = ok ? 0 : 1;
    if (!ok) atomicMin (first_bad + c, k);
}

// The repair loop of one channel from its first mismatch k (biquad_commit_kernel's): every chunk that did not start from the state
// its predecessor left is computed again from that state, until the run rejoins a speculative trajectory.  `en` [K - 1] is the
// channel's exact final state afterwards.
template <int S, bool PLANAR, bool REV>
__device__ __forceinline__ void repair_chunks (SectionRegs *r, int k, int c, int K, int L, const art_s *in, spec_stride<PLANAR> stride, art_s *out,
                                               spec_stride<PLANAR> out_stride, int frames, const SpecState *st, SpecState *en, const unsigned char *flags,
                                               unsigned int *repairs)
{
    unsigned int redone = 0;
    while (k < K) {
        // chunk k again, from the exact state its predecessor left
        put_state<S> (r, en + (size_t)(k - 1) * S);
        const int first = k * L, last = min (first + L, frames);
        dir_run<S, S, true, PLANAR, REV> (r, in, stride, out, out_stride, c, first, last, frames);
        SpecState now [S];
        get_state<S> (now, r);
#pragma unroll
        for (int s = 0; s < S; ++s) en [(size_t) k * S + s] = now [s];
        ++redone;
        if (k + 1 >= K) break;
        if (same_state<S> (now, st + (size_t)(k + 1) * S)) {
            // rejoined the speculative trajectory: everything up to the next recorded mismatch stands
            int next = k + 2;
            while (next < K && !flags [next]) ++next;
            k = next;
        }
        else ++k;
    }
    if (redone) atomicAdd (repairs, redone);
}

// One channel committed in place (bq_clips_commit_kernel): repaired, first_bad re-armed for the next call, and the final state
// stored — the sections read from `from` and stored to `sections`, which the single call reads and stores in one array.
template <int S, bool PLANAR>
__device__ __forceinline__ void commit_channel (const Biquad *from, Biquad *sections, int c, int K, int L, const art_s *in, spec_stride<PLANAR> stride, art_s *out,
                                                spec_stride<PLANAR> out_stride, int frames,
                                                const SpecState *starts, SpecState *ends, const unsigned char *bad, int *first_bad, unsigned int *repairs)
{
    SpecState *en = ends + (size_t) c * K * S;

    SectionRegs r [S];
#pragma unroll
    for (int s = 0; s < S; ++s) load_section (r [s], from [(size_t) c * S + s]);

    const int k = first_bad [c];
    first_bad [c] = INT_MAX;
    repair_chunks<S, PLANAR, false> (r, k, c, K, L, in, stride, out, out_stride, frames, starts + (size_t) c * K * S, en, bad + (size_t) c * K, repairs);

    put_state<S> (r, en + (size_t)(K - 1) * S);
#pragma unroll
    for (int s = 0; s < S; ++s) {
        // store_section, with the index counted on from `from`'s (store_section counts on from the index of the section it writes)
        Biquad &f = sections [(size_t) c * S + s];
        const int i = from [(size_t) c * S + s].index + frames;
#pragma unroll
        for (int k = 0; k < 4; ++k) { f.x [(i - k) & 3] = r [s].x [k]; f.y [(i - k) & 3] = r [s].y [k]; }
        f.index = i;
    }
}

// One channel committed out of place (bq_filter_commit_kernel): repaired only — no state goes back anywhere, and first_bad is not
// re-armed (the next call's spec pass arms its own).
template <int S, bool PLANAR, bool REV>
__device__ __forceinline__ void filter_commit_channel (const Biquad *from, int c, int K, int L, const art_s *in, spec_stride<PLANAR> stride, art_s *out,
                                                       spec_stride<PLANAR> out_stride, int frames,
                                                       const SpecState *starts, SpecState *ends, const unsigned char *bad, const int *first_bad, unsigned int *repairs)
{
    const int k = first_bad [c];
    if (k >= K) return;

    SectionRegs r [S];
#pragma unroll
    for (int s = 0; s < S; ++s) load_section (r [s], from [(size_t) c * S + s]);

    repair_chunks<S, PLANAR, REV> (r, k, c, K, L, in, stride, out, out_stride, frames, starts + (size_t) c * K * S, ends + (size_t) c * K * S, bad + (size_t) c * K, repairs);
}

// ---------------------------------------------------------------------------------------------------
// Many banks' TIME-PARALLEL calls in shared launches (biquadBankApplyClipsPlanarDevice): the passes of biquad_spec_kernel,
// biquad_check_kernel and biquad_commit_kernel over a table of items (ArtBqClip), one item per call.  The task space is the items' (chunk, channel) spaces
// laid end to end; a thread finds its item by binary search over the items' first tasks (item_of) and runs the single call's passes (spec_task, check_task, commit_channel)
// with the item's own C, K, L, W and frames: the chunk cuts, and so the bits, the repairs and the final state, are the single
// call's.  Lanes of different items (different L and K) share a wave.  One instantiation per (section count, layout).
// ---------------------------------------------------------------------------------------------------
template <int S, bool PLANAR>
__global__ __launch_bounds__ (256)
void bq_clips_spec_kernel (const ArtBqClip *items, int n, long tasks)
{
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= tasks) return;
    const ArtBqClip &a = item_of (items, n, task);
    const long t = task - a.task0;
    const int C = a.C, K = a.K;
    const int c = PLANAR ? (int)(t / K) : (int)(t % C), k = PLANAR ? (int)(t % K) : (int)(t / C);
    SpecState *const starts = (SpecState *) a.states, *const ends = starts + (size_t) C * K * S;
    spec_task<S, PLANAR, false> (a.from, c, k, K, a.L, a.W, a.in, (spec_stride<PLANAR>) a.in_stride, a.out, (spec_stride<PLANAR>) a.out_stride, a.frames, starts, ends);
}

template <int S>
__global__ __launch_bounds__ (256)
void bq_clips_check_kernel (const ArtBqClip *items, int n, long tasks)
{
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= tasks) return;
    const ArtBqClip &a = item_of (items, n, task);
    const long t = task - a.task0;
    const int C = a.C, K = a.K;
    SpecState *const starts = (SpecState *) a.states, *const ends = starts + (size_t) C * K * S;
    check_task<S> ((int)(t / K), (int)(t % K), K, starts, ends, (unsigned char *)(ends + (size_t) C * K * S), a.first_bad);
}

// one thread per (item, channel): the item is the last whose first channel (chan0) is not beyond the thread's
template <int S, bool PLANAR>
__global__ __launch_bounds__ (64)
void bq_clips_commit_kernel (const ArtBqClip *items, int n, int channels)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= channels) return;
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items [mid].chan0 <= ch) lo = mid; else hi = mid - 1; }
    const ArtBqClip &a = items [lo];
    const int C = a.C, K = a.K;
    SpecState *const starts = (SpecState *) a.states, *const ends = starts + (size_t) C * K * S;
    commit_channel<S, PLANAR> (a.from, a.sections, ch - a.chan0, K, a.L, a.in, (spec_stride<PLANAR>) a.in_stride, a.out, (spec_stride<PLANAR>) a.out_stride, a.frames,
                               starts, ends, (const unsigned char *)(ends + (size_t) C * K * S), a.first_bad, a.repairs);
}

// ---------------------------------------------------------------------------------------------------
// Whole clips OUT OF PLACE from the banks' first state, forwards or with TIME REVERSED (biquadBankFilterClipsPlanarDevice): the
// gathered passes once more, reading the caller's input where it lies (no set-aside copy) and storing no state back.  REV: frame n
// of the recurrence lives at address frames - 1 - n on both sides, so the item's L, W and K — computed by the host as ever — cut the
// REVERSED sequence where the forward call would cut it, and the arithmetic per frame is the forward call's in the same order.
// From rest, that is the transpose of the forward map (art_hip.h).  The direction is a parameter of run_plane, spec_warm_up,
// spec_task and repair_chunks, and forwards they are the in-place entry's instantiations; dir_run holds the one copy left, the
// reversed interleaved run.
// The check pass has no direction and no buffers: bq_clips_check_kernel is launched as it is.  An item's first_bad lies behind its
// own chunk states and is armed by the spec pass (task k = 0 of every channel), the launch before the check.
// ---------------------------------------------------------------------------------------------------
template <int S, bool PLANAR, bool REV>
__global__ __launch_bounds__ (256)
void bq_filter_spec_kernel (const ArtBqClip *items, int n, long tasks)
{
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= tasks) return;
    const ArtBqClip &a = item_of (items, n, task);
    const long t = task - a.task0;
    const int C = a.C, K = a.K;
    const int c = PLANAR ? (int)(t / K) : (int)(t % C), k = PLANAR ? (int)(t % K) : (int)(t / C);
    SpecState *const starts = (SpecState *) a.states, *const ends = starts + (size_t) C * K * S;
    if (k == 0) a.first_bad [c] = INT_MAX;
    spec_task<S, PLANAR, REV> (a.from, c, k, K, a.L, a.W, a.in, (spec_stride<PLANAR>) a.in_stride, a.out, (spec_stride<PLANAR>) a.out_stride, a.frames, starts, ends);
}

template <int S, bool PLANAR, bool REV>
__global__ __launch_bounds__ (64)
void bq_filter_commit_kernel (const ArtBqClip *items, int n, int channels)
{
    const int ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= channels) return;
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (items [mid].chan0 <= ch) lo = mid; else hi = mid - 1; }
    const ArtBqClip &a = items [lo];
    const int C = a.C, K = a.K;
    SpecState *const starts = (SpecState *) a.states, *const ends = starts + (size_t) C * K * S;
    filter_commit_channel<S, PLANAR, REV> (a.from, ch - a.chan0, K, a.L, a.in, (spec_stride<PLANAR>) a.in_stride, a.out, (spec_stride<PLANAR>) a.out_stride, a.frames,
                                           starts, ends, (const unsigned char *)(ends + (size_t) C * K * S), a.first_bad, a.repairs);
}

// ... and their serial route: the pipeline of biquad_batch_pipe_kernel (bq_pipe_body) over lanes that are read on one side and
// written on the other, from sections that are only read.
template <int S, bool REV>
__global__ __launch_bounds__ (ST_THREADS)
void bq_filter_pipe_kernel (const ArtBqFilterLane *table, int lanes, int chunk_frames)
{
    bq_pipe_body<S, REV> (table, lanes, chunk_frames);
}

// Many strided copies in one launch (the gathered calls' inputs set aside, and banks' sections put back to their first state): item
// = rows of `width` 4-byte words, row starts src_pitch / dst_pitch words apart.  A task is one 16-byte group of a row, counted from
// the 16-byte boundary at or before the row's SOURCE address: whole groups move as one 16-byte access where the destination is on a
// boundary too (the set-aside planes are placed so), the rest word by word.
__global__ __launch_bounds__ (256)
void copy_rows_group_kernel (const ArtCopyRows *items, int n, long tasks)
{
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= tasks) return;
    const ArtCopyRows &a = item_of (items, n, task);
    const long t = task - a.task0, row = t / a.groups, g = t - row * a.groups;
    const unsigned int *const src = a.src + row * a.src_pitch;
    unsigned int *const dst = a.dst + row * a.dst_pitch;
    const long w0 = g * 4 - (long)(((uintptr_t) src >> 2) & 3), width = a.width;
    if (w0 >= 0 && w0 + 4 <= width && !((uintptr_t)(dst + w0) & 15)) {
        *reinterpret_cast<uint4 *> (dst + w0) = *reinterpret_cast<const uint4 *> (src + w0);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (w0 + j >= 0 && w0 + j < width) dst [w0 + j] = src [w0 + j];
}

// one little-endian integer sample (p: its first value byte) times g (reference decimator.c:416-450)
__device__ __forceinline__ art_s decode_pcm (const unsigned char *p, int bits, art_s g)
{
    if (bits <= 8) return (art_s)((int) p [0] - 128) * g;
    if (bits <= 16) return (art_s)(int)(short)(p [0] | (p [1] << 8)) * g;
    return (art_s)(int)((uint32_t) p [0] | ((uint32_t) p [1] << 8) | ((uint32_t)(int)(signed char) p [2] << 16)) * g;
}

__global__ void ingest_kernel (const unsigned char *in, art_s g, int bits, int bytes, int stride, art_s *out, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int width = (bits + 7) / 8;
    out [i] = decode_pcm (in + (size_t) i * stride * bytes + (bytes - width), bits, g);
}

// floatIntegersBatchLEDevice: ingest_kernel over many buffers in one launch.  A thread converts a run of ART_INGEST_RUN consecutive
// samples of one item (16 bytes of output: one store where the address allows it) and finds its item by binary search over the
// items' first tasks, as decimate_batch_parallel_kernel does.  Per sample: ingest_kernel's bytes, casts and one multiply.
__global__ __launch_bounds__ (256)
void ingest_batch_kernel (const ArtIngestItem *items, int n, long tasks)
{
    typedef art_s run_t __attribute__ ((ext_vector_type (ART_INGEST_RUN)));
    const long task = (long) blockIdx.x * blockDim.x + threadIdx.x;
    if (task >= tasks) return;
    const ArtIngestItem &a = item_of (items, n, task);
    const long s0 = (task - a.task0) * ART_INGEST_RUN - a.head;     // first sample of the run (the head run starts before 0)
    const int bits = a.bits, bytes = a.bytes, stride = a.stride, count = a.count;
    const int width = (bits + 7) / 8;
    const unsigned char *const in = a.in + (bytes - width);
    const art_s g = a.gain_factor;
    art_s *const out = a.out;
    run_t v;
#pragma unroll
    for (int j = 0; j < ART_INGEST_RUN; ++j) {
        art_s x = 0;
        if (s0 + j >= 0 && s0 + j < count) x = decode_pcm (in + (size_t)(int)(s0 + j) * stride * bytes, bits, g);
        v [j] = x;
    }
    if (s0 >= 0 && s0 + ART_INGEST_RUN <= count && !((uintptr_t)(out + s0) & 15)) {
        *(run_t *)(out + s0) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < ART_INGEST_RUN; ++j)
        if (s0 + j >= 0 && s0 + j < count) out [s0 + j] = v [j];
}

} // namespace

// The serial stages are latency-bound per lane, so a workgroup gains nothing from more channels — but its LDS chunk (and
// with it the work per barrier) shrinks in proportion.  Many-channel calls are therefore spread over MORE workgroups of
// 8 channels (one per CU and beyond) rather than packed 64 to a workgroup; only beyond 512 workgroups do the groups grow.
static int channels_per_workgroup (int C)
{
    int cpw = 8;
    while (cpw < 64 && (C + cpw - 1) / cpw > 512) cpw += 8;
    return cpw;
}

// Lanes per workgroup of a serial batch class of `lanes` lanes in all: enough workgroups to fill the CUs first, then more lanes per
// serial wave (a lane's time is its chain, whatever the lane count; LDS and helper work grow with the lanes), until the class is
// `workgroups` workgroups.
static int batch_lanes (int lanes, int workgroups)
{
    int L = 1;
    while (L < 64 && (lanes + L - 1) / L > workgroups) L *= 2;
    return L;
}
// Measured (profiles/decimate_batch.txt): the fastest L puts 512-1,024 workgroups on the chip at 2,048, 8,192 and 16,384 lanes,
// and L = 1-2 wins below that.  1,024 is four per CU (a small workgroup's LDS lets several share a CU; their serial waves are
// latency-bound).
static constexpr int DEC_BATCH_WORKGROUPS = 1024;
// Measured (profiles/biquad_batch.txt, ART's post-filter): the fastest L leaves 256-512 workgroups at 2,048, 8,192 and 16,384 lanes,
// where the decimator's 1,024 is 9 % slower at 2,048 lanes; below 512 lanes every L is within a few microseconds of the launch.
static constexpr int BQ_BATCH_WORKGROUPS = 512;

// frames per chunk of a serial batch workgroup of L lanes: the LDS tile's row (a multiple of 4) or `run`, whichever is less
static int batch_chunk_frames (int L, int run) { return min (((DEC_CHUNK / L) - 4) & ~3, run); }

// The decimator kernel of a launch from its shaper order (0: none; above 4 as 4), whether dither is on and whether a side is planar:
// one function per kernel family, the only places that name an instantiation.  The pipelined families' dynamic LDS goes up to
// DEC_PIPE_LDS, past the default limit: that is set the first time an instantiation is handed out.
typedef void (*DecCallKernel) (ArtDecArgs, const art_s *, int, unsigned char *, int, long, long);
typedef void (*DecParallelKernel) (ArtDecTask);
typedef void (*DecBatchPipeKernel) (const ArtDecLane *, int, int);
typedef void (*DecBatchParallelKernel) (const ArtDecTask *, int, long);
static constexpr size_t DEC_PIPE_LDS = (size_t) 5 * DEC_CHUNK * sizeof (art_s);          // three sample tiles, two dither tiles

#define DEC_PICK2(KERNEL) (pitched ? (dither ? KERNEL<true, true> : KERNEL<false, true>) : (dither ? KERNEL<true, false> : KERNEL<false, false>))
#define DEC_PICK3(KERNEL, O) (pitched ? (dither ? KERNEL<O, true, true> : KERNEL<O, false, true>) : (dither ? KERNEL<O, true, false> : KERNEL<O, false, false>))
static DecParallelKernel dec_parallel_kernel (bool dither, bool pitched) { return DEC_PICK2 (decimate_parallel_kernel); }
static DecBatchParallelKernel dec_batch_parallel_kernel (bool dither, bool pitched) { return DEC_PICK2 (decimate_batch_parallel_kernel); }
static DecCallKernel dec_lds_kernel (int order, bool dither, bool pitched)
{
    switch (order) {
        case 0: return DEC_PICK3 (decimate_lds_kernel, 0);
        case 1: return DEC_PICK3 (decimate_lds_kernel, 1);
        case 2: return DEC_PICK3 (decimate_lds_kernel, 2);
        case 3: return DEC_PICK3 (decimate_lds_kernel, 3);
        default: return DEC_PICK3 (decimate_lds_kernel, 4);
    }
}
template <typename Kernel>
static Kernel dec_pipe_lds_allowed (Kernel k, int order, bool dither, bool pitched, bool (&done) [5][2][2])
{
    bool &once = done [order < 0 || order > 4 ? 4 : order][dither][pitched];      // (as the pickers' switches: anything else is 4)
    if (!once) { (void) hipFuncSetAttribute ((const void *) k, hipFuncAttributeMaxDynamicSharedMemorySize, (int) DEC_PIPE_LDS); once = true; }
    return k;
}
static DecCallKernel dec_pipe_kernel (int order, bool dither, bool pitched)               // order >= 1
{
    static bool done [5][2][2];
    DecCallKernel k;
    switch (order) {
        case 1: k = DEC_PICK3 (decimate_pipe_kernel, 1); break;
        case 2: k = DEC_PICK3 (decimate_pipe_kernel, 2); break;
        case 3: k = DEC_PICK3 (decimate_pipe_kernel, 3); break;
        default: k = DEC_PICK3 (decimate_pipe_kernel, 4); break;
    }
    return dec_pipe_lds_allowed (k, order, dither, pitched, done);
}
static DecBatchPipeKernel dec_batch_pipe_kernel (int order, bool dither, bool pitched)
{
    static bool done [5][2][2];
    DecBatchPipeKernel k;
    switch (order) {
        case 0: k = DEC_PICK3 (decimate_batch_pipe_kernel, 0); break;
        case 1: k = DEC_PICK3 (decimate_batch_pipe_kernel, 1); break;
        case 2: k = DEC_PICK3 (decimate_batch_pipe_kernel, 2); break;
        case 3: k = DEC_PICK3 (decimate_batch_pipe_kernel, 3); break;
        default: k = DEC_PICK3 (decimate_batch_pipe_kernel, 4); break;
    }
    return dec_pipe_lds_allowed (k, order, dither, pitched, done);
}
// the clips entry's kernels
typedef void (*DecClipsPipeKernel) (const ArtDecClipLane *, int, int);
typedef void (*DecClipsParallelKernel) (const ArtDecClipTask *, int, long);
static DecClipsParallelKernel dec_clips_parallel_kernel (bool dither)
{
    return dither ? decimate_clips_parallel_kernel<true> : decimate_clips_parallel_kernel<false>;
}
#define DEC_PICK_CLIPS(O) (dither ? decimate_clips_pipe_kernel<O, true> : decimate_clips_pipe_kernel<O, false>)
static DecClipsPipeKernel dec_clips_pipe_kernel (int order, bool dither)
{
    static bool done [5][2][2];
    DecClipsPipeKernel k;
    switch (order) {
        case 0: k = DEC_PICK_CLIPS (0); break;
        case 1: k = DEC_PICK_CLIPS (1); break;
        case 2: k = DEC_PICK_CLIPS (2); break;
        case 3: k = DEC_PICK_CLIPS (3); break;
        default: k = DEC_PICK_CLIPS (4); break;
    }
    return dec_pipe_lds_allowed (k, order, dither, true, done);
}
#undef DEC_PICK_CLIPS
#undef DEC_PICK3
#undef DEC_PICK2

// The time-parallel bit-exact cascade (biquad_spec_kernel), the one body of arthip_biquad_spec (strides) and arthip_biquad_spec_planar
// (pitches)
template <bool PLANAR>
static int biquad_spec_launch (Biquad *d_sections, int C, int S, const art_s *d_in, spec_stride<PLANAR> in_stride, art_s *d_out, spec_stride<PLANAR> out_stride,
                               int frames, int L, int W, void *d_states, int *d_first_bad, unsigned int *d_repairs, void *stream)
{
    if (frames <= 0) return 0;
    if (S < 1 || S > MAX_CHAIN || L < 1) return -1;
    const int K = (frames + L - 1) / L;
    SpecState *starts = (SpecState *) d_states, *ends = starts + (size_t) C * K * S;
    unsigned char *bad = (unsigned char *)(ends + (size_t) C * K * S);
    const long tasks = (long) C * K;
    const dim3 grid ((unsigned int)((tasks + 255) / 256)), block (256);
    hipStream_t st = (hipStream_t) stream;
#define SPEC_GO(SS) do { \
        hipLaunchKernelGGL ((biquad_spec_kernel<SS, PLANAR>), grid, block, 0, st, (const Biquad *) d_sections, C, K, L, W, d_in, in_stride, d_out, out_stride, frames, starts, ends); \
        hipLaunchKernelGGL (biquad_check_kernel<SS>, grid, block, 0, st, C, K, (const SpecState *) starts, (const SpecState *) ends, bad, d_first_bad); \
        hipLaunchKernelGGL ((biquad_commit_kernel<SS, PLANAR>), dim3 ((C + 63) / 64), dim3 (64), 0, st, d_sections, C, K, L, d_in, in_stride, d_out, out_stride, frames, \
                            (const SpecState *) starts, ends, (const unsigned char *) bad, d_first_bad, d_repairs); } while (0)
    switch (S) { case 1: SPEC_GO (1); break; case 2: SPEC_GO (2); break; case 3: SPEC_GO (3); break; default: SPEC_GO (4); }
#undef SPEC_GO
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

// kernel<1 .. 4, ...> by the section count
#define BQ_PICK_S(S, kernel, ...) ((S) == 1 ? kernel<1, ##__VA_ARGS__> : (S) == 2 ? kernel<2, ##__VA_ARGS__> : (S) == 3 ? kernel<3, ##__VA_ARGS__> : kernel<4, ##__VA_ARGS__>)

// one launch of one serial class from its slice of the uploaded table: lanes, LDS and grid for either pipe kernel
template <typename Lane>
static int bq_pipe_launch (void (*kernel) (const Lane *, int, int), const ArtBqClass *cls, const void *d_table, void *stream)
{
    const Lane *items = (const Lane *)((const char *) d_table + cls->slice.offset);
    const int L = cls->slice.lanes;
    if (cls->slice.count <= 0) return 0;
    if (L < 1 || L > 64 || cls->slice.count % L || cls->S < 1 || cls->S > 4) return -1;
    const int chunk_frames = batch_chunk_frames (L, BQ_BATCH_RUN);
    const size_t lds = (size_t) 3 * L * (chunk_frames + 4) * sizeof (art_s);          // <= 3 DEC_CHUNK samples (48 KiB)
    hipLaunchKernelGGL (kernel, dim3 ((unsigned int)(cls->slice.count / L)), dim3 (ST_THREADS), lds, (hipStream_t) stream, items, L, chunk_frames);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

// the three launches of one (section count, layout) class of gathered time-parallel calls, from its slice of the uploaded table:
// the entry's spec kernel, the check pass (it has no layout and no direction) and the entry's commit kernel
static int bq_clips_launch (void (*spec) (const ArtBqClip *, int, long), void (*commit) (const ArtBqClip *, int, int), const ArtBqClipClass *cls,
                            const void *d_table, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    const ArtBqClip *items = (const ArtBqClip *)((const char *) d_table + cls->offset);
    const int n = cls->count, channels = cls->channels;
    const long tasks = cls->tasks;
    if (n <= 0) return 0;
    if (cls->S < 1 || cls->S > MAX_CHAIN || tasks <= 0 || channels <= 0) return -1;
    const dim3 grid ((unsigned int)((tasks + 255) / 256)), block (256);
    hipLaunchKernelGGL (spec, grid, block, 0, st, items, n, tasks);
    hipLaunchKernelGGL (BQ_PICK_S (cls->S, bq_clips_check_kernel), grid, block, 0, st, items, n, tasks);
    hipLaunchKernelGGL (commit, dim3 ((unsigned int)((channels + 63) / 64)), dim3 (64), 0, st, items, n, channels);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

extern "C" {

// The time-parallel bit-exact cascade (biquad_spec_kernel): `d_in` -> `d_out` (distinct buffers), frames x C with the given
// strides; W = warm-up frames per section (host: decay of the recursive part), L = chunk length.  d_states: scratch of
// arthip_biquad_spec_scratch (C, S, frames, L) bytes.  d_repairs: device counter (chunks that had to be recomputed).
size_t arthip_biquad_spec_scratch (int C, int S, int frames, int L)
{
    const size_t K = (size_t)((frames + L - 1) / L);
    return (size_t) C * K * S * sizeof (SpecState) * 2 + (((size_t) C * K + 255) & ~(size_t) 255);
}

// d_first_bad: C ints of device memory that hold a value beyond any chunk count between calls (armed once, here)
int arthip_biquad_spec_arm (int *d_first_bad, int C, void *stream)
{
    return hipMemsetAsync (d_first_bad, 0x7f, sizeof (int) * (size_t) C, (hipStream_t) stream) == hipSuccess ? 0 : -1;     // 0x7f7f7f7f
}

int arthip_biquad_spec (Biquad *d_sections, int C, int S, const art_s *d_in, int in_stride, art_s *d_out, int out_stride, int frames,
                        int L, int W, void *d_states, int *d_first_bad, unsigned int *d_repairs, void *stream)
{
    return biquad_spec_launch<false> (d_sections, C, S, d_in, in_stride, d_out, out_stride, frames, L, W, d_states, d_first_bad, d_repairs, stream);
}

int arthip_biquad_spec_planar (Biquad *d_sections, int C, int S, const art_s *d_in, long in_pitch, art_s *d_out, long out_pitch, int frames,
                               int L, int W, void *d_states, int *d_first_bad, unsigned int *d_repairs, void *stream)
{
    return biquad_spec_launch<true> (d_sections, C, S, d_in, in_pitch, d_out, out_pitch, frames, L, W, d_states, d_first_bad, d_repairs, stream);
}

int arthip_biquad_order2 (Biquad *d_sections, int C, int S, art_s *d_buf, int frames, int stride, void *stream)
{
    if (frames <= 0) return 0;
    if (S == 1 || S == 2) {
        const size_t lds = (size_t) 9 * FF_CAP * sizeof (art_s) + 256;           // 108 KiB of the CU's 160 (+ look-ahead slack)
        static bool once = false;
        if (!once) {
            (void) hipFuncSetAttribute ((const void *) biquad_order2_ff_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
            (void) hipFuncSetAttribute ((const void *) biquad_order2_ff_kernel<2>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
            once = true;
        }
        const int cpw = channels_per_workgroup (C);
        const dim3 grid ((C + cpw - 1) / cpw);
        if (S == 1) hipLaunchKernelGGL (biquad_order2_ff_kernel<1>, grid, dim3 (ST_THREADS), lds, (hipStream_t) stream, d_sections, C, stride, d_buf, frames, cpw);
        else hipLaunchKernelGGL (biquad_order2_ff_kernel<2>, grid, dim3 (ST_THREADS), lds, (hipStream_t) stream, d_sections, C, stride, d_buf, frames, cpw);
    }
    else return -1;
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

int arthip_biquad_chain (Biquad *d_sections, int C, int S, art_s *d_buf, int frames, int stride, void *stream)
{
    if (S < 1 || S > MAX_CHAIN || frames <= 0) return S < 1 || S > MAX_CHAIN ? -1 : 0;
    const int sample_form = stride < 0;                  // negative stride selects the per-sample association
    if (sample_form) stride = -stride;
    if (!sample_form && stride == C && frames >= 64) {   // interleaved frames: LDS-staged form
        hipLaunchKernelGGL (biquad_chain_lds_kernel, dim3 ((C + 63) / 64), dim3 (ST_THREADS), 0, (hipStream_t) stream, d_sections, C, S, d_buf, frames);
        return hipGetLastError () == hipSuccess ? 0 : -1;
    }
    hipLaunchKernelGGL (biquad_chain_kernel, dim3 ((C + 63) / 64), dim3 (64), 0, (hipStream_t) stream, d_sections, C, S, d_buf, frames, stride, sample_form);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

static int decimate_launch (const ArtDecArgs *a, const art_s *d_in, long in_pitch, int frames, unsigned char *d_out, long out_pitch, void *stream)
{
    if (frames <= 0) return 0;
    hipLaunchKernelGGL (decimate_kernel, dim3 ((a->C + 63) / 64), dim3 (64), 0, (hipStream_t) stream, *a, d_in, in_pitch, frames, d_out, out_pitch);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

// in_pitch / out_pitch: samples / bytes between the planes of that side, 0: that side is interleaved.  The kernel is chosen as for
// the interleaved call; with a pitch on either side it is that kernel's PITCHED instantiation.
int arthip_decimate_pitched (const ArtDecArgs *a, const art_s *d_in, long in_pitch, int frames, unsigned char *d_out, long out_pitch, void *stream)
{
    const bool pitched = in_pitch || out_pitch, dither = a->dither_on != 0;
    hipStream_t st = (hipStream_t) stream;
    if (frames >= 64 && !a->shaping_on && (!dither || a->gens_next) && (DEC_SEG % 2) == 0) {
        const long tasks = (long) a->C * ((frames + DEC_SEG - 1) / DEC_SEG);
        ArtDecTask item;                                       // the call as the batch's table would hold it: one item, first task 0
        item.in = d_in; item.out = d_out; item.in_pitch = in_pitch; item.out_pitch = out_pitch; item.frames = frames; item.task0 = 0;
        item.feedback = a->feedback; item.gens = a->gens; item.gens_next = a->gens_next; item.clipped = a->clipped;
        item.scale = a->scale; item.C = a->C; item.bits = a->bits; item.bytes = a->bytes; item.dither_type = a->dither_type;
        hipLaunchKernelGGL (dec_parallel_kernel (dither, pitched), dim3 ((unsigned int)((tasks + 255) / 256)), dim3 (256), 0, st, item);
        return hipGetLastError () == hipSuccess ? 1 : -1;      // 1: generator state now lives in gens_next
    }
    if (frames >= 64) {
        const int cpw = channels_per_workgroup (a->C);
        const dim3 grid ((a->C + cpw - 1) / cpw), block (ST_THREADS);
        const int order = a->shaping_on ? a->shaping_order : 0;
        // with more workgroups than CUs the chip is busy anyway and the smaller LDS footprint of the unpipelined form
        // (more workgroups per CU) wins: 4,096 channels 49 vs 36 Gsamples/s
        if (order >= 1 && grid.x <= 256)
            hipLaunchKernelGGL (dec_pipe_kernel (order, dither, pitched), grid, block, DEC_PIPE_LDS, st, *a, d_in, frames, d_out, cpw, in_pitch, out_pitch);
        else
            hipLaunchKernelGGL (dec_lds_kernel (order, dither, pitched), grid, block, 0, st, *a, d_in, frames, d_out, cpw, in_pitch, out_pitch);
        return hipGetLastError () == hipSuccess ? 0 : -1;
    }
    return decimate_launch (a, d_in, in_pitch, frames, d_out, out_pitch, stream);
}

int arthip_decimate (const ArtDecArgs *a, const art_s *d_in, int frames, unsigned char *d_out, void *stream)
{
    return arthip_decimate_pitched (a, d_in, 0, frames, d_out, 0, stream);
}

int arthip_decimate_planar (const ArtDecArgs *a, const art_s *d_in, long in_pitch, int frames, unsigned char *d_out, long out_pitch, void *stream)
{
    return decimate_launch (a, d_in, in_pitch, frames, d_out, out_pitch, stream);
}

int arthip_decimate_batch_lanes (int lanes) { return batch_lanes (lanes, DEC_BATCH_WORKGROUPS); }

int arthip_decimate_batch_launch (const ArtDecClass *cls, const void *d_table, void *stream)
{
    hipStream_t st = (hipStream_t) stream;
    const void *items = (const char *) d_table + cls->slice.offset;
    if (cls->slice.count <= 0) return 0;
    if (!cls->serial) {
        const dim3 grid ((unsigned int)((cls->tasks + 255) / 256));
        if (cls->clips)
            hipLaunchKernelGGL (dec_clips_parallel_kernel (cls->dither != 0), grid, dim3 (256), 0, st, (const ArtDecClipTask *) items, cls->slice.count, cls->tasks);
        else
            hipLaunchKernelGGL (dec_batch_parallel_kernel (cls->dither != 0, cls->pitched != 0), grid, dim3 (256), 0, st,
                                (const ArtDecTask *) items, cls->slice.count, cls->tasks);
        return hipGetLastError () == hipSuccess ? 0 : -1;
    }
    const int L = cls->slice.lanes;
    if (L < 1 || L > 64 || cls->slice.count % L) return -1;
    const int chunk_frames = batch_chunk_frames (L, DEC_BATCH_RUN);
    const size_t lds = (size_t) 5 * L * (chunk_frames + 4) * sizeof (art_s);          // <= DEC_PIPE_LDS (80 KiB)
    if (cls->clips) {
        hipLaunchKernelGGL (dec_clips_pipe_kernel (cls->order, cls->dither != 0), dim3 ((unsigned int)(cls->slice.count / L)), dim3 (ST_THREADS), lds, st,
                            (const ArtDecClipLane *) items, L, chunk_frames);
        return hipGetLastError () == hipSuccess ? 0 : -1;
    }
    hipLaunchKernelGGL (dec_batch_pipe_kernel (cls->order, cls->dither != 0, cls->pitched != 0), dim3 ((unsigned int)(cls->slice.count / L)), dim3 (ST_THREADS), lds, st,
                        (const ArtDecLane *) items, L, chunk_frames);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

int arthip_biquad_batch_lanes (int lanes) { return batch_lanes (lanes, BQ_BATCH_WORKGROUPS); }

int arthip_biquad_batch_launch (const ArtBqClass *cls, const void *d_table, void *stream)
{
    return bq_pipe_launch<ArtBqLane> (BQ_PICK_S (cls->S, biquad_batch_pipe_kernel), cls, d_table, stream);
}

// ... and of one serial class of the out-of-place entry (ArtBqFilterLane lanes)
int arthip_biquad_filter_batch_launch (const ArtBqClass *cls, const void *d_table, int reversed, void *stream)
{
    return bq_pipe_launch<ArtBqFilterLane> (reversed ? BQ_PICK_S (cls->S, bq_filter_pipe_kernel, true) : BQ_PICK_S (cls->S, bq_filter_pipe_kernel, false), cls, d_table, stream);
}

int arthip_biquad_clips_launch (const ArtBqClipClass *cls, const void *d_table, void *stream)
{
    if (cls->planar) return bq_clips_launch (BQ_PICK_S (cls->S, bq_clips_spec_kernel, true), BQ_PICK_S (cls->S, bq_clips_commit_kernel, true), cls, d_table, stream);
    return bq_clips_launch (BQ_PICK_S (cls->S, bq_clips_spec_kernel, false), BQ_PICK_S (cls->S, bq_clips_commit_kernel, false), cls, d_table, stream);
}

// the same three launches out of place and with a direction (biquadBankFilterClipsPlanarDevice): the spec pass arms the items' flags
int arthip_biquad_filter_clips_launch (const ArtBqClipClass *cls, const void *d_table, int reversed, void *stream)
{
#define FILTER_GO(PL, RV) bq_clips_launch (BQ_PICK_S (cls->S, bq_filter_spec_kernel, PL, RV), BQ_PICK_S (cls->S, bq_filter_commit_kernel, PL, RV), cls, d_table, stream)
    if (cls->planar) return reversed ? FILTER_GO (true, true) : FILTER_GO (true, false);
    return reversed ? FILTER_GO (false, true) : FILTER_GO (false, false);
#undef FILTER_GO
}

// one launch of `n` strided copies (`tasks`: the sum of rows * groups over the items) from the uploaded table
int arthip_copy_rows_launch (const void *d_items, int n, long tasks, void *stream)
{
    if (n <= 0 || tasks <= 0) return 0;
    hipLaunchKernelGGL (copy_rows_group_kernel, dim3 ((unsigned int)((tasks + 255) / 256)), dim3 (256), 0, (hipStream_t) stream, (const ArtCopyRows *) d_items, n, tasks);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

int arthip_ingest (const unsigned char *d_in, art_s g, int bits, int bytes, int stride, art_s *d_out, int n, void *stream)
{
    if (n <= 0) return 0;
    hipLaunchKernelGGL (ingest_kernel, dim3 ((n + 255) / 256), dim3 (256), 0, (hipStream_t) stream, d_in, g, bits, bytes, stride, d_out, n);
    return hipGetLastError () == hipSuccess ? 0 : -1;
}

// The ingest batch has no context to keep its table in: each calling thread keeps one in device memory.  `ev` marks the last launch
// that read it; a call on another stream than that launch's waits for it on the device before the table is rewritten.  Like the
// pinned staging (device_rt.hip), the table and event live as long as the process: a thread that ends leaves its table behind (one
// allocation of at most twice its largest call's table), so a service calls from long-lived threads.
struct IngestTable { void *d; size_t cap; int device; hipEvent_t ev; hipStream_t last; bool used; };

int arthip_ingest_batch (const ArtIngestItem *items, int n, long tasks, void *stream)
{
    static thread_local IngestTable t = { nullptr, 0, -1, nullptr, nullptr, false };
    hipStream_t st = (hipStream_t) stream;
    const size_t bytes = sizeof (ArtIngestItem) * (size_t) n;
    int device = 0;
    if (n <= 0 || tasks <= 0) return 0;
    if (hipGetDevice (&device) != hipSuccess) return -1;
    if (t.device != device || bytes > t.cap) {
        if (t.used) (void) hipEventSynchronize (t.ev);
        if (t.d) (void) hipFree (t.d);
        if (t.ev && t.device != device) { (void) hipEventDestroy (t.ev); t.ev = nullptr; }
        t.d = nullptr; t.cap = 0; t.used = false; t.device = device;
        if (!t.ev && hipEventCreateWithFlags (&t.ev, hipEventDisableTiming) != hipSuccess) { t.ev = nullptr; return -1; }
        const size_t cap = bytes * 2 > 4096 ? bytes * 2 : 4096;
        if (hipMalloc (&t.d, cap) != hipSuccess) { t.d = nullptr; return -1; }
        t.cap = cap;
    }
    if (t.used && t.last != st && hipStreamWaitEvent (st, t.ev, 0) != hipSuccess) return -1;
    if (arthip_table_upload (items, bytes, t.d, st)) return -1;
    hipLaunchKernelGGL (ingest_batch_kernel, dim3 ((unsigned int)((tasks + 255) / 256)), dim3 (256), 0, st, (const ArtIngestItem *) t.d, n, tasks);
    if (hipGetLastError () != hipSuccess) return -1;
    // (the table may be rewritten only after this launch: if the event cannot be recorded, wait for the stream instead)
    if (hipEventRecord (t.ev, st) != hipSuccess) { t.used = false; return hipStreamSynchronize (st) == hipSuccess ? 0 : -1; }
    t.last = st; t.used = true;
    return 0;
}

}
