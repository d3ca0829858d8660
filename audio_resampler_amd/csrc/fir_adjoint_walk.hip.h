#pragma once
// fir_adjoint_walk.hip.h — the chunk walk of the gather adjoints (gfx950): fir_adjoint.hip's blocks kernel and fir_sample.hip's two adjoints share
// this one copy, each with its own source of output positions: adj_walk asks adj_locate<INTERP> (rate, segs, n), an overload set — the one
// below for a planned phase, fir_sample.hip's for an entry of a position array (found at instantiation, through its argument types).  With the
// source as a pair of operands passed on as locate ()'s were, fir_adjoint.hip's device code is what it was before the walk moved here,
// instruction for instruction in both widths (a functor that holds the pair moved one conversion and renumbered a scalar register in the
// blocks kernel's eight instantiations).  Compiled with -ffp-contract=off, as both are.
#include "fir_common.hip.h"

namespace {

constexpr int ADJ_TILE = 256;            // input frames per workgroup = its threads
constexpr int ADJ_CHUNK = 256;           // outputs per trip through the LDS
constexpr int ADJ_UNROLL = 4;            // outputs whose coefficient loads are in flight together
static_assert (ADJ_CHUNK % ADJ_UNROLL == 0, "whole groups per chunk");

// the position source of a planned phase: the forward's own locate () on the phase's ratio and segments
template <bool INTERP>
__device__ __forceinline__ Pos adj_locate (const AdjRate &rate, const AdjSegs &segs, unsigned int n) { return locate<INTERP> (rate, segs, n); }

// the one bank of an unbanded walk: a planned item's, or rung 0 of a curve item's ladder (its only rung there) — settled at compile time
template <typename Item>
__device__ __forceinline__ const art_s *adj_bank (const Item &it) { return it.bank; }
__device__ __forceinline__ const art_s *adj_bank (const ArtSampleItem &it) { return it.bank [0]; }

// One phase's share of a lane's sum: the outputs [n_begin, n_end) of the phase (g0: its first output among the clip's), whose windows may hold the
// lane's frame at linear index `lin` of the phase's space (live: the lane has a frame there at all), in chunks of ADJ_CHUNK through the LDS.
// Every thread of the workgroup calls it with the same range.  adj_locate<INTERP> (rate, segs, n) is output n's Pos, ip in the space `lin`
// lives in.  It is fir_adjoint_kernel's chunk loop line for line, and written so that that
// kernel could call it too (Item: ArtAdjItem, ArtAdjBlocksItem or ArtSampleItem — bank, gy, gy_pitch, gy_frames, C, T, F, lowpass); it does not, because with
// the call in place the compiler allocates that kernel's registers differently (1-3 SGPRs more in thirteen of the sixteen
// instantiations, +-2 VGPRs in three: profiles/clip_warp.txt), and the two-phase kernel keeps the code object it was measured with.
// A change to the arithmetic is made in both places; tests/test_gpu_clip_warp.py holds the two kernels to the same bits on one-block
// clips.
// BAND (fir_sample.hip's banded adjoint; INTERP only): the item holds a ladder of banks of one shape, it.bank [0 .. K), and adj_level (segs, n, rung, lam) gives
// output n's rung L and blend lam: its weight is rung L's where lam == 0 — the line below, on that bank — and elsewhere
// (art_s)(w_L * (1.0 - lam) + w_{L+1} * lam) with w_k = h0 * f0 + h1 * f1 of rung k unrounded, in double.  Two more rows of the chunk in the
// LDS (s_rung, s_lam).  Without BAND nothing of this is compiled: the other instantiations are what they were.
template <int CG, bool INTERP, bool BAND = false, typename Item, typename Rate, typename Segs>
__device__ __forceinline__ void adj_walk (art_s (&acc) [CG], const Item &it, const Rate &rate, const Segs &segs, int ch0, int tid, int lin, bool live,
                                          unsigned int g0, int n_begin, int n_end, int *s_w, int *s_row, int *s_pass, double *s_f0, double *s_f1, art_s *s_gy,
                                          int *s_rung = nullptr, double *s_lam = nullptr)
{
    static_assert (INTERP || !BAND, "a ladder is blended on interpolating banks only");
    const art_s *bank = nullptr;
    if constexpr (!BAND) bank = adj_bank (it);
    const int T = it.T, half = T / 2;

    for (int n0 = n_begin; n0 < n_end; n0 += ADJ_CHUNK) {
        const int cnt = min (ADJ_CHUNK, n_end - n0);
        __syncthreads ();                          // (the chunk before is done with)
        if (tid < cnt) {
            const Pos pos = adj_locate<INTERP> (rate, segs, (unsigned int)(n0 + tid));
            s_w [tid] = pos.ip - half + 1;
            s_row [tid] = pos.fi * T;
            if constexpr (BAND) adj_level (segs, (unsigned int)(n0 + tid), s_rung [tid], s_lam [tid]);
            if constexpr (INTERP) { s_f0 [tid] = 1.0 - pos.frac; s_f1 [tid] = pos.frac; }
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
            if constexpr (BAND) {
                // (what a group's outputs ask is the same for every lane: a group on whole rungs loads what the unbanded walk loads)
                bool blend = false;
#pragma unroll
                for (int u = 0; u < ADJ_UNROLL; ++u) blend = blend || (i0 + u < cnt && s_lam [i0 + u] != 0.0);
#pragma unroll
                for (int u = 0; u < ADJ_UNROLL; ++u) {
                    const int rung = i0 + u < cnt ? s_rung [i0 + u] : 0;
                    const double lam = i0 + u < cnt ? s_lam [i0 + u] : 0.0;
                    const art_s *h = it.bank [rung] + at [u];
                    const double left = (double) h [0] * s_f0 [i0 + u], right = (double) h [T] * s_f1 [i0 + u];
                    double v = left + right;
                    if (blend) {
                        const art_s *g = it.bank [lam != 0.0 ? rung + 1 : rung] + at [u];
                        const double left1 = (double) g [0] * s_f0 [i0 + u], right1 = (double) g [T] * s_f1 [i0 + u];
                        const double lower = v * (1.0 - lam), upper = (left1 + right1) * lam;
                        if (lam != 0.0) v = lower + upper;
                    }
                    w [u] = ok [u] ? (art_s) v : (art_s) 0;
                }
            }
            else {
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
            }
#pragma unroll
            for (int u = 0; u < ADJ_UNROLL; ++u)
#pragma unroll
                for (int c = 0; c < CG; ++c) acc [c] = fused (w [u], s_gy [(i0 + u) * CG + c], acc [c]);
        }
    }
}

} // namespace
