"""Helper of test_gpu_general_pipe.py: plays fixed sessions through the GENERAL kernel (kernel preference 1) on two twin contexts in
one process and prints one sha256 per session and twin.  One twin makes single calls (resampleProcessInterleavedDevice: the pipelined
or lean tap loop, whichever the host picks for the shape); the other makes every call as a batch of one
(resampleProcessBatchInterleavedDevice: fir_general_batch_kernel, which runs the plain loop for every shape).  Both twins make the
same calls: a free-ratio stream's positions depend on where its calls begin, so only equal cuts can leave equal bits."""
import ctypes as C
import hashlib, json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import audio_resampler_amd as A
from audio_resampler_amd.api import ArtamdPosition, ArtamdSegment, ResampleResult, process_batch_device
from _hip import HipResampler
from _oracle import noise, BH, INTERP, LOWPASS, PRECISE

SESSIONS = [
    # (channels, taps, filters, ratio, flags, blocks)
    (8, 988, 988, 48000 / 44100, BH | INTERP, (30000, 4096, 1000, 17, 9000)),
    (4, 1024, 256, 44100 / 48000 * 1.0001, BH | INTERP, (20000, 5000)),
    (5, 988, 988, 1.37, BH | INTERP, (12000, 3000)),                       # five channels: a column group of eight, three idle
    (8, 988, 32, 2.0, BH, (9000, 2000)),                                   # nearest filter without a low-pass: pass-through outputs among the others
    (8, 600, 600, 0.731, BH, (16000, 800)),
    (16, 512, 512, 48000 / 44100, BH | INTERP | PRECISE, (6000, 2500)),    # double accumulators
    (32, 988, 988, 0.5, BH | INTERP, (5000, 1200)),
    (8, 1024, 64, 1.25, BH | INTERP, (8000, 3000)),                        # the longest filter: two full rounds of taps per output
]


def pieces(n, T):
    """a block of n frames as calls of at most 45 T frames: the ring rewinds every 15 T frames, so such a call has at most four
    ring-epoch segments — as many as a batched call may have (fir_general.hip, BATCH_SEGS).  Longer calls the batch hands back
    to the single-call path, and the twins would compare a loop with itself."""
    step = 45 * T
    return [min(step, n - k) for k in range(0, n, step)]


def segments(r, n, cap, ratio):
    """(ring-epoch segments, input used, outputs made) of the call the context r is about to make, planned as the batch plans it"""
    c = r.c
    pos = ArtamdPosition(c.numTaps, c.numFilters, c.flags, c.inputIndex, 0, c.outputOffset, c.fixedRatio)     # (floorActive: only a flush sets it)
    res, segs, floor = ResampleResult(), (ArtamdSegment * 64)(), C.c_int()
    nseg = A.lib().artamdPlanCall(C.byref(pos), n, cap, ratio, C.byref(res), segs, 64, C.byref(floor))
    return nseg, res.input_used, res.output_generated


def tile_of(T, ch, ratio, outputs):
    """(column group, outputs per workgroup tile, outputs per pass of its four waves) of a single call's general-kernel launch:
    fir_general.hip's general_geometry restated (one launch in the grid).  A tile of more than one pass has each wave walk
    several outputs — the later ones' coefficients loaded inside the loop, not ahead of the staging."""
    cg = 8 if ch > 4 else 4 if ch > 2 else 2 if ch == 2 else 1
    one_pass = 4 * (64 // (16 if T <= 512 else 32))
    tile = min(math.floor((65536 // (4 * cg) - T - 3) * ratio), 48)
    if tile > one_pass:
        k = tile // one_pass
        while k > 1 and -(-outputs // (k * one_pass)) < 1024:
            k -= 1
        tile = k * one_pass
    return cg, max(tile, 1), one_pass


def play(ch, T, F, flags, pref, x, calls):
    """calls: [(frames, ratio), ...] over the input x [frames, ch].  Returns [single, batched], each {"frames", "sha256", "calls",
    "form": [column group, interpolating, double accumulators], "pass": outputs per pass, "tiles": the single calls' tile sizes}."""
    single, batched = HipResampler(ch, T, F, 0.0, flags, kernel=pref), HipResampler(ch, T, F, 0.0, flags, kernel=1)
    # The batch hands a call back to the single-call path, silently, for a strict-order, extrapolating or flushed context, a
    # sharded one (ARTAMD_SHARDS) or one with timing on — the twins would then compare a loop with itself.  (The contexts'
    # own flags: ARTAMD_STRICT sets the strict order at creation.)
    for r in (single, batched):
        assert not r.c.flags & (A.RESAMPLE_STRICT_ORDER | A.EXTRAPOLATE_ENDPOINTS | A.RESAMPLER_FLUSHED), r.c.flags
        assert r.shards() == [], r.shards()
    max_segs = A.lib().arthip_fir_batch_max_segments()
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    hashes, made, tiles = [hashlib.sha256(), hashlib.sha256()], [0, 0], set()
    for r in (single, batched):
        r.advance(T / 2)
    pos = 0
    for n, ratio in calls:
        cap = int(n * ratio) + 4000
        d_in = d_x[pos:pos + n]
        nseg, used, planned = segments(batched, n, cap, ratio)
        assert nseg <= max_segs and planned > 0, (n, nseg, planned)          # (so the batch gathers the call: it runs on the batch kernel)
        d_out = [torch.empty(cap, ch, device="cuda") for _ in range(2)]
        u, g = single.process_device(d_in, n, d_out[0], cap, ratio)
        assert u == n and single.last_kernel() == 1, (u, n, single.last_kernel())
        [(ub, gb)] = process_batch_device([batched], [d_in], [n], [d_out[1]], [cap], [ratio])
        assert (ub, gb) == (used, planned) == (u, g) and batched.last_kernel() == 1, ((ub, gb), (used, planned), (u, g))
        for k, gk in enumerate((g, gb)):
            hashes[k].update(d_out[k][:gk].cpu().numpy().tobytes()); made[k] += gk
        cg, tile, one_pass = tile_of(T, ch, ratio, g)
        tiles.add(tile)
        pos += n
    form = [cg, bool(flags & A.SUBSAMPLE_INTERPOLATE), bool(flags & A.EXTEND_CONVOLUTION_MATH)]
    return [{"frames": m, "sha256": h.hexdigest(), "calls": len(calls), "form": form, "pass": one_pass, "tiles": sorted(tiles)}
            for m, h in zip(made, hashes)]


def main():
    out = {"single": [], "batched": []}
    for ch, T, F, ratio, flags, blocks in SESSIONS:
        x, _ = noise(sum(blocks) * ch, state=(ch * 1000 + T) | 1)
        calls = [(p, ratio) for n in blocks for p in pieces(n, T)]
        for side, rec in zip(("single", "batched"), play(ch, T, F, flags, 1, x.reshape(-1, ch), calls)):
            out[side].append({"session": [ch, T, F, ratio], **rec})
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())
