"""The yardstick of the clip warper's tests: the dense operator A of a whole clip made block by block (fresh context, a process call per
block at the block's ratio, the flush with the last), built from the CPU oracle alone — one unit impulse per input frame through the
strict oracle, a reset in between.  A [n, j] is the oracle's weight of output n on input j, whichever block made n.  Built once per shape
and shared (callers must not write into what they get); the sums and the ulp come from _adjoint_ref.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

import _oracle as O
from _adjoint_ref import expected_gradient, ulp_of  # noqa: F401


def _run(r, taps, x, blocks, ratios):
    """the clip x [frames, 1] through oracle r block by block -> (outputs per block (the flush's with the last), y [M])"""
    r.reset()
    at, made, parts = 0, [], []
    for k, (n, ratio) in enumerate(zip(blocks, ratios)):
        last = k == len(blocks) - 1
        cap = int((n + taps + 2) * ratio) + 64
        used, got, y = r.process(x[at:at + n], cap, float(ratio), and_flush=last)
        assert used == n and got < cap, (k, used, n, got, cap)
        at += n
        made.append(got)
        parts.append(y[:, 0].astype(np.float64))
    return made, np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def dense_operator(taps, filters, flags, blocks, ratios, lowpass_ratio=0.0, width=32):
    """(A as float64 [M, sum(blocks)], outputs per block) for `blocks` (frames of every block, a tuple) at `ratios` (a tuple)"""
    B = O.binding(width)
    smp = np.float64 if width == 64 else np.float32
    r = B.OracleResampler(1, taps, filters, lowpass_ratio, flags, kind="strict")
    frames = int(sum(blocks))
    per_block, zero = _run(r, taps, np.zeros((frames, 1), smp), blocks, ratios)
    assert not zero.any()
    cols = []
    for j in range(frames):
        e = np.zeros((frames, 1), smp)
        e[j, 0] = 1.0
        made, y = _run(r, taps, e, blocks, ratios)
        assert made == per_block, (j, made, per_block)
        cols.append(y)
    A = np.stack(cols, axis=1) if cols else np.zeros((sum(per_block), 0))
    A.setflags(write=False)
    return A, tuple(per_block)


@functools.lru_cache(maxsize=None)
def output_count(taps, filters, flags, blocks, ratios, lowpass_ratio=0.0, fixed=None):
    """the clip's output frames M on the oracle (of silence: the count does not depend on the samples)"""
    r = O.OracleResampler(1, taps, filters, lowpass_ratio, flags, fixed=fixed, kind="strict")
    if fixed is not None:
        ratios = (float(fixed[1]) / float(fixed[0]),) * len(blocks)
    return sum(_run(r, taps, np.zeros((int(sum(blocks)), 1), np.float32), blocks, ratios)[0])


def clip_blocks(length, block, ratios):
    """ClipWarper's cut of a clip: (frames of every block, their ratios) — an empty clip is one block of no frames"""
    k = max(1, -(-length // block))
    return tuple(min(block, length - q * block) for q in range(k)), tuple(float(v) for v in ratios[:k])
