"""GPU: both clip adjoint entries reproduce, bit for bit, what resampleAdjointClipsPlanarDevice gave at the commit before this test
(tests/golden/clip_adjoint_parent_bits.npz, made by tests/golden/make_golden_clip_adjoint.py at the commit the file names): the two
kernels of fir_adjoint.hip keep the chunk loop twice, and whatever is done to either, or to merge them, has these bits to give.  resampleAdjointClipsPlanarDevice takes each clip as given, resampleAdjointScheduleClipsPlanarDevice as one block.  The cases
(tests/_clip_adjoint_bits.py): interpolating both ways and at any ratio, the nearest filter, the pass-through, every channel-group width
and a partial group, the 8-byte build."""
import os

import numpy as np
import pytest

import _clip_adjoint_bits as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_adjoint_parent_bits.npz")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", G.CASES, ids=[c[0] for c in G.CASES])
def test_both_entries_give_the_parent_commits_bits(case):
    pytest.importorskip("torch")
    stored = np.load(GOLDEN)
    assert len(str(stored["parent_commit"])) == 40
    for blocks in (False, True):
        launches, got = G.run(case, blocks)
        assert launches == 1
        for i, gx in enumerate(got):
            want = stored[f"{case[0]}/{i}"]
            assert want.dtype == gx.dtype and want.shape == gx.shape == (case[2], case[8][i]) and np.any(want != 0), (blocks, i)
            assert np.array_equal(bits(gx), bits(want)), ("schedule entry" if blocks else "clips entry", i, int((bits(gx) != bits(want)).sum()))


def test_the_file_holds_exactly_the_cases():
    """(no GPU needed)"""
    stored = np.load(GOLDEN)
    assert sorted(stored.files) == sorted(["parent_commit"] + [f"{c[0]}/{i}" for c in G.CASES for i in range(len(c[8]))])
