"""GPU: the six curve-sampling entries (sampler: forward, adjoint, position gradient; band: forward, adjoint, gradients) reproduce, bit
for bit and in both sample widths, what they gave at the commit before their kernels were folded into one body per pass
(tests/golden/clip_curve_parent_bits.npz, made by tests/golden/make_golden_clip_curve.py at the commit the file names).  The identity
tests that compare the banded entries with the unbanded ones say less once both sides run one body; these arrays are the parent's own.
The cases (tests/_clip_curve_bits.py): clips of 0, 5, 300 and 601 frames in one batch, more than 256 outputs and more than 256 of them
in one input tile's range, 1, 2 and 5 channels, planar with padded pitches and interleaved, interpolating, nearest and pass-through
contexts, positions outside the window on both sides, infinite, NaN and a tiny negative one, ladders of 1, 3 and 8 rungs, levels of
every sort, gp alone, gl alone and both.  Every result buffer is compared whole, with what the entry left alone."""
import os

import numpy as np
import pytest

import _clip_curve_bits as G

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_curve_parent_bits.npz")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("width", G.WIDTHS)
@pytest.mark.parametrize("name", list(G.CASES))
def test_the_entries_give_the_parent_commits_bits(name, width):
    pytest.importorskip("torch")
    stored = np.load(GOLDEN)
    assert len(str(stored["parent_commit"])) == 40
    got = G.run(name, width)
    assert sorted(got) == sorted(G.keys(name))
    for key, value in got.items():
        want = stored[f"{name}/{width}/{key}"]
        assert want.dtype == value.dtype and want.shape == value.shape, key
        assert np.array_equal(bits(value), bits(want)), (key, int((bits(value) != bits(want)).sum()))


def test_the_file_holds_exactly_the_cases():
    """(no GPU needed)"""
    stored = np.load(GOLDEN)
    assert sorted(stored.files) == sorted(["parent_commit"] + [f"{n}/{w}/{k}" for n in G.CASES for w in G.WIDTHS for k in G.keys(n)])
    assert os.path.getsize(GOLDEN) < 512 * 1024
