#!/usr/bin/env python3
"""The clip adjoint's results at a given commit: clip_adjoint_parent_bits.npz.  Run on the GPU, with the libraries of the commit to pin:

    python tests/golden/make_golden_clip_adjoint.py --commit HASH

The stored file was made at the parent of the commit that added it, through the two-phase fir_adjoint_kernel; its hash is in the file
(`parent_commit`).  The cases and their inputs are tests/_clip_adjoint_bits.py's (synthetic, regenerated from a seed); of the library only
adjoint_clips_planar_device is called, so the script runs whichever kernel stands behind that entry.
Stored per case and clip: gx [channels, frames].  Data only."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _clip_adjoint_bits as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", required=True, help="hash of the commit the loaded libraries were built from")
ap.add_argument("--out", default=os.path.join(HERE, "clip_adjoint_parent_bits.npz"))
a = ap.parse_args()

out = {"parent_commit": np.array(a.commit)}
for case in G.CASES:
    launches, gxs = G.run(case, blocks=False)
    assert launches == 1, (case[0], launches)
    for i, gx in enumerate(gxs):
        assert gx.shape == (case[2], case[8][i]) and np.any(gx != 0) and not np.any(gx == -777.25), (case[0], i)
        out[f"{case[0]}/{i}"] = gx
    print(case[0], [g.shape for g in gxs])
np.savez_compressed(a.out, **out)
print(a.out, os.path.getsize(a.out), "bytes")
