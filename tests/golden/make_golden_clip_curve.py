#!/usr/bin/env python3
"""The curve-sampling entries' results at a given commit: clip_curve_parent_bits.npz.  Run on the GPU, with the libraries of the commit to pin:

    python tests/golden/make_golden_clip_curve.py --commit HASH

The stored file was made at the parent of the commit that added it, when fir_sample.hip and fir_band.hip each had their own kernels' bodies;
its hash is in the file (`parent_commit`).  The cases and their inputs are tests/_clip_curve_bits.py's (synthetic, regenerated from a seed);
of the library only the six public wrappers of audio_resampler_amd.sampler and audio_resampler_amd.band are called, so the script runs
whichever kernels stand behind those entries.
Stored per case, sample width and clip: y, gx, and gp / gl where the case asks for them — each the whole result buffer.  Data only."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _clip_curve_bits as G  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", required=True, help="hash of the commit the loaded libraries were built from")
ap.add_argument("--out", default=os.path.join(HERE, "clip_curve_parent_bits.npz"))
a = ap.parse_args()

out = {"parent_commit": np.array(a.commit)}
for name in G.CASES:
    for width in G.WIDTHS:
        got = G.run(name, width)
        for key, value in got.items():
            out[f"{name}/{width}/{key}"] = value
        live = [v for k, v in got.items() if k.endswith("/y") or k.endswith("/gx")]
        assert any(np.any((v != 0) & (v != G.SENTINEL)) for v in live), (name, width)
        print(name, width, {k: v.shape for k, v in got.items()})
np.savez_compressed(a.out, **out)
print(a.out, os.path.getsize(a.out), "bytes")
