#!/usr/bin/env python3
"""Golden vectors of the end-point LPC extrapolation from the REAL reference (extrapolator.c compiled into
oracle/_ref/libartref{,64}_strict.so by oracle/Makefile).  Run in the build container only:
    make -C oracle ref && python tests/golden/make_golden_extrapolate.py

Inputs are synthetic (tests/_extrapolate.py: signal(), regenerated from a seed).  Stored per case (width, kind, count,
direction): for every extras value of the case a digest of the reference's samples, and the first HEAD / last TAIL samples of
the longest.  Data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _extrapolate as X  # noqa: E402

out = {}
for width in (32, 64):
    R = X.RefExtrapolator(width)
    for kind in X.KINDS:
        for count in X.COUNTS:
            for backward in (False, True):
                known = X.place(kind, count, width, backward)
                k = X.key(width, kind, count, backward)
                longest = None
                for e in X.extras_of(count):
                    y = R.run(known, e, backward)
                    out[f"{k}/{e}"] = X.digest(y)
                    longest = y
                out[k + "/head"] = longest[:X.HEAD]
                out[k + "/tail"] = longest[-X.TAIL:]
        print(width, kind, flush=True)
np.savez_compressed(os.path.join(HERE, "extrapolate.npz"), **out)
