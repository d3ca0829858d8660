"""GPU: the failure path of the batch entries' grouped matrix-core launch.  A grouped launch that fails returns -1 from the entry, is counted
once in artamdErrorCount, and leaves its contexts { 0, 0 } with position and history untouched — so the repeated call, and everything after it,
gives the bits of an undisturbed run.  Through the and-flush entry no flush is made behind a failed process phase, and the failure is still
counted once.  ARTAMD_TEST_FAIL_FIR=k (the test hook of tests/test_gpu_failure_path.py) fails the k-th FIR launch of the process before it
enqueues anything; a grouped launch counts as one."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

CHILD = r'''
import sys, json, hashlib
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import numpy as np, torch
import audio_resampler_amd as A
from _oracle import noise
B = A.binding(32); L = B.lib()
ch, T, n, N = 2, 380, 24576, 3
rs = []
for _ in range(N):
    r = B.Resampler(ch, T, T, 0.0, A.BLACKMAN_HARRIS | A.SUBSAMPLE_INTERPOLATE, (44100.0, 48000.0, 0)); r.set_kernel(6); r.advance(T / 2); rs.append(r)
x, _ = noise(3 * N * n * ch); x = torch.from_numpy(x.reshape(3, N, n, ch)).cuda()
cap = int(n * 48000 / 44100) + 4 * T + 64
log, digest, gathered = [], hashlib.sha256(), []
for k in range(3):
    fn = B.process_and_flush_batch_device if k == 2 else B.process_batch_device
    out = torch.zeros(N, cap, ch, device="cuda")
    args = (rs, [x[k, i] for i in range(N)], [n] * N, [out[i] for i in range(N)], [cap] * N, [0.0] * N)
    before = [r.state() for r in rs]
    try:
        res = fn(*args)
    except RuntimeError:
        assert [r.state() for r in rs] == before, (before, [r.state() for r in rs])
        log.append((k, L.artamdErrorCount()))
        res = fn(*args)                           # nothing moved: the repeated call is the undisturbed one
    assert all(u == n and g > 0 for u, g in res), (k, res)
    gathered.append([r.last_gathered() for r in rs])
    for i, (u, g) in enumerate(res):
        digest.update(out[i, :g].cpu().numpy().tobytes())
print(json.dumps({"sha256": digest.hexdigest(), "errors": L.artamdErrorCount(), "log": log, "gathered": gathered}))
'''


def _run(fail_at):
    env = dict(os.environ)
    env.pop("ARTAMD_TEST_FAIL_FIR", None); env.pop("ARTAMD_BATCH_MATRIX", None)
    if fail_at:
        env["ARTAMD_TEST_FAIL_FIR"] = str(fail_at)
    code = CHILD % dict(root=os.path.dirname(HERE), tests=HERE)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_a_failed_grouped_launch_moves_nothing_and_is_counted_once():
    pytest.importorskip("torch")
    clean, _ = _run(0)
    assert clean["errors"] == 0 and clean["log"] == []
    assert clean["gathered"][0] == [0, 0, 0] and clean["gathered"][1] == [1, 1, 1], clean      # round 1 builds the rows singly: FIR launches 1 - 3
    # launch 4: the grouped launch of round 2 (resampleProcessBatchInterleavedDevice); launch 5: that of the and-flush entry's process phase
    for fail_at, rnd in ((4, 1), (5, 2)):
        got, err = _run(fail_at)
        assert got["errors"] == 1 and got["log"] == [[rnd, 1]], (fail_at, got)
        assert "grouped" in err, err[-1500:]
        assert got["sha256"] == clean["sha256"], (fail_at, got, clean)
