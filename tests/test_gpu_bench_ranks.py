"""GPU (-m gpu): bench.py's multi-rank path, executed.  The driver runs `python -m torch.distributed.run --nproc-per-node N bench.py
--gpus N` on an 8-GPU node at round end; on the one-GPU box the same command line runs with two or four ranks sharing the device and the
few scalars of the reduction travelling over gloo (ARTAMD_BENCH_BACKEND=gloo, bench.py) — rendezvous, channel slices of ONE
stream, barrier + max-over-ranks timing, frame-count agreement and the JSON line are what is under test, not the numbers.
(Never more ranks than that: every rank holds the device, beside this test's own process, and a device shared with other work takes
a handful of such processes at most.)"""
import json
import os

import numpy as np
import pytest

from _spawn import report, run_ranks

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("scaling", ["weak", "strong"])
def test_bench_runs_with_two_ranks(scaling):
    out = run_ranks(2, ["--gpus", "2", "--steps", "4", "--warmup", "1", "--block-frames", "262144", "--preroll-ms", "20",
                        "--scaling", scaling, "--no-cpu-baseline"], ARTAMD_BENCH_BACKEND="gloo")
    assert out.returncode == 0, report(out)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout [-2000:]                # rank 0 alone prints
    line = json.loads(lines [0])
    assert line ["n_gpus"] == 2 and line ["steps"] == 4 and line ["scaling"] == scaling
    cfg = line ["config"]
    if scaling == "strong":
        assert cfg ["stream_channels"] == 32 and cfg ["channels_per_gpu"] == 16
    else:
        assert cfg ["stream_channels"] == 16 and cfg ["channels_per_gpu"] == 8
    # whole-job throughput: both ranks' samples over the slower rank's time
    frames_per_step = 262144 * 48000 / 44100
    assert abs(line ["value"] * 1e6 * line ["ms_per_step"] * 1e-3 / (frames_per_step * cfg ["stream_channels"]) - 1.0) < 0.01
    assert line ["roofline"] ["launches"] == 4
    # BASELINE.json configs[3] rides along in the default (weak) command line: one 32-channel stream shared among the ranks
    if scaling == "weak":
        d = line ["config_d"]
        assert d ["scaling"] == "strong" and d ["stream_channels"] == 32 and d ["channels_per_gpu"] == 16 and d ["n_gpus"] == 2 and d ["frames_consistent"]
        assert abs(d ["value"] * 1e6 * d ["ms_per_step"] * 1e-3 / (frames_per_step * 32) - 1.0) < 0.01
    else:
        assert "config_d" not in line


def test_bench_runs_with_four_ranks_at_the_driver_partition(tmp_path):
    """The partition of the driver's N = 8 tier on four ranks: the headline keeps 8 channels per rank (a 32-channel stream here, 64 at
    N = 8) and config_d gets 4 channels per rank, as BASELINE.json configs[3] has at N = 8 (one 16-channel stream here, 32 at N = 8;
    channel_slice(32, 8, r) itself: test_shard_gloo.py).  Partition, rendezvous, barrier, agreement, the JSON line and every rank's
    --dump-outputs slice are under test, not the numbers."""
    dump = str(tmp_path / "dump")
    out = run_ranks(4, ["--gpus", "4", "--steps", "3", "--warmup", "1", "--block-frames", "131072", "--preroll-ms", "10",
                        "--total-channels", "16", "--no-cpu-baseline", "--dump-outputs", dump], ARTAMD_BENCH_BACKEND="gloo")
    assert out.returncode == 0, report(out)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout [-2000:]
    line = json.loads(lines [0])
    assert line ["n_gpus"] == 4 and line ["steps"] == 3 and line ["scaling"] == "weak"
    cfg = line ["config"]
    assert cfg ["stream_channels"] == 32 and cfg ["channels_per_gpu"] == 8
    frames_per_step = 131072 * 48000 / 44100
    assert abs(line ["value"] * 1e6 * line ["ms_per_step"] * 1e-3 / (frames_per_step * 32) - 1.0) < 0.01
    d = line ["config_d"]
    assert d ["scaling"] == "strong" and d ["stream_channels"] == 16 and d ["channels_per_gpu"] == 4 and d ["n_gpus"] == 4 and d ["frames_consistent"]
    # every rank dumped its own channel slice of the last timed step; the ranks agree on the frame counts
    assert sorted(os.listdir(dump)) == sorted(f"output_rank{r}{s}.npy" for r in range(4) for s in ("", "_counts"))
    counts = [np.load(os.path.join(dump, f"output_rank{r}_counts.npy")) for r in range(4)]
    assert all(np.array_equal(c, counts [0]) for c in counts) and counts [0] [0] == 131072 and abs(counts [0] [1] / frames_per_step - 1.0) < 1e-3
    for r in range(4):
        y = np.load(os.path.join(dump, f"output_rank{r}.npy"))
        assert y.dtype == np.float32 and y.shape == (int(counts [0] [1]), 8) and np.all(np.isfinite(y)) and np.any(y != 0)
