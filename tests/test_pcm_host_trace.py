"""pcm_host.c's gathered entries, call for call and table byte for table byte, without a GPU.

pcm_host.c is plain C whose only undefined project symbols are the device runtime's (arthip_*) and two helpers of
resampler_host.c.  tests/host_trace/pcm_stub_rt.c defines all of them as functions that print their arguments (and hex-dump every
uploaded table); tests/host_trace/pcm_trace_main.c drives the decimator batch / clips body, the biquad batch, clips and
filter-clips entries and the ingest batch through a fixed list of cases.  The program's stdout must equal the golden, which was
recorded from the pcm_host.c of commit 3ebd4d8 (before the entries' shared steps were factored out): the sequence of runtime
calls, every table byte, every return value, the error count and the message texts of every case.

Eleven cases dump their tables as hex; their variants and failures print the table's length and a hash of its bytes.  When one of
those differs, run the program with PCM_TRACE_DUMP=1 on both sources to see every table dumped.

To record the goldens again from another pcm_host.c (both widths):

    git show 3ebd4d8:audio_resampler_amd/csrc/pcm_host.c > /tmp/parent_pcm_host.c
    python tests/test_pcm_host_trace.py --record /tmp/parent_pcm_host.c
"""
import os
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "audio_resampler_amd", "csrc")
INC = os.path.join(ROOT, "include")
TRACE = os.path.join(HERE, "host_trace")
WIDTHS = (32, 64)


def golden_path(width):
    return os.path.join(HERE, "golden", "pcm_host_trace_%d.txt" % width)


def trace(pcm_host, width, workdir):
    """Compile `pcm_host` with the stub runtime and the driver as build.py compiles it; the program's stdout."""
    exe = os.path.join(workdir, "pcm_trace_%d" % width)
    cmd = ["gcc", "-std=c99", "-O2", "-ffp-contract=off", "-Wall", "-I", INC, "-I", CSRC, pcm_host,
           os.path.join(TRACE, "pcm_stub_rt.c"), os.path.join(TRACE, "pcm_trace_main.c"), "-o", exe, "-lm", "-lpthread"]
    if width == 64:
        cmd.append("-DPATH_WIDTH=64")
    subprocess.check_call(cmd)
    # (ARTAMD_* variables steer pcm_host.c: the routes, the warm-up, abort on error)
    env = {k: v for k, v in os.environ.items() if not k.startswith("ARTAMD_")}
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert run.returncode == 0, run.stderr[-2000:]
    return run.stdout


@pytest.mark.parametrize("width", WIDTHS)
def test_pcm_host_trace_equals_the_parent(width, tmp_path):
    got = trace(os.path.join(CSRC, "pcm_host.c"), width, str(tmp_path)).splitlines()
    with open(golden_path(width)) as f:
        want = f.read().splitlines()
    case = "(before the first case)"
    for number, (g, w) in enumerate(zip(got, want), 1):
        if w.startswith("== "):
            case = w
        assert g == w, "line %d, in case %r" % (number, case)
    assert len(got) == len(want)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        for width in WIDTHS:
            with open(golden_path(width), "w") as f:
                f.write(trace(os.path.abspath(sys.argv[2]), width, tmp))
            print("recorded", golden_path(width))
