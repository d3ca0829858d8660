"""GPU (-m gpu): the store policies of the fixed-point path's bulk stores (csrc/fir_matrix_common.hip.h: ST_*) and the slab kernel's late look
at the stand-by flag.  Cache-policy bits cannot change arithmetic; what they could break is VISIBILITY — a later reader (the next launch on
any XCD, a copy engine, another stream behind an event, the host) finding stale bytes — and the flag's move could break the stand-by.
So: the slab kernel's bytes against the 32-slot kernels' for the same stream, read back every way a caller can; and a stream whose second
call holds an infinity.  The switches are read once per process: every variant plays in a process of its own (_store_policy_stream.py)."""
import functools, json, os, subprocess, sys, tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CALLS, CH, BAD_CHANNEL = 3, 8, 3                              # (_store_policy_stream.py's stream; the helper is not imported: it needs torch and a GPU)

SLABS, TILES32 = (("ARTAMD_I8_SLAB_MIN", "1"),), (("ARTAMD_I8_SLAB_MIN", "1000000"),)
NO_KEPT_ROWS = (("ARTAMD_ROWS_CACHE", "0"),)
_TMP = tempfile.TemporaryDirectory(prefix="store_policy_")


def _sessions(**env):
    r = subprocess.run([sys.executable, os.path.join(HERE, "_slab_sessions.py")], env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def _stream(kernel, inf, env):
    """(per-call records, the three readings of every call's output) of the small stream in a process with `env` set; played once per variant"""
    path = os.path.join(_TMP.name, f"k{kernel}_i{inf}_" + "_".join(v for _, v in env) + ".npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "_store_policy_stream.py"), str(kernel), str(inf), path],
                       env=dict(os.environ, **dict(env)), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with np.load(path) as z:
        return json.loads(r.stdout.strip().splitlines()[-1]), {k: z[k] for k in z.files}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_sessions_leave_the_same_bits_with_slabs_and_without():
    a, b = _sessions(ARTAMD_I8_SLAB_MIN="1"), _sessions(ARTAMD_I8_SLAB_MIN="1000000")
    assert len(a) == len(b) >= 8
    assert [s["frames"] for s in a] == [s["frames"] for s in b]
    assert {s["sha256"] for s in a} == {s["sha256"] for s in b}, (a, b)
    assert [s["sha256"] for s in a] == [s["sha256"] for s in b]


def test_every_reader_behind_a_call_sees_the_outputs():
    """the slab kernel's outputs — through the same stream's copy, another stream's copy behind an event, and the host — are the bytes the
    32-slot form leaves for the same stream; calls 2 and 3 read the history the call before rolled (the roll's stores) and its own planes"""
    (ca, a), (cb, b) = _stream(7, 0, SLABS), _stream(7, 0, TILES32)
    assert [c["form"] for c in ca] == ["fir_i8_slab_kernel"] * CALLS, ca
    assert all(c["state"] == 1 and c["form"] in ("fir_i8_stream_kernel", "fir_i8_dma_kernel") for c in cb), cb
    assert [c["frames"] for c in ca] == [c["frames"] for c in cb]
    for k in range(CALLS):
        want = b[f"host{k}"]
        assert want.shape[0] == ca[k]["frames"] > 0 and np.all(np.isfinite(want)), k
        for reading in ("same", "other", "host"):
            assert np.array_equal(_bits(a[f"{reading}{k}"]), _bits(want)), (k, reading)
            assert np.array_equal(_bits(b[f"{reading}{k}"]), _bits(want)), (k, reading, "32-slot form")


@pytest.mark.parametrize("rows", [NO_KEPT_ROWS, ()], ids=["rows_per_launch", "rows_kept"])
def test_an_infinity_in_the_second_call_stands_that_call_down_and_no_other(rows):
    """the slab kernel examines the stand-by flag behind its first chunk's pieces: call 2 (one infinity) is the f32 tile loop's, calls 1 and 3
    are fixed point and the bytes they are without the infinity.  Call 2's finite channels are the f32 streaming kernel's bytes (preference 6):
    the stand-by is that kernel's tile loop — with every launch's rows built from its own positions, and on rows kept across calls too, this
    stream's canonical period being founded by its first call, where preference 6 anchors its tiles as well"""
    (cs, s), (c6, f), (c0, clean) = _stream(7, 1, SLABS + rows), _stream(6, 1, SLABS + rows), _stream(7, 0, SLABS + rows)
    assert [c["state"] for c in cs] == [1, 2, 1], cs
    assert [c["state"] for c in c0] == [1, 1, 1] and [c["state"] for c in c6] == [0, 0, 0], (c0, c6)
    assert [c["frames"] for c in cs] == [c["frames"] for c in c6] == [c["frames"] for c in c0]
    for k in (0, 2):
        for reading in ("same", "other", "host"):
            assert np.array_equal(_bits(s[f"{reading}{k}"]), _bits(clean[f"host{k}"])), (k, reading)
    finite = [c for c in range(CH) if c != BAD_CHANNEL]
    assert not np.all(np.isfinite(s["host1"][:, BAD_CHANNEL])) and not np.all(np.isfinite(f["host1"][:, BAD_CHANNEL]))
    for reading in ("same", "other", "host"):
        got, want = s[f"{reading}1"][:, finite], f["host1"][:, finite]
        assert np.all(np.isfinite(want)) and got.shape == want.shape
        assert np.array_equal(_bits(got), _bits(want)), reading
