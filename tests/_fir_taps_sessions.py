"""Helper of test_gpu_fir_taps.py: plays impulse-train sessions (tests/_fir_taps.py) in THIS process's environment — the ARTAMD_*
switches are read once per process — and leaves every call's outputs as .npy files beside one JSON record of traces and kernel forms;
the parent compares.  argv: <directory> <session id>:<form> ..."""
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _fir_taps as FT


def main():
    where, record = sys.argv[1], {}
    for item in sys.argv[2:]:
        sid, form = item.split(":")
        outs, trace, kinds, fallbacks = FT.play_hip(sid, form)
        for i, y in enumerate(outs):
            np.save(os.path.join(where, f"{sid}.{form}.{i}.npy"), y)
        record[item] = {"trace": trace, "kinds": kinds, "calls": len(outs)}
    with open(os.path.join(where, "record.json"), "w") as f:
        json.dump(record, f)


if __name__ == "__main__":
    sys.exit(main())
