# where the headline step's time and traffic go, per library variant under _abl/ (tools/micro/store_policy_build.sh), on one box:
#   bash tools/micro/store_policy_prof.sh OUTDIR VARIANT...
# per variant: (1) rocprofv3 --kernel-trace --stats of the default bench command -> the three launches' averages (dispatches grouped by kernel and
# grid: the bench's other legs run the same kernels at other sizes); (2), (3) counter runs of their own, no tracing: FETCH_SIZE, then WRITE_SIZE, of
# the headline shape -> the slab kernel's HBM-side bytes per dispatch (FETCH_SIZE x 2: the gfx950 wide-read correction of tools/roofline_report.py).
# A step that fails or runs into its time limit ends the script.
export TMPDIR=/tmp; R=$(cd "$(dirname "$0")/../.." && pwd); mkdir -p "$1"; O=$(cd "$1" && pwd); shift
cd /tmp
SHAPE="8 988 988 44100 48000 0 1 1048576 7"
for v in "$@"; do
  export ARTAMD_LIB=$R/_abl/libartamd_$v.so
  timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $O/$v -o trace -- python $R/bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline --no-other-configs > $O/$v.trace.log 2>&1 || { echo "$v: trace run failed"; tail -5 $O/$v.trace.log; exit 1; }
  timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/$v -o fetch -- python $R/tools/bench_shapes.py $SHAPE > $O/$v.fetch.log 2>&1 || { echo "$v: FETCH_SIZE run failed"; tail -5 $O/$v.fetch.log; exit 1; }
  timeout -k 10 240 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/$v -o write -- python $R/tools/bench_shapes.py $SHAPE > $O/$v.write.log 2>&1 || { echo "$v: WRITE_SIZE run failed"; tail -5 $O/$v.write.log; exit 1; }
done
python - "$O" "$@" <<'PY' | tee $O/summary.txt
import csv, glob, collections, re, sys
O, variants = sys.argv[1], sys.argv[2:]
def short(k):
    m = re.search(r"(fir_i8_\w+|i8_\w+)(<[^>]*>)?", k)
    return m.group(0) if m else k[:60]
for v in variants:
    print("==", v)
    d = collections.defaultdict(list)
    for f in glob.glob(f"{O}/{v}/**/trace_kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "i8" in r["Kernel_Name"]: d[(short(r["Kernel_Name"]), r.get("Grid_Size", r.get("Grid_Size_X", "?")))].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k in sorted(d): print("   %-62s grid %-8s calls %4d  average %.1f us" % (k[0], k[1], len(d[k]), sum(d[k]) / len(d[k])))
    c = collections.defaultdict(list)
    for f in glob.glob(f"{O}/{v}/**/*_counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "fir_i8_slab" in r["Kernel_Name"]: c[r["Counter_Name"]].append(float(r["Counter_Value"]))
    m = {k: sum(x) / len(x) for k, x in c.items()}
    for k in m: print("   slab kernel %-12s per dispatch %.1f KB (%d dispatches)" % (k, m[k], len(c[k])))
    if "FETCH_SIZE" in m and "WRITE_SIZE" in m: print("   slab kernel traffic per dispatch: %.1f MB" % ((2 * m["FETCH_SIZE"] + m["WRITE_SIZE"]) * 1024 / 1e6))
PY
