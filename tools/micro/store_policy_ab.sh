# alternating A/B of store-policy variants (tools/micro/store_policy_build.sh -> _abl/libartamd_NAME.so) on one box, on the slab kernel's four
# shapes of tools/micro/slab_ab.sh:  REPS=4 SHAPES="0 1 2 3" bash tools/micro/store_policy_ab.sh OUTDIR VARIANT...
# "step" is a whole call (peak pass, quantise pass, slab kernel: what the boundaries cost shows here), "kernel" the slab kernel between HIP events.
# A run that fails or runs into its time limit ends the script: nothing is started behind it.
export TMPDIR=/tmp; R=$(cd "$(dirname "$0")/../.." && pwd); mkdir -p "$1"; O=$(cd "$1" && pwd); shift
cd /tmp
SH=("8 988 988 44100 48000 0 1 1048576" "4 988 988 44100 48000 0 1 1048576" "32 988 988 44100 48000 0 1 262144" "8 988 988 44100 48000 0 1 524288"); [ -n "$EXTRA_SHAPE" ] && SH+=("$EXTRA_SHAPE")        # (EXTRA_SHAPE: shape 4 of SHAPES; KERNEL: the kernel preference, 7 = fixed point)
: > $O/ab.txt
for rep in $(seq ${REPS:-4}); do
for s in ${SHAPES:-0 1 2 3}; do
  for v in "$@"; do
    ARTAMD_LIB=$R/_abl/libartamd_$v.so timeout -k 10 120 python $R/tools/bench_shapes.py ${SH[$s]} ${KERNEL:-7} > $O/run.txt 2>&1 || { echo "$v: FAILED (exit $?)" >> $O/ab.txt; cat $O/run.txt; exit 1; }
    grep -v amdgpu.ids $O/run.txt | sed "s/^/$v: /" >> $O/ab.txt
  done
done
done
python - <<PY | tee $O/table.txt
import re,statistics,collections
d=collections.defaultdict(list)
for l in open("$O/ab.txt"):
    m=re.match(r"(\w+): ch (\d+) .* block (\d+) .*step ([0-9.]+) ms\s+fir kernel ([0-9.]+) ms",l)
    if m: d[(int(m.group(2)),int(m.group(3)),m.group(1))].append((float(m.group(5))*1000,float(m.group(4))*1000))
for k in sorted(d): print("%2d ch %7d %-8s kernel %.1f us  step %.1f us   kernel runs %s  step runs %s"%(k[0],k[1],k[2],statistics.median(x[0] for x in d[k]), statistics.median(x[1] for x in d[k]), [round(x[0],1) for x in d[k]], [round(x[1],1) for x in d[k]]))
PY
