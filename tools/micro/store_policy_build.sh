# one library variant for tools/micro/store_policy_ab.sh: bash tools/micro/store_policy_build.sh NAME [CONST=AUX ...]
# -> _abl/libartamd_NAME.so = the tree's library with the named store-policy constants of csrc/fir_matrix_common.hip.h (ST_SLAB_OUT, ST_PLANES,
# ST_TILE32_OUT, ST_STREAM_OUT) set to the given aux values (0 default, 2 nt, 16 sc1, 17 sc0|sc1) in a private copy of the sources.  Only the two
# files that hold those stores are compiled; the other objects are the tree's (python -m audio_resampler_amd.build first).  SRC=dir: sources other
# than the tree's csrc (a checkout of another commit, for an A/B of a code change); the product build has no switch for any of this.
set -e
R=$(cd "$(dirname "$0")/../.." && pwd); NAME=$1; shift
SRC=${SRC:-$R/audio_resampler_amd/csrc}; OBJ=$R/audio_resampler_amd/_obj; T=$(mktemp -d); mkdir -p $R/_abl
cp $SRC/* $T/
for kv in "$@"; do
  c=${kv%%=*}; v=${kv##*=}
  sed -i "s/^constexpr int $c = [0-9]*;/constexpr int $c = $v;/" $T/fir_matrix_common.hip.h
  grep -q "^constexpr int $c = $v;" $T/fir_matrix_common.hip.h || { echo "no constant $c" >&2; exit 1; }
done
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
for f in fir_matrix.hip fir_matrix_i8.hip; do
  $HIPCC --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -Wall -I $R/include -I $T -c $T/$f -o $T/$f.o &
done
wait
objs=$(ls $OBJ/*.o | grep -v -e /fir_matrix.hip.o -e /fir_matrix_i8.hip.o)
$HIPCC --offload-arch=gfx950 -shared -fPIC -o $R/_abl/libartamd_$NAME.so $objs $T/fir_matrix.hip.o $T/fir_matrix_i8.hip.o -lm -lpthread
rm -r $T
echo $R/_abl/libartamd_$NAME.so
