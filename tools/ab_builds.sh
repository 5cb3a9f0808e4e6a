# same-box A/B of two (library, environment) pairs on the default bench line, alternating; the pattern of tools/pconv_tall_ab.sh with a tunable on either side.
#   tools/ab_builds.sh LABEL LIB_A "ENV_A" LIB_B "ENV_B" [alternations = 4]
# LIB_x: a libfcl_hip.so handed over as FCL_LIB ("" = the in-tree build); ENV_x: "" or one NAME=value (e.g. FCL_LSTM_SMALL_M=640).
# Every run's `value` (the median of its 11 regions) is appended to $OUT/ab.log (OUT: default ${TMPDIR:-/tmp}/ab).  A gain = every value of B above every value of A.
LABEL=$1; LA=$2; EA=$3; LB=$4; EB=$5; N=${6:-4}
OUT=${OUT:-${TMPDIR:-/tmp}/ab}
mkdir -p $OUT
ARGS="--full --no-cpu-baseline --no-extras --regions 11"
val() { python3 -c "import json,sys; print('%.0f' % json.loads(sys.stdin.read().strip().split('\n')[-1])['value'])"; }
run() {
  local lib=$1 e=$2
  if [ -n "$lib" ]; then lib="FCL_LIB=$(readlink -f $lib)"; fi
  env $lib $e timeout -k 10 300 python3 bench.py $ARGS 2>>$OUT/err.log | val
}
for rep in $(seq 1 $N); do
  a=$(run "$LA" "$EA") || exit 1
  b=$(run "$LB" "$EB") || exit 1
  echo "$LABEL rep $rep  A[${LA:-in-tree} $EA] $a  B[${LB:-in-tree} $EB] $b" | tee -a $OUT/ab.log
done
