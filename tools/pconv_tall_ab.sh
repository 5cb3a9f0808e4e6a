# same-box A/B of two builds of the library, alternating: $1 = the parent's libfcl_hip.so (FCL_LIB) against the in-tree build; $2 = workload (default synthesis), $3 = repetitions.
# Every run's `value` (the median of its 11 regions) -> $TMPDIR/r7/pconv_tall_ab.log.  A gain = every value of the new build above every value of the parent.
BASE=$(readlink -f $1); W=${2:-synthesis}; N=${3:-4}
OUT=${TMPDIR:-/tmp}/r7
mkdir -p $OUT
case $W in
  synthesis) ARGS="--full --no-cpu-baseline --no-extras --regions 11";;
  tts_e2e)   ARGS="--workload tts_e2e --steps 5 --warmup 2 --no-cpu-baseline --regions 5";;
  *)         ARGS="--workload $W --no-cpu-baseline --no-dp-schedule --regions 5";;
esac
val() { python3 -c "import json,sys; print(json.loads(sys.stdin.read().strip().split('\n')[-1])['value'])"; }
for rep in $(seq 1 $N); do
  a=$(FCL_LIB=$BASE timeout -k 10 300 python3 bench.py $ARGS 2>>$OUT/err.log | val) || exit 1
  b=$(timeout -k 10 300 python3 bench.py $ARGS 2>>$OUT/err.log | val) || exit 1
  echo "$W rep $rep parent $a new $b" >> $OUT/pconv_tall_ab.log
done
cat $OUT/pconv_tall_ab.log
