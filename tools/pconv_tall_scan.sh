# headline (four streams) under the stencil's tall / 96-column tile thresholds: FCL_PCONV_N96_MIN=0 = the parent's tiles, X=0 = the defaults (128 x 96 tile for the last postnet
# layer), FCL_PCONV_TALL_MIN=40 = the postnet on 256-row tiles (98 tiles at B = 32), 20 = the encoder / predictor convolutions too; twice round: $TMPDIR/$1/tall_scan.log
OUT=${TMPDIR:-/tmp}/${1:-r7}
mkdir -p $OUT
val() { python3 -c "import json,sys; d=json.loads(sys.stdin.read().strip().split('\n')[-1]); print(round(d['value']/1e6,2), ' '.join('%s=%.3f' % (k.split('_kernel')[1], v['ms_per_step']) for k, v in d['kernels'].items() if 'pconv' in k))"; }
for e in FCL_PCONV_N96_MIN=0 X=0 FCL_PCONV_TALL_MIN=40 FCL_PCONV_TALL_MIN=20 FCL_PCONV_N96_MIN=0 X=0 FCL_PCONV_TALL_MIN=40 FCL_PCONV_TALL_MIN=20; do
  v=$(env $e timeout -k 10 300 python3 bench.py --full --no-cpu-baseline --no-extras --regions 11 2>>$OUT/err.log | val) || exit 1
  echo "$e -> $v" >> $OUT/tall_scan.log
done
cat $OUT/tall_scan.log
