# round-2 evidence run: benches of every config + rocprofv3 passes (summaries are copied to profiles/)
TAG=${1:-r2b}
OUT=${OUT_ROOT:-results}/$TAG      # the bench lines, the batch sweep and the training trace
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
bash profiles/collect.sh ${TAG}_prof > gpurun_out/${TAG}_collect.log 2>&1
cp gpurun_out/${TAG}_prof/traffic.json profiles/traffic_mobilenet_v2_b64.json
python bench.py --full --layers > $OUT/bench_mbv2_b64.json 2> $OUT/bench_mbv2_b64_layers.txt
python bench.py --full --backbone vgg16 --layers > $OUT/bench_vgg16_b32.json 2> $OUT/bench_vgg16_b32_layers.txt
python bench.py --full --img-size 512 --batch 16 --no-cpu-baseline > $OUT/bench_mbv2_512_b16.json 2>/dev/null
python bench.py --full --train --steps 10 --warmup 3 > $OUT/bench_train_mbv2_b32.json 2>/dev/null
python bench.py --full --train --backbone vgg16 --batch 16 --steps 5 --warmup 2 > $OUT/bench_train_vgg16_b16.json 2>/dev/null
for b in 1 16 32 128 256; do python bench.py --full --batch $b --no-cpu-baseline 2>/dev/null | python -c "import sys,json; r=json.loads(sys.stdin.read()); print('B=%d %.0f img/s %.3f ms' % ($b, r['value'], r['ms_per_step']))"; done > $OUT/batch_sweep.txt
python tests/bench_decoder.py > $OUT/bench_decoder.txt 2>&1
bash profiles/collect_sq.sh ${TAG}_sq > gpurun_out/${TAG}_sq.log 2>&1
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/train_trace -o t -- python bench.py --full --train --steps 5 --warmup 2 > $OUT/train_trace.log 2>&1
find gpurun_out -name '*kernel_trace.csv' -delete; find gpurun_out -name '*counter_collection.csv' -size +4M -delete
find $OUT -name '*kernel_trace.csv' -delete
for f in $OUT/*.json; do echo $f; cut -c1-260 $f; done
cat $OUT/batch_sweep.txt
