# Round-end evidence in one GPU run: `bash tools/round_end.sh <commit> <out dir>`: the full bench line (`bench.py --full`), tools/prof_all.sh
# (kernel traces, PMC passes, training trace, timeline; its own outputs where its header says) and the parity ablation; this script's outputs
# under <out dir> (copy <out dir>/r04/* and the bench line into profiles/).
set -e
REV=${1:-final}
OUT=${2:?usage: bash tools/round_end.sh <commit> <out dir>}
mkdir -p $OUT/r04
python bench.py --full > $OUT/r4_bench_final.json 2> $OUT/r4_bench_final.err
python -c "import json,sys;d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]);print(round(d['value'],2),'fps', round(d['roofline']['correlation_kernel']['launch_ms'],2),'ms corr; bf16', round(d['bf16_letter']['value'],2),'; harness', round(d['harness']['value'],2),'; train', round(d['train']['value'],1),'; cpu', d['cpu_baseline']['sample'][:120])" $OUT/r4_bench_final.json
bash tools/prof_all.sh $REV > $OUT/r4_prof_all.log 2>&1
tail -3 $OUT/r4_prof_all.log
python tools/ablate_parity.py --out $OUT/r04/ablate_parity.json > $OUT/r04/r04_parity_ablation.txt 2>&1
tail -3 $OUT/r04/r04_parity_ablation.txt | cut -c1-160
