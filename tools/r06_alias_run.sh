set -x
export OUT=${OUT:?set OUT to the directory for this run's files}
mkdir -p $OUT
./tools/ubench/corun > $OUT/corun.txt 2>&1; cat $OUT/corun.txt
python -m pytest tests -m gpu -x -q 2>&1 | tail -5
python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench.json 2> $OUT/bench.err; tail -3 $OUT/bench.err
python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['OUT'], 'bench.json')).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['paf_identical'], d['hbm_resident_gb'], d['cli_end_to_end']['wall_s'], d['config5']['value'], d['config2']['value'])
PY
