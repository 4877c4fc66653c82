# every step under its own timeout: a hung kernel must not eat the GPU budget
# usage: tools/gpu_probe.sh [output directory, default .]
O=${1:-.}; mkdir -p $O
timeout 300 python -m pytest tests/test_elas_gpu.py -x -q 2>&1 | tail -2
timeout 120 python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --batch 64 --lanes 1 --group 4 > $O/probe.json 2>$O/probe.err
python - $O/probe.json <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
k=d["roofline"]["kernels_us_probe_step"]
print("probe pairs/s", round(d["value"]), "sum_us", round(sum(k.values()),1))
print(k)
PY
timeout 180 python bench.py --full --no-cpu-baseline > $O/bench.json
python - $O/bench.json <<'PY'
import json, sys
d=json.load(open(sys.argv[1]))
print("bench", d["value"], d["roofline"]["kernel"], d["roofline"]["frac"])
PY
