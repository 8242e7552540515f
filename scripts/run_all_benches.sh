cd "$GRAFT_REPO_ROOT"
O="${1:?usage: run_all_benches.sh OUTPUT_DIR}"; mkdir -p "$O"
bash scripts/run_prof.sh --full > "$O/prof_stdout.txt" 2>&1
python bench.py --full --flow --cpu-frames 0 2>&1 | tail -1 > "$O/bench_flow.json"
python bench.py --full --height 1024 --width 1024 --steps 16 --warmup 4 --cpu-frames 0 2>&1 | tail -1 > "$O/bench_1024_single.json"
python bench.py --full --height 1024 --width 1024 --scales 2 --steps 16 --warmup 4 --cpu-frames 0 2>&1 | tail -1 > "$O/bench_1024_2scale.json"
python bench.py --full --height 1024 --width 1024 --scales 2 --flow --steps 16 --warmup 4 --cpu-frames 0 2>&1 | tail -1 > "$O/bench_1024_2scale_flow.json"
for f in "$O"/bench_*.json; do echo $f; python -c "
import json,sys; d=json.loads(open('$f').read()); print(d['value'], d['ms_per_step'], d['roofline']['achieved'], d['roofline']['layer'])"; done
