# usage: bash tools/round_end_profile.sh <tag>  -- the judged command (driver style, with the NK_BENCH_API leg of --full), the
# default command, its kernel trace and its PMC traffic -> $NK_OUT_DIR/<tag>/ (copy what is to be judged to profiles/)
cd "${GRAFT_REPO_ROOT:?}"
tag=${1:-r05}
out=${NK_OUT_DIR:-bench_out}/$tag
mkdir -p $out
NK_BENCH_API=1 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $out/bench_driver_style.log 2>&1
grep "^{\"metric\"" $out/bench_driver_style.log > $out/bench_driver_style_line.json
python bench.py --full > $out/bench_default.log 2>&1
grep "^{\"metric\"" $out/bench_default.log > $out/bench_default_line.json
bash tools/prof_bench.sh ${tag} --steps 2 --warmup 1 --no-cpu-baseline > $out/prof.log 2>&1
bash tools/pmc_bench.sh ${tag} > $out/pmc.log 2>&1
grep -o '"value": [0-9.]*' $out/*.json | head
grep -o '"api": {[^}]*}' $out/bench_driver_style_line.json
grep -o '"ms_per_transform_rank0": [0-9.]*' $out/*.json
