#!/bin/bash
# On the GPU box: regenerate the round-3 artefacts of profiles/ under gpurun_out/<tag>/ (copy them to profiles/ afterwards).
#   tools/refresh_profiles_r03.sh <tag> [quick]
#   quick: kernel trace only (no bench line with the CPU baseline, no PMC passes)
set -u
TAG=${1:-r03}
QUICK=${2:-}
R=$GRAFT_REPO_ROOT
OUT=$R/gpurun_out/$TAG
mkdir -p $OUT
if [ -z "$QUICK" ]; then
  cd $R && python3 bench.py --full > $OUT/r03_bench.json 2> $OUT/bench.err
fi
cd /tmp && export TMPDIR=/tmp
# kernel trace of the bench command (headline S3 rollouts + S1 + learning loops; C2 / C3 / C5 / deploy side measurements too)
timeout 1200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/r03_bench_profiled.json 2> $OUT/kt.log
if [ -z "$QUICK" ]; then
  # HBM traffic of the dominant kernels (separate --pmc passes, kernel trace off): the S3 rollout only, then C5 only
  for C in FETCH_SIZE WRITE_SIZE; do
    timeout 600 rocprofv3 --pmc $C --output-format csv -d $OUT/$C -- python3 $R/bench.py --full --no-cpu-baseline --train-steps 0 --no-configs --s1-steps 0 --s2-steps 20 --spinup 20 --repeats 2 > $OUT/$C.log 2>&1
    timeout 600 rocprofv3 --pmc $C --output-format csv -d $OUT/C5_$C -- python3 $R/tools/time_c5.py pmc > $OUT/C5_$C.log 2>&1
  done
fi
cd $R
python3 - "$OUT" <<'PY'
import csv, glob, json, shutil, sys
out = sys.argv[1]
for f in glob.glob(f"{out}/kt/**/*kernel_stats.csv", recursive=True):
    shutil.copy(f, f"{out}/r03_bench_kernel_stats.csv")
per = {}
for f in glob.glob(f"{out}/kt/**/*kernel_trace.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        n = r["Kernel_Name"].split("(")[0].replace("void ", "")
        per.setdefault(n, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
summ = {k: dict(launches=len(v), mean_us=sum(v) / len(v), min_us=min(v), max_us=max(v)) for k, v in per.items() if "mdq" in k}
json.dump(summ, open(f"{out}/r03_kernel_trace_summary.json", "w"), indent=1)
res = {}
for tag, pre in (("s3", ""), ("c5", "C5_")):
    res[tag] = {}
    for c in ("FETCH_SIZE", "WRITE_SIZE"):
        vals = {}
        for f in glob.glob(f"{out}/{pre}{c}/**/*counter_collection.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                if r["Counter_Name"] == c and "mdq" in r["Kernel_Name"]:
                    vals.setdefault(r["Kernel_Name"].split("(")[0].replace("void ", ""), []).append(float(r["Counter_Value"]))
        res[tag][c] = {k: dict(n=len(v), mean=sum(v) / len(v)) for k, v in vals.items()}
pmc = dict(units="FETCH_SIZE / WRITE_SIZE as reported by rocprofv3 (KiB per launch); hbm bytes = KiB x 1024; the gfx950 x2 correction of the "
                 "guide applies to wide (16 B per lane) coalesced reads: both the raw and the corrected figure are given", per_kernel=res)
for tag in res:
    for k in res[tag].get("FETCH_SIZE", {}):
        f_ = res[tag]["FETCH_SIZE"][k]["mean"]
        w_ = res[tag].get("WRITE_SIZE", {}).get(k, dict(mean=0.0))["mean"]
        pmc.setdefault("hbm_bytes_per_launch", {}).setdefault(tag, {})[k] = dict(raw=(f_ + w_) * 1024, corrected=(2 * f_ + w_) * 1024)
json.dump(pmc, open(f"{out}/r03_pmc_summary.json", "w"), indent=1)
print(json.dumps({k: v for k, v in summ.items()}, indent=1)[:6000])
print(json.dumps(pmc.get("hbm_bytes_per_launch", {}), indent=1)[:3000])
PY
find $OUT -name "*kernel_trace.csv" -delete; find $OUT -name "*agent_info.csv" -delete; find $OUT -name "*counter_collection.csv" -delete
ls $OUT
