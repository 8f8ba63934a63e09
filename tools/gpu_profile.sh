# Round profile pass on the GPU box: the full bench line (--full: + CPU baseline, bf16 side line, per-kernel breakdown), rocprofv3 kernel
# trace of the same workload, the two HBM-traffic PMC passes (separate runs, no trace domains), per-kernel summaries under OUT_DIR
# (default: prof_out/ in the repository, git-ignored; copied to profiles/ by hand).
#   bash tools/gpu_profile.sh <tag> [OUT_DIR]            e.g. r02e
TAG=${1:-r03}
set -x
R=$(cd "$(dirname "$0")/.." && pwd)
O=${2:-$R/prof_out}
mkdir -p $O && O=$(cd $O && pwd)
cd $R
timeout 600 python bench.py --full --breakdown $O/${TAG}_breakdown.json > $O/${TAG}_bench.json 2> $O/${TAG}_bench.err; tail -1 $O/${TAG}_bench.json | cut -c1-600
cd /tmp && export TMPDIR=/tmp
CMD="python $R/bench.py --full --steps 2 --warmup 0 --no-cpu-baseline --no-side-modes --eager --no-overlap"
timeout 300 rocprofv3 --kernel-trace --stats -d $O/prof_kt -- $CMD > $O/${TAG}_prof_kt.log 2>&1
timeout 300 rocprofv3 --pmc FETCH_SIZE -d $O/prof_fetch -- $CMD > $O/${TAG}_prof_fetch.log 2>&1
timeout 300 rocprofv3 --pmc WRITE_SIZE -d $O/prof_write -- $CMD > $O/${TAG}_prof_write.log 2>&1
cd $R
python tools/rocpd_stats.py $O/prof_kt/*/*_results.db 70 > $O/${TAG}_kernel_stats.txt
python tools/rocpd_pmc.py $O/prof_fetch/*/*_results.db $O/prof_write/*/*_results.db --top 24 --json $O/${TAG}_pmc_hbm.json > $O/${TAG}_pmc_hbm.txt 2>&1
python tools/make_traffic_json.py $O/${TAG}_pmc_hbm.json $O/${TAG}_pmc_hbm_traffic.json "profiles/${TAG}_pmc_hbm.json"
rm -rf $O/prof_kt $O/prof_fetch $O/prof_write
head -30 $O/${TAG}_kernel_stats.txt
