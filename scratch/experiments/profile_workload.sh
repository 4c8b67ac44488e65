# rocprofv3 kernel stats of bench.py on another workload (GPU box): bash scratch/experiments/profile_workload.sh rmat22 [extra bench args]
set -u
w=$1; shift
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
mkdir -p results
tag=${TAG:-$w}
rm -rf results/prof_$tag
rocprofv3 --kernel-trace --stats --output-format csv -d results/prof_$tag -- python3 bench.py --full --no-cpu-baseline --workload $w "$@" > results/prof_$tag.log 2>&1
tail -1 results/prof_$tag.log | cut -c 1-200
cp $(find results/prof_$tag -name "*kernel_stats.csv" | head -1) results/ks_$tag.csv
cp $(find results/prof_$tag -name "*kernel_trace.csv" | head -1) results/kt_$tag.csv
