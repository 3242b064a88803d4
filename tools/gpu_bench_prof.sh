set -e
mkdir -p gpurun_out
R=$GRAFT_REPO_ROOT
O=${OUT:-$PWD/out} && mkdir -p $O
timeout -k 10 400 python bench.py --full --steps 30 --warmup 5 > $O/bench.json 2> $O/bench.err
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -f csv -d $O/prof -o run -- python3 $R/bench.py --full --steps 30 --warmup 5 --no-cpu > $O/prof.log 2>&1
