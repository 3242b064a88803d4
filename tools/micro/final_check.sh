# round-end rehearsal: every GPU test, smoke(), the default bench line
set -e
timeout -k 10 600 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread > gpurun_out/final_tests.log 2>&1
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > gpurun_out/final_smoke.log 2>&1
O=${OUT:-$PWD/out} && mkdir -p $O
timeout -k 10 400 python bench.py --full > $O/final_bench.json 2> $O/final_bench.err
