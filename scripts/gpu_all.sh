# whole GPU suite (incl. full-size C4/C5 parity), then the C4 bench line with its CPU baseline (--full)
# results go to $OUT (default bench_out/)
set -o pipefail
cd $GRAFT_REPO_ROOT
O=${OUT:-bench_out}
mkdir -p $O
nproc > $O/host.txt; lscpu | grep "Model name" >> $O/host.txt
GP_ORACLE_PROGRESS=1 timeout -k 10 1000 python -u -m pytest tests -x -v -s --timeout 1200 --timeout-method thread -m gpu --durations=15 > $O/pytest_gpu.log 2>&1
rc=$?; echo "pytest exit $rc"; tail -25 $O/pytest_gpu.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 3 > $O/bench.json 2> $O/bench.err
rc=$?; echo "c4 bench exit $rc"; cat $O/bench.json; tail -5 $O/bench.err
exit $rc
