# The part of profiles/collect.sh that depends on the exact build: GPU test log, the default bench lines, the
# sequential rocprofv3 stats / timeline and the PMC traffic passes (run from the repo root; writes to $O/).
set -x
R=$PWD
O=${O:-out}; export O          # where the run's files go (relative to the repo root)
mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -3 > $O/final_pytest.txt; cat $O/final_pytest.txt
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $R/$O/prof_seq -o r04 -- python $R/bench.py --full --no_cpu_baseline --no_verify --no_overlap --no_graph --transport zerocopy > $R/$O/prof_seq.log 2>&1
mkdir -p $R/$O/pmc
for m in calib bench; do for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $R/$O/pmc/${m}_$c -o p -- python $R/profiles/pmc_probe.py $m > $R/$O/pmc/${m}_$c.log 2>&1
done; done
cd $R
python profiles/rocpd_summary.py $O/prof_seq/r04_results.db 40 > $O/stats_seq.txt
python profiles/rocpd_timeline.py $O/prof_seq/r04_results.db -4 > $O/timeline_seq.txt
python profiles/pmc_summary.py $O/pmc --json $O/traffic.json > $O/pmc_hbm_traffic.txt 2>&1
rm -rf $O/prof_seq
find $O/pmc -name "*kernel_trace.csv" -size +20M -delete
# the bench lines read profiles/traffic.json: put the fresh one in place first
cp $O/traffic.json profiles/traffic.json
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; tail -3 $O/bench_default.err
python bench.py --full --steps 20 --warmup 5 --no_cpu_baseline > $O/bench_driver_args.json 2>/dev/null
python bench.py --full --force_sharded --no_cpu_baseline 2>/dev/null | tail -1 > $O/bench_sharded_w1.json
