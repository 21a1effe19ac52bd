# Regenerates every artefact under profiles/ (r06_*) on an MI355X box (run from the repo root; writes to $O/).
# NOTE on rocprofv3: with the profiler attached the HIP runtime executes hipMemcpyAsync as a blit KERNEL
# (__amd_rocclr_copyBuffer) instead of an SDMA transfer (profiles/r02_probe_sdma.txt), so a profiled run of the
# default (worker-transport) pipeline shows copy kernels that an unprofiled run does not have, and runs slower.
# Kernel durations for the roofline therefore come from the sequential zero-copy run (every kernel alone on the GPU).
set -x
R=$PWD
O=${O:-out}; export O          # where the run's files go (relative to the repo root)
mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -x -q 2>&1 | tail -3 > $O/final_pytest.txt; cat $O/final_pytest.txt
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; tail -3 $O/bench_default.err
python bench.py --full --steps 20 --warmup 5 --no_cpu_baseline > $O/bench_driver_args.json 2>/dev/null
python bench.py --full --no_cpu_baseline --transport zerocopy > $O/bench_zerocopy.json 2>/dev/null
python bench.py --full --no_cpu_baseline --no_overlap > $O/bench_seq.json 2>/dev/null
python bench.py --full --no_cpu_baseline --use_lfu > $O/bench_lfu.json 2>/dev/null
python bench.py --full --no_cpu_baseline --async_copy 2>/dev/null | tail -1 > $O/bench_staged.json
python bench.py --full --no_cpu_baseline --unchanged_trainer 2>/dev/null | tail -1 > $O/bench_unchanged_trainer.json
python bench.py --full --force_sharded --no_cpu_baseline 2>/dev/null | tail -1 > $O/bench_sharded_w1.json
python bench.py --full --no_cpu_baseline --arrangement interleaved 2>/dev/null | tail -1 > $O/bench_interleaved.json
python bench.py --full --no_cpu_baseline --arrangement overlap 2>/dev/null | tail -1 > $O/bench_overlap.json
python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 1 --steps 64 --warmup 16 --no_cpu_baseline 2>/dev/null | tail -1 > $O/bench_torchrun1.json
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $R/$O/prof_seq -o r06 -- python $R/bench.py --full --no_cpu_baseline --no_verify --no_overlap --no_graph --transport zerocopy > $R/$O/prof_seq.log 2>&1
rocprofv3 --kernel-trace --stats -d $R/$O/prof_ov -o r06 -- python $R/bench.py --full --no_cpu_baseline --no_verify > $R/$O/prof_ov.log 2>&1
rocprofv3 --kernel-trace --stats -d $R/$O/prof_il -o r06 -- python $R/bench.py --full --no_cpu_baseline --no_verify --arrangement interleaved > $R/$O/prof_il.log 2>&1
rocprofv3 --kernel-trace --stats -d $R/$O/prof_k1 -o r06 -- python $R/bench.py --full --no_cpu_baseline --no_verify --workload criteo_kaggle --cache_ratio 0.05 --prefetch_num 1 --arrangement interleaved > $R/$O/prof_k1.log 2>&1
mkdir -p $R/$O/pmc
for m in calib bench; do for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $R/$O/pmc/${m}_$c -o p -- python $R/profiles/pmc_probe.py $m > $R/$O/pmc/${m}_$c.log 2>&1
done; done
cd $R
python profiles/rocpd_summary.py $O/prof_seq/r06_results.db 40 > $O/stats_seq.txt
python profiles/rocpd_summary.py $O/prof_ov/r06_results.db 40 > $O/stats_ov.txt
python profiles/rocpd_summary.py $O/prof_il/r06_results.db 40 > $O/stats_il.txt
python profiles/rocpd_summary.py $O/prof_k1/r06_results.db 40 > $O/stats_k1.txt
python profiles/rocpd_timeline.py $O/prof_seq/r06_results.db -4 > $O/timeline_seq.txt
python profiles/rocpd_timeline.py $O/prof_ov/r06_results.db steady > $O/timeline_ov.txt
python profiles/rocpd_timeline.py $O/prof_il/r06_results.db steady > $O/timeline_il.txt
python profiles/rocpd_timeline.py $O/prof_k1/r06_results.db steady > $O/timeline_k1.txt
python profiles/pmc_summary.py $O/pmc --json $O/traffic.json > $O/pmc_hbm_traffic.txt 2>&1
rm -rf $O/prof_ov $O/prof_seq $O/prof_il $O/prof_k1
find $O/pmc -name "*kernel_trace.csv" -size +20M -delete
du -sh $O
bash profiles/config_matrix.sh > $O/config_matrix.md 2>&1
# the default lines once more, now that profiles/traffic.json carries this build's digest (roofline.traffic)
cp $O/traffic.json profiles/traffic.json
python bench.py --full > $O/bench_default.json 2> $O/bench_default.err; tail -3 $O/bench_default.err
python bench.py --full --steps 20 --warmup 5 --no_cpu_baseline > $O/bench_driver_args.json 2>/dev/null
bash profiles/dlrm_main_run.sh > $O/dlrm_main_run.log 2>&1
python profiles/sharded_terms.py 2 4 8 > $O/sharded_terms.md 2>$O/sharded_terms.err
for W in 2 3; do
python -m torch.distributed.run --nnodes=1 --nproc-per-node $W --master-addr 127.0.0.1 --master-port 2951$W bench.py --full --gpus $W --share_gpu --verify_sharded --table_scale 0.25 --no_cpu_baseline 2>$O/share$W.err | tail -1 > $O/bench_share$W.json
done
