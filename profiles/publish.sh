# Copies what profiles/collect.sh left in $O/ to the tracked names of this round (run from the repo root).
O=${O:-out}                   # where profiles/collect.sh left its files
R=${1:-r06}
cp $O/final_pytest.txt profiles/${R}_pytest_gpu.txt
for n in default driver_args zerocopy seq lfu staged unchanged_trainer sharded_w1 torchrun1 interleaved overlap share2 share3; do
  cp $O/bench_$n.json profiles/${R}_bench_$n.json
done
cp $O/stats_seq.txt profiles/${R}_kernel_stats_criteo1tb_seq.txt
cp $O/stats_ov.txt profiles/${R}_kernel_stats_criteo1tb_default_profiled.txt
cp $O/stats_il.txt profiles/${R}_kernel_stats_criteo1tb_interleaved_profiled.txt
cp $O/stats_k1.txt profiles/${R}_kernel_stats_kaggle_p1_interleaved_profiled.txt
cp $O/timeline_il.txt profiles/${R}_timeline_one_window_interleaved_profiled.txt
cp $O/timeline_k1.txt profiles/${R}_timeline_kaggle_p1_interleaved_profiled.txt
cp $O/sharded_terms.md profiles/${R}_sharded_terms.md
cp $O/timeline_seq.txt profiles/${R}_timeline_one_window_seq.txt
cp $O/timeline_ov.txt profiles/${R}_timeline_one_window_default_profiled.txt
cp $O/pmc_hbm_traffic.txt profiles/${R}_pmc_hbm_traffic.txt
cp $O/traffic.json profiles/traffic.json
cp $O/config_matrix.md profiles/${R}_config_matrix.md
for n in overlap interleaved auto unchanged tunable graph graph_tunable; do
  [ -f $O/dlrm_main_$n.json ] && cp $O/dlrm_main_$n.json profiles/${R}_dlrm_main_criteo1tb_$n.json
done
