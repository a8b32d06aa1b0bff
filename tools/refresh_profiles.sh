cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
export O=${O:-out}      # output directory (git-ignored by default)
mkdir -p $O
python bench.py --full > $O/bench_final.json 2> $O/bench_final.err || exit 1
echo bench done
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof3 -- python3 bench.py --full --no-cpu > $O/prof3.log 2>&1 || exit 1
echo stats done
rocprofv3 --kernel-trace --pmc FETCH_SIZE --output-format csv -d $O/pmc_f -- python3 bench.py --full --no-cpu --steps 18 > $O/pmc_f.log 2>&1 || exit 1
rocprofv3 --kernel-trace --pmc WRITE_SIZE --output-format csv -d $O/pmc_w -- python3 bench.py --full --no-cpu --steps 18 > $O/pmc_w.log 2>&1 || exit 1
python tools/pmc_summary.py $O/pmc_f $O/pmc_w srl_k_render 111656960 > $O/render_pmc.json || exit 1
echo pmc done
python tools/stamps_render.py > $O/stamps.txt 2>&1 || exit 1
# (the ablation timings and instruction counts of round 1 came from build switches that are retired:
#  tools/experiments/render_ablation_switches.patch, profiles/README.md)
echo all done
# settle kernel counters (profiles/r01_settle_pmc.txt)
cd /tmp && cd $GRAFT_REPO_ROOT
rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS --output-format csv -d $O/pmc_s1 -- python3 bench.py --full --no-cpu --steps 18 > $O/pmc_s1.log 2>&1 || exit 1
rocprofv3 --kernel-trace --pmc SQ_INSTS_SMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAIT_INST_LDS --output-format csv -d $O/pmc_s2 -- python3 bench.py --full --no-cpu --steps 18 > $O/pmc_s2.log 2>&1 || exit 1
python tools/pmc_insts.py srl_k_step $O/pmc_s1 $O/pmc_s2 > $O/settle_pmc.txt
echo settle pmc done
