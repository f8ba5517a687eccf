# Round profile of the headline benchmark: bench line, rocprofv3 kernel stats, five PMC passes
# (separate runs: --pmc must not be combined with tracing domains other than --kernel-trace).
#   bash tools/run_profile.sh r02       (on the GPU machine; OUT=<dir> picks the output folder)
# Outputs under $OUT (scratch, default profile_out/ in the repo root); copy the summaries you want judged into profiles/.
set -x
tag=${1:-r03}
export TMPDIR=/tmp
R=$(cd "$(dirname "$0")/.." && pwd)
out=${OUT:-$R/profile_out}
mkdir -p $out
cd $R
python bench.py --full > $out/bench_${tag}.json 2> $out/bench_${tag}.err
cd /tmp
rocprofv3 --kernel-trace --stats -d $out/prof_${tag} -- python $R/bench.py > $out/prof_${tag}.log 2>&1
for c in "SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY" "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD" "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_LDS_BANK_CONFLICT SQ_INST_CYCLES_SALU" "FETCH_SIZE" "WRITE_SIZE"; do
  n=$(echo $c | tr ' ' '_' | cut -c1-24)
  rocprofv3 --kernel-trace --pmc $c -d $out/pmc_${tag}_$n -- python $R/bench.py --steps 3 --warmup 1 > $out/pmc_${tag}_$n.log 2>&1
done
# LDS pipe of the headline kernel (index-active / conflict cycles, FIFO stalls, shader clock)
i=0
for c in "SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT SQ_LDS_UNALIGNED_STALL" "SQ_LDS_DATA_FIFO_FULL SQ_LDS_CMD_FIFO_FULL SQ_WAIT_INST_LDS SQ_INST_LEVEL_LDS" "GRBM_GUI_ACTIVE SQ_BUSY_CYCLES"; do
  i=$((i+1))
  rocprofv3 --kernel-trace --pmc $c -d $out/ldspmc_${tag}_$i -- python $R/bench.py --steps 3 --warmup 1 > $out/ldspmc_${tag}_$i.log 2>&1
done
cd $R
python tools/rocpd_summary.py $out/ldspmc_${tag}_* 2>&1 | grep -v "not a database\|\.log" > $out/${tag}_headline_lds_pmc.txt
python tools/rocpd_summary.py $out/prof_${tag} $out/pmc_${tag}_* 2>&1 | grep -v "not a database\|\.log" > $out/${tag}_headline_pmc.txt
python tools/pmc_to_json.py --kernel "mc_lean_kernel<2, 2, 1, false, 0, false, false, true" --replicas 4096 --mc 125000 --source profiles/${tag}_headline_pmc.txt $out/pmc_${tag}_* > $out/pmc_constants_${tag}.json
tail -c 600 $out/bench_${tag}.json
# the raw rocpd databases are scratch: keep the summaries only
rm -rf $out/prof_${tag} $out/pmc_${tag}_*/ $out/ldspmc_${tag}_*/
