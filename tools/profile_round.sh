# The rocprofv3 passes behind profiles/<tag>_* and profiles/traffic.json.  Run on the GPU box:  bash tools/profile_round.sh
# (kernel trace + stats of the default bench command, the full bench line, and three separate PMC passes -- FETCH_SIZE,
# WRITE_SIZE, SQ/GRBM -- at the default batch size; PMC and tracing domains are never combined).  Every bench run is a --full one:
# the profiles cover the by_launch passes and the standalone pooling kernel too.  Outputs go to $PROF_OUT (default prof_out/),
# where tools/write_profiles.py reads them.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
cd "$ROOT"
O=${PROF_OUT:-prof_out}
mkdir -p $O
rm -rf $O/prof_stats $O/prof_fetch $O/prof_write $O/prof_sq
rocprofv3 --kernel-trace --stats -d $O/prof_stats -- python bench.py --full --cpu-budget 0 --e2e-utts 0 --no-fp32-leg --no-extra-legs > $O/bench_under_prof.json 2> $O/prof_stats.err
python bench.py --full > $O/bench_plain.json 2> $O/bench_plain.err
rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $O/prof_fetch -- python bench.py --full --steps 1 --warmup 0 --cpu-budget 0 --e2e-utts 0 --no-fp32-leg --no-extra-legs > /dev/null 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $O/prof_write -- python bench.py --full --steps 1 --warmup 0 --cpu-budget 0 --e2e-utts 0 --no-fp32-leg --no-extra-legs > /dev/null 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_INSTS_MFMA SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE -d $O/prof_sq --kernel-trace -- python bench.py --full --steps 1 --warmup 0 --cpu-budget 0 --e2e-utts 0 --no-fp32-leg --no-extra-legs > /dev/null 2>&1
python tools/prof_summary.py stats $(find $O/prof_stats -name "*.db" | head -1) > $O/round_stats.txt
: > $O/round_pmc.txt
for d in prof_fetch prof_write prof_sq; do python tools/prof_summary.py pmc $(find $O/$d -name "*.db" | head -1) >> $O/round_pmc.txt; done
rm -rf $O/prof_stats $O/prof_fetch $O/prof_write $O/prof_sq
