# End-of-round records (on an MI355X: tools/round_profiles.sh OUTDIR); copy what matters to profiles/.
# Every GPU step has its own time limit, and the script stops at the first step that fails.
set -eu
O=$(mkdir -p "${1:?usage: tools/round_profiles.sh OUTDIR}" && cd "$1" && pwd)
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
export T=${T:-r04}
timeout -k 10 300 python3 $R/bench.py --full > $O/${T}_bench_distM.json 2> $O/${T}_bench_distM.err
timeout -k 10 300 python3 $R/bench.py --loc-dist I > $O/${T}_bench_distI.json 2> $O/${T}_bench_distI.err
rm -rf $O/stats_b
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_b -- python3 $R/bench.py > $O/stats_b.log 2>&1
find $O/stats_b -name "*kernel_stats.csv" -exec cp {} $O/${T}_bench_kernel_stats_batch128_distM.csv \;
find $O/stats_b -name "*.csv" -size +1M -delete
timeout -k 10 600 python3 $R/tools/bench_msda_op.py --shapes P2 --batches 8,32,128 --dists I,M,U --dtypes f32 > $O/${T}_op_col_P2.txt 2> $O/${T}_op.err
timeout -k 10 600 python3 $R/tools/bench_msda_op.py --shapes P1,P4 --batches 8,128 --dists I,M --dtypes f32 >> $O/${T}_op_col_P2.txt 2>> $O/${T}_op.err
timeout -k 10 600 python3 $R/tools/bench_msda_op.py --shapes P3 --batches 1,4 --dists I,M,U --dtypes f16,bf16 --iters 50 > $O/${T}_op_col16_P3.txt 2>> $O/${T}_op.err
timeout -k 10 600 python3 $R/tools/bench_msda_op.py --shapes P2 --batches 8,128 --dists I,M --dtypes f16,bf16 >> $O/${T}_op_col16_P3.txt 2>> $O/${T}_op.err
# MSDeformAttn backward (pyramid-column kernel): op table, kernel stats (rocprofv3) of the op bench
bash $R/tools/record_bwd.sh $O > $O/${T}_bwd_record.txt 2>&1
