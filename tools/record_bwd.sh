# MSDeformAttn backward records (on an MI355X: tools/record_bwd.sh OUTDIR): op tables of both kernels, kernel stats of the op
# bench under rocprofv3; prints a summary.  Every GPU step has its own time limit, and the script stops at the first that fails.
set -eu
O=$(mkdir -p "${1:?usage: tools/record_bwd.sh OUTDIR}" && cd "$1" && pwd)
R=$(cd "$(dirname "$0")/.." && pwd)
cd /tmp && export TMPDIR=/tmp
T=${T:-r03}
timeout -k 10 600 python3 $R/tools/bench_msda_bwd.py --cases P1:8,P2:2,P2:8,P2:32,P2:128 --dists I,M,U 2> $O/${T}_bwd.err > $O/${T}_bwd_op_P2_col.txt
PCT_MSDA_BWD_KERNEL=win timeout -k 10 300 python3 $R/tools/bench_msda_bwd.py --cases P1:1,P1:2,P1:4,P2:1,P2:2 --dists I,M 2>> $O/${T}_bwd.err > $O/${T}_bwd_small_win.txt
PCT_MSDA_BWD_KERNEL=col timeout -k 10 300 python3 $R/tools/bench_msda_bwd.py --cases P1:1,P1:2,P1:4,P2:1,P2:2 --dists I,M 2>> $O/${T}_bwd.err > $O/${T}_bwd_small_col.txt
rm -rf $O/stats_bwd
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats_bwd -- python3 $R/tools/bench_msda_bwd.py --cases P2:2,P2:8,P2:32 --dists M > $O/${T}_bwd_op_M_rocprof.txt 2>&1
find $O/stats_bwd -name "*kernel_stats.csv" -exec cp {} $O/${T}_bwd_col_kernel_stats_P2_distM.csv \;
find $O/stats_bwd -name "*.csv" -size +1M -delete
cat $O/${T}_bwd_op_P2_col.txt; echo; paste -d'\n' $O/${T}_bwd_small_win.txt $O/${T}_bwd_small_col.txt; head -4 $O/${T}_bwd_col_kernel_stats_P2_distM.csv | cut -c1-200
