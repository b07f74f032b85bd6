#!/bin/bash
# tools/measure_build.sh LABEL [LIB] : what a change to a frame kernel is judged by, for ONE build of libkwy.so (LIB, a
# path relative to the repository root, is copied over kwiiyatta_amd/libkwy.so first; default: the library in the tree),
# written to $KWY_MEASURE_OUT/LABEL/ (default: measure_out/LABEL/ in the repository root):
#   bench.json                the default bench line; its --dump-outputs arrays in dump/
#   serial_kernel_stats.csv   rocprofv3 --kernel-trace --stats of `bench.py --driver serial` (per-launch durations)
#   pmc_summary.json          SQ counters of the frame kernels (tools/pmc_sq_summary.py), two counter-ONLY passes
#                             (no tracing beside --pmc) of one wave of 16 pairs, kernel by kernel
# Run it for both builds in one session on one machine (boxes differ by ~2 % in clocks), then compare the dumps with
# numpy on the host.  Every GPU step runs under its own time limit and the script stops at the first failure.
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=${KWY_MEASURE_OUT:-$R/measure_out}/$1
mkdir -p $O
cd $R
if [ -n "$2" ]; then cp "$R/$2" $R/kwiiyatta_amd/libkwy.so || exit 1; fi
timeout -k 10 300 python bench.py --dump-outputs $O/dump > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/serial -- python $R/bench.py --driver serial --steps 10 --warmup 10 > $O/serial.log 2>&1 || { tail -20 $O/serial.log; exit 1; }
cp "$(ls -t $O/serial/*/*kernel_stats.csv | head -1)" $O/serial_kernel_stats.csv
rm -rf $O/serial
CMD="python $R/bench.py --driver serial --batch 16 --steps 2 --warmup 1 --no-graph"
timeout -k 10 400 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_INSTS_VALU GRBM_GUI_ACTIVE \
  --output-format csv -d $O/pass1 -- $CMD > $O/pass1.log 2>&1 || { tail -20 $O/pass1.log; exit 1; }
timeout -k 10 400 rocprofv3 --pmc SQ_WAVES SQ_INSTS_LDS SQ_INSTS_SALU SQ_INSTS_VMEM_RD SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_ACTIVE_INST_SCA \
  --output-format csv -d $O/pass2 -- $CMD > $O/pass2.log 2>&1 || { tail -20 $O/pass2.log; exit 1; }
python $R/tools/pmc_sq_summary.py $O > $O/pmc_summary.json
echo done > $O/DONE
