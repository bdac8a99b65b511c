#!/bin/bash
# usage (on an MI355X): tests/tools/prof_step.sh <tag> [bench.py arguments, default --no-graph]
#   -> $OUT_DIR (default out/): ss_<tag>.txt, timeline_<tag>.txt   (PAIRS=<pairs per step> when --batch is given: star_kernels.py needs it)
tag=${1:-x}
shift
extra=${@:---no-graph}
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT || exit 1
mkdir -p "${OUT_DIR:=out}"
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT_DIR/prof_$tag -o e -- python3 bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-online --no-dp-overhead --no-legs $extra > $OUT_DIR/be.log 2>$OUT_DIR/be.err || exit 1
trace=$(find $OUT_DIR/prof_$tag -name "e_kernel_trace.csv" | head -1)
python tests/tools/steady_state.py $trace 10 "$tag steady state ($extra)" > $OUT_DIR/ss_$tag.txt
python tests/tools/step_timeline.py $trace fastest > $OUT_DIR/timeline_$tag.txt
python tests/tools/forward_window.py $trace 10 > $OUT_DIR/fw_$tag.txt
python tests/tools/star_kernels.py $trace 10 ${PAIRS:-4} > $OUT_DIR/star_$tag.txt
cp $(find $OUT_DIR/prof_$tag -name "e_kernel_stats.csv" | head -1) $OUT_DIR/ks_$tag.csv
rm -rf $OUT_DIR/prof_$tag
tail -1 $OUT_DIR/be.log | cut -c1-120
