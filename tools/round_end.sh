#!/bin/bash
# Round-end GPU run: the whole -m gpu suite, then tools/final_measure.sh (bench lines, rocprofv3 summaries, PMC passes).
#   gpurun --timeout 3600 -- "bash tools/round_end.sh <tag> <commit>"
TAG=${1:-r04}; COMMIT=${2:-unknown}
# tools/final_measure.sh writes the bench records to $RECORD_DIR and tools/collect_record.sh reads them from there: it must name a
# directory that comes back with the logs below, so it is asked for here instead of falling back to bench_records/ on the GPU box
export RECORD_DIR=${RECORD_DIR:?"set RECORD_DIR to where the bench records go (a directory that comes back with the logs of this run)"}
timeout 2400 python -m pytest tests -q -x -m gpu > gpurun_out/${TAG}_round_end_tests.log 2>&1; echo "tests rc=$?"; tail -3 gpurun_out/${TAG}_round_end_tests.log | cut -c1-200
timeout 900 python -m pytest tests -q -m perf > gpurun_out/${TAG}_round_end_perf.log 2>&1; echo "perf rc=$?"; tail -3 gpurun_out/${TAG}_round_end_perf.log | cut -c1-200
bash tools/final_measure.sh $TAG $COMMIT > gpurun_out/${TAG}_final_measure.log 2>&1; tail -30 gpurun_out/${TAG}_final_measure.log | cut -c1-200
