#!/bin/bash
# Diagnostic: rocprofv3 --pmc passes of vector-L1 (TCP) and address-unit (TA) counters over a
# short bench run (3 timed batches), one small counter group per run (two TA counters at most:
# a larger request is refused as exceeding the hardware) and no tracing beside it; per-kernel
# CSVs under <out>/<name>_{tcp,ta,vmem}/, <out> being $L1_OUT or build/l1_pass.
#   bash tools/diag/l1_pass.sh <name> <bench.py args...>
# then: python tools/diag/sq_summary.py <out>/<name>_tcp/run_counter_collection.csv <kernel substring>
# (profiles/r11_unpart_floor.txt: the final un-partition before and after the staged runs)
set -u
cd "$(dirname "$0")/../.."
ROOT=$(pwd)
OUT=${L1_OUT:-$ROOT/build/l1_pass}
mkdir -p "$OUT"
name=$1
shift
cd /tmp && export TMPDIR=/tmp
pass() {   # pass <suffix> <counters...>
    local sfx=$1; shift
    timeout -s KILL 60 rocprofv3 --pmc "$@" --output-format csv -d "$OUT/${name}_$sfx" -o run -- \
        python3 "$ROOT/bench.py" --steps 3 --warmup 1 --cpu-seconds 0 --no-host-buffer --no-strdir "${ARGS[@]}" || exit $?
}
ARGS=("$@")
pass tcp TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_GATE_EN1_sum TCP_PENDING_STALL_CYCLES_sum GRBM_GUI_ACTIVE
pass ta TA_TA_BUSY_sum TA_ADDR_STALLED_BY_TC_CYCLES_sum GRBM_GUI_ACTIVE
pass vmem TA_FLAT_WAVEFRONTS_sum SQ_INSTS_VMEM SQ_WAVES
