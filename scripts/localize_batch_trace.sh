#!/bin/bash
# Kernel trace of agh_localize_batch alone (8 C2-style captures; 4 host-buffer and 4 device calls, warm-up included): every kernel's launch count and time, to check that the
# preprocessing, compaction and handle-search kernels run once per batch, not once per capture.
#   scripts/localize_batch_trace.sh <output dir>
set -euo pipefail
out=${1:-localize_batch_trace}
cd "$(dirname "$0")/.."
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$out" -o run -- python scripts/localize_batch_bench.py --reps 1 --batches 8 --batch-only
