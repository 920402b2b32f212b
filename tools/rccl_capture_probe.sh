#!/bin/bash
# Runs tools/rccl_capture_probe in its modes, each as its own process under a timeout, once each, and stops at the
# first mode that crashes (its exit code and the last step it printed say where).  Output: the file OUT names below.
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
OUT=$ROOT/gpurun_out/rccl_capture_probe.txt
BIN=$ROOT/tools/rccl_capture_probe
export NCCL_DEBUG=${NCCL_DEBUG:-WARN}
# PROBE_LIBDIR: run against another copy of librccl / the HIP runtime (e.g. the one PyTorch bundles)
if [ -n "$PROBE_LIBDIR" ]; then export LD_LIBRARY_PATH=$PROBE_LIBDIR:$LD_LIBRARY_PATH; OUT=${OUT%.txt}_$(basename $(dirname $PROBE_LIBDIR)).txt; fi
: > $OUT; ldd $BIN | grep -i "rccl\|amdhip" >> $OUT
for mode in origin fork-nonblocking fork-blocking fork-eager-first; do
  timeout -k 5 60 $BIN $mode >> $OUT 2>&1
  rc=$?
  echo "== mode $mode: exit code $rc" >> $OUT
  # 2: an API call returned an error (printed); anything else is a crash or a timeout: no further mode runs
  if [ $rc -ne 0 ] && [ $rc -ne 2 ]; then break; fi
done
cat $OUT
