#!/bin/bash
# Run GPU steps in order; stop at the first step that did not exit cleanly (0) or with an ordinary
# test failure (1).  Faults / aborts / timeouts (124, 134, 137, 139, ...) end the session.
# usage: tools/gpu_session.sh "<name>:<timeout_s>:<command>" ...
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${TMAE_OUT_DIR:-bench_out}  # where logs, traces and profiles go
mkdir -p $OUT
export HSA_ENABLE_IPC_MODE_LEGACY=0
for spec in "$@"; do
  name="${spec%%:*}"; rest="${spec#*:}"; tmo="${rest%%:*}"; cmd="${rest#*:}"
  echo "=== $name (timeout ${tmo}s): $cmd" | tee -a $OUT/session.log
  start=$(date +%s)
  timeout -k 10 "$tmo" bash -c "$cmd" > "$OUT/$name.log" 2>&1
  rc=$?
  echo "=== $name rc=$rc ($(( $(date +%s) - start ))s)" | tee -a $OUT/session.log
  tail -5 "$OUT/$name.log"
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stopping: $name rc=$rc"; exit $rc; fi
done
exit 0
