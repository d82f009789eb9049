#!/bin/bash
# Same-box A/B of library builds: tools/ab_bench.sh <out dir> <rounds> <name> [<name> ...]   (name = variants/<name>.so, or "head" = the tree's own build)
# Alternates the builds <rounds> times with the driver's bench command (short form) and prints ms per batch of each run.
# AB_ARGS: further bench.py arguments (a later --steps / --warmup wins).  A run that fails or runs into its time limit ends the
# script (the tree's own build is put back first): nothing more is started on a GPU that may have faulted.
set -u
O=$1; R=$2; shift 2
mkdir -p $O
LIB=prompt-free-diffusion_amd/libpfd_hip.so
cp $LIB $O/head.so
for i in $(seq 1 $R); do
  for n in "$@"; do
    if [ "$n" = head ]; then cp $O/head.so $LIB; else cp variants/$n.so $LIB; fi
    timeout -k 10 600 python bench.py --steps 6 --warmup 2 --no-cpu-baseline --no-prof ${AB_ARGS:-} > $O/bench_${n}_$i.json 2> $O/bench_${n}_$i.err
    rc=$?
    if [ $rc -ne 0 ]; then
      cp $O/head.so $LIB; rm -f $O/head.so
      echo "$n run $i: bench.py exit status $rc"; tail -5 $O/bench_${n}_$i.err
      exit $rc
    fi
    echo "$n run $i: $(python -c "import json; d=json.load(open('$O/bench_${n}_$i.json')); print(round(d['ms_per_step'],2), 'ms/batch', round(d['value'],3), 'images/s')" 2>&1 | tail -1)"
  done
done
cp $O/head.so $LIB; rm -f $O/head.so
