#!/bin/bash
# Interleaved A/B of library builds and environments over bench.py, one JSON line per (round, leg),
# with the serial-leg kernel times (--full --no-cpu).  On the GPU box, from the repository root:
#   bash profiles/ray_tiles/gpu_ab.sh <out dir> <rounds> name=lib[,ENV=V] ...
# lib "" = the built library; e.g.
#   parent=noetic-slam_amd/lib/var/libtsdf_hip_parent.so new= off=,TSDF_RAY_TILES=0
# A leg that fails ends the call.
set -o pipefail
export TMPDIR=/tmp
O=$1; R=$2; shift 2
mkdir -p $O
for i in $(seq 1 $R); do
  for nl in "$@"; do
    n=${nl%%=*}; rest=${nl#*=}; lib=${rest%%,*}; envs=""
    [ "$rest" != "$lib" ] && envs=${rest#*,}
    env TSDF_HIP_LIB=$lib $envs timeout -k 10 200 python3 bench.py --no-cpu --full --steps 32 $BENCH_ARGS > $O/${n}_$i.json 2> $O/${n}_$i.err || { tail -3 $O/${n}_$i.err; exit 1; }
    python3 -c "import json; d=json.load(open('$O/${n}_$i.json')); print('${n}_$i', d['value'], d['ms_per_step'], d.get('serial_kernel_ms_per_launch'))"
  done
done
