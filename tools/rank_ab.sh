#!/bin/bash
# rank A/B: tools/rank_bench.py on lib/variants/<name>.so (tools/build_variant.sh) and the
# default build in alternation, 4 rounds.  Every rank and the points-in call is a process of
# its own under its own time limit (a run takes ~10 s: torch's import, six ray-cast scenes,
# 54 steps -- 4 s of them at rank 16 on a build without the batched replay), so a run that is
# cut off names the step that ran out of time.  One JSON line per run in
# OUT/rb_<build>.<step>.<round>.json.  usage: tools/rank_ab.sh OUT VARIANT...
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
O=${1:?usage: tools/rank_ab.sh OUT VARIANT...}
shift
mkdir -p "$O"
run() {  # build, step name, round, time limit, rank_bench arguments
  local v=$1 step=$2 rep=$3 limit=$4
  shift 4
  if [ "$v" = default ]; then unset C3HLAC_LIB; else export C3HLAC_LIB=$R/mapping-private_amd/lib/variants/$v.so; fi
  timeout -k 10 "$limit" python3 "$R/tools/rank_bench.py" "$@" > "$O/rb_$v.$step.$rep.json" 2>> "$O/rb_err.log"
  local rc=$?
  if [ $rc -ne 0 ]; then echo "rank_ab: $v $step round $rep: exit status $rc" >&2; exit 3; fi
  tail -1 "$O/rb_$v.$step.$rep.json"
}
for rep in 1 2 3 4; do
  for v in "$@" default; do
    for rank in 1 2 4 16; do
      run "$v" rank$rank $rep 120 --ranks $rank --points 0
    done
    run "$v" points $rep 120 --ranks "" --points 64
  done
done
