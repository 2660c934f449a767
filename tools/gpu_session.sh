#!/bin/bash
# One GPU-box session: GPU tests, bench line, rocprofv3 kernel trace of the bench.  usage: tools/gpu_session.sh <tag> [pytest -k expr] (results: $MUVO_PROFILE_OUT)
set -uo pipefail
: ${GRAFT_REPO_ROOT:?}
tag=$1; kexpr=${2:-}
R=$GRAFT_REPO_ROOT
out=${MUVO_PROFILE_OUT:?directory that receives the results}
mkdir -p $out && out=$(cd $out && pwd)
cd $R
if [ -n "$kexpr" ]; then
  python -m pytest tests -m gpu -q --maxfail=12 -k "$kexpr" > $out/${tag}_tests.log 2>&1
else
  python -m pytest tests -m gpu -q --maxfail=12 > $out/${tag}_tests.log 2>&1
fi
echo "pytest rc=$?" >> $out/${tag}_tests.log
tail -5 $out/${tag}_tests.log
python bench.py --steps 10 --warmup 3 --full --layer-table $out/${tag}_conv_layers.txt > $out/${tag}_bench.json 2> $out/${tag}_bench.err
echo "bench rc=$?"; cut -c1-600 $out/${tag}_bench.json
cd /tmp && export TMPDIR=/tmp
GPU_MAX_HW_QUEUES=8 rocprofv3 --kernel-trace --stats -d $out/prof_${tag} -o p -- python3 $R/bench.py --steps 8 --warmup 2 --no-cpu-baseline --no-kernel-timing --no-exact-f32 > $out/${tag}_prof.log 2>&1
cd $R
db=$(ls $out/prof_${tag}/*/p_results.db $out/prof_${tag}/p_results.db 2>/dev/null | head -1)
python tools/rocpd_stats.py $db --top 90 > $out/${tag}_kernel_stats.txt
rm -rf $out/prof_${tag}
head -30 $out/${tag}_kernel_stats.txt | cut -c1-160
