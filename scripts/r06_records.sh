#!/bin/bash
# the round's records in one GPU session: bash scripts/r06_records.sh TAG OUTDIR
TAG=${1:-r06a}; OUT=${2:?usage: r06_records.sh TAG OUTDIR}
git rev-parse --short HEAD > .commit_id 2>/dev/null
python bench.py --full --steps 20 --warmup 5 2> $OUT/${TAG}_bench.err | tail -1 > $OUT/${TAG}_bench.json; echo "bench rc=$?"
cp bench_detail.json $OUT/${TAG}_bench_detail.json
cd /tmp; export TMPDIR=/tmp; cd "$GRAFT_REPO_ROOT"
for leg in headline tolbatch ba; do
  rm -rf $OUT/prof_$leg
  rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$leg -o $leg -- python3 bench.py --only $leg --steps 20 --warmup 5 > $OUT/${TAG}_${leg}_profiled.json 2>/dev/null
  cp $OUT/prof_$leg/${leg}_kernel_stats.csv $OUT/${TAG}_${leg}_kernel_stats.csv
  tail -1 $OUT/${TAG}_${leg}_profiled.json > $OUT/${TAG}_${leg}_profiled.json.tmp && mv $OUT/${TAG}_${leg}_profiled.json.tmp $OUT/${TAG}_${leg}_profiled.json
  rm -rf $OUT/prof_$leg
done
bash scripts/tol_pmc.sh 128 u8 $OUT/${TAG}_pmc_pyramid_batch_s128.json | tail -4
bash scripts/tol_pmc.sh 128 u8tol $OUT/${TAG}_pmc_pyramid_tol_batch_s128.json | tail -4
head -c 600 $OUT/${TAG}_bench.json; echo
bash scripts/ba_mfma_pmc.sh $OUT/${TAG}_ba_mfma_pmc.txt | tail -40
bash scripts/ba_batch_prof.sh 128 ${TAG}_p20 P20 | head -12 > $OUT/${TAG}_ba_batch_p20_kernels.txt; cat $OUT/${TAG}_ba_batch_p20_kernels.txt
