# A/B of library variants on the bench's isolated kernel times: VARS="a b" ARGS="--steps 10" -> $MIM_OUT/ab_<v>_<i>.log (default bench_out/)
set -e
cd $GRAFT_REPO_ROOT
O=${MIM_OUT:-bench_out}
mkdir -p $O
for i in 1 2; do
  for v in ${VARS}; do
    MIM_LIB=$PWD/computervision_objectdetection_featurematching_amd/lib/variants/libmim_$v.so timeout -k 10 200 python3 bench.py --full --cpu-sample 0 ${ARGS:---steps 10} > $O/ab_${v}_$i.log 2>&1
  done
done
