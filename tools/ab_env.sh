# same-box A/B of two environments on the headline step: bash tools/ab_env.sh OUT "ENV_A" "ENV_B" [rounds] [bench.py arguments...]
#   e.g. bash tools/ab_env.sh ab1 "ASD_GEMM_PLAN_FILE=tools/data/gemm_plans_r02.json" "" 3
#        bash tools/ab_env.sh ab2 "ASD_HIP_LIB=scaledreamer_amd/variants/libasd_hip_NAME.so" "" 3 --workload W
# every bench.py runs under its own time limit; the first one that fails ends the script (nothing more is started on the GPU)
O=gpurun_out/${1:-ab}; mkdir -p $O; : > $O/ab.txt
A="$2"; B="$3"; N=${4:-3}
shift $(( $# < 4 ? $# : 4 ))
for i in $(seq 1 $N); do
  for v in A B; do
    if [ $v = A ]; then E="$A"; else E="$B"; fi
    env $E timeout -k 10 600 python bench.py --steps 30 --warmup 8 --no-cpu-baseline "$@" > $O/last.txt 2>/dev/null
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v round $i: bench.py exit $rc, stopping" | tee -a $O/ab.txt; exit $rc; fi
    python -c "import sys,json; d=json.loads(open('$O/last.txt').read().strip().splitlines()[-1]); print('$v', d['ms_per_step'], d['value'], d.get('gpu_ms_per_step_median', ''))" >> $O/ab.txt || exit 1
  done
done
cat $O/ab.txt
