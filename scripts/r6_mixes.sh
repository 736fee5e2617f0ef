set -o pipefail
O=${OUT:-bench_out}/r6
mkdir -p $O
for m in slo phase-ts 8mix; do
  timeout -k 10 420 python -u bench.py --full --mix $m --reps 3 --steps 20 --warmup 3 --no-cu-check --out $O/s1_$m.json > $O/s1_$m.log 2>&1 || exit $?
done
