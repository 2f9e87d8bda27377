# A B A B of two library builds (ab_libs/a.so, ab_libs/b.so) through bench.py --full; outputs under $1 (default ab_out/).
OUT=${1:-ab_out}
mkdir -p $OUT
for r in 1 2; do
for v in a b; do
LAVIE_HIP_LIB=$PWD/ab_libs/$v.so python bench.py --full --steps 2 --warmup 1 --cpu-steps 0 --no-extra-legs > $OUT/ab_pk_$v$r.json 2> $OUT/ab_pk_$v$r.err || exit 1
python - <<PY
import json
d=json.loads(open("$OUT/ab_pk_$v$r.json").read().strip().splitlines()[-1])
print("$v$r", d["value"], d["ms_per_step"], [(c["name"][:14], c["ms"]) for c in d["kernel_breakdown"]["classes"] if c["ms"]])
PY
done; done
