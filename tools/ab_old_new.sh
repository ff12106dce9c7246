cd $GRAFT_REPO_ROOT
run() { env "$@" timeout 120 python bench.py --full --no-cpu-baseline --no-traffic --no-full-check --steps 20 --warmup 5 2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d['roofline']; n=d['north_star_variant']
print(' '.join(sys.argv[1:]), '|', r['kernel'], 'kernel_ms', round(r['kernel_ms'],4), 'frac', round(r['frac'],4), '| ns', round(n['kernel_ms'],4), round(n['roofline_frac'],4))
" "$@"; }
OLD=PG_GPU_LIB=$PWD/tools/variants/libpinot_gpu_old.so
for i in 1 2 3; do
  run $OLD PG_NO_PIPE=1; run X=new PG_NO_PIPE=1; run $OLD; run X=new
done
