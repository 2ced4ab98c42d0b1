O=${O:-$(mktemp -d)}
for v in 1 0; do LH_SC_EQ_FACTORING=$v LH_HP_DEBUG=1 python bench.py --workload hyperplonk --log-n 20 --full --no-cpu-baseline 2> $O/hp_dbg_$v.err | python -c "import json,sys; d=json.loads(sys.stdin.read()); print(d['value'], [(k['name'],k['launches'],round(k['ms'],2)) for k in d['kernels'][:14]])"; grep "\[expr\]" $O/hp_dbg_$v.err | sort | uniq -c | head -12; done
