cd $GRAFT_REPO_ROOT
O=${O:-build/r6final2}; mkdir -p $O
(timeout 1800 python -m pytest tests -m gpu -q --timeout 1500 2>&1 | tail -8 > $O/gpu_tests.txt)
(timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.txt 2>&1)
(timeout 1200 python bench.py --full > $O/bench_default.json 2> $O/bench_default.err)
tail -3 $O/gpu_tests.txt; tail -1 $O/smoke.txt; python -c "
import json; j=json.loads(open('$O/bench_default.json').readline()); print(j['value'], j['roofline']['frac'], j['configs']['embedding_like_10Mx768']['qps'], j['configs']['c2_1Mx768_b1_latency']['value'])"
