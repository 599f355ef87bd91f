#!/bin/bash
# development aid (GPU box): the DESIGN section 5 table -- every BASELINE configuration that fits one GPU.
# Prints one summary line per configuration; the full bench lines (--full: the CPU baseline and the oracle check with them)
# go to $OUT/bench_configs.jsonl (OUT from the environment, default evidence/).
OUT=${OUT:-evidence}
mkdir -p "$OUT"; : > "$OUT/bench_configs.jsonl"
run() { python bench.py --full --steps 5 --warmup 2 --no-live-pmc "$@" 2>/dev/null | tee -a "$OUT/bench_configs.jsonl" | python -c "
import json,sys; d=json.loads(sys.stdin.read()); print('%-44s %9.0f MB/s %7.2f ms  %s exact=%s cpu=%s' % (' '.join(sys.argv[1:]), d['value'], d['ms_per_step'], d['stage_ms'], d.get('bit_exact_vs_oracle'), (d.get('cpu_baseline') or {}).get('value')))" "$@"; }
run --workload zeros
run --workload zeros --level default
run --workload random
run --workload enwik8
run --workload enwik8 --level fast
run --workload enwik8 --level best
run --workload silesia
