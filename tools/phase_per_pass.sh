#!/bin/bash
# mean wavefront time per pass of the persistent loop, per phase (development builds with -DM4Q_DEV_PHASE_CLOCK):
#   tools/phase_per_pass.sh <lib> [ENV=VAL ...]     -> ns per pass for backward / forward and the launch time
# A slot named "a | b" is a in a clipped kernel and b in an exact one (the exact-only slots tell which ran).  A clipped kernel splits
# "step done" (slots 10, 11, 13): "step: bookkeeping, us", "step: plant to xs", "step: exit, rest"; "step done (plant)" is then what is
# left of it, the passes in which no row ends a step, and "step done, all" their sum.
lib=$1; shift
for kv in "$@"; do export "$kv"; done
M4Q_LIB=$lib M4Q_PHASE_TRACE=1 python bench.py --steps 3 --warmup 1 --no-cpu-baseline $M4Q_BENCH_ARGS 2>&1 | python3 -c "
import sys, json, re
t = {}; ms = None
for line in sys.stdin:
    m = re.match(r'm4q phase (.*?)\s+(\d+)( ticks)?', line)
    if m: t[m.group(1).strip()] = int(m.group(2))
    if line.startswith('{'): ms = json.loads(line)['roofline']['avg_launch_ms']
p = t.get('passes', 1)
exact = any(v > 0 for k, v in t.items() if k.startswith('exact:'))        # slots only an exact kernel fills
pick = lambda k: k.split('|')[-1 if exact else 0].strip()
t = {pick(k): v for k, v in t.items() if exact or not pick(k).startswith('exact')}
out = ['%s %.0f' % (k, 10.0 * v / p) for k, v in t.items() if v > 0 and 'passes' not in k]
if any(k.startswith('step:') and v > 0 for k, v in t.items()): out.append('step done, all %.0f' % (10.0 * sum(v for k, v in t.items() if k.startswith('step')) / p))
print('launch %.2f ms | ns per pass: %s' % (ms or -1, '; '.join(out)))
"
