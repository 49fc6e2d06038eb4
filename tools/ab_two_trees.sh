#!/bin/bash
# Same-box comparison of TWO BUILT CHECKOUTS on the whole bench (box-to-box spread on the pool is +-3 %: a commit is only ever
# compared with its parent on one box, in one session, arms alternating):
#   bash tools/ab_two_trees.sh <parent checkout> <branch checkout> [rounds=3] [out dir=ab_out]
# Both trees must have been built (python __graft_entry__.py).  Every run has its own time limit and the first failure ends the
# script.  Prints one line per run and a summary: per-arm median, the parent's own spread (max - min) and the drop.
set -uo pipefail
parent="$(cd "$1" && pwd)"; branch="$(cd "$2" && pwd)"; rounds=${3:-3}; out=${4:-ab_out}
mkdir -p "$out"; out="$(cd "$out" && pwd)"
: > "$out/rounds.txt"
for r in $(seq 1 "$rounds"); do
  for arm in parent branch; do
    if [ "$arm" = parent ]; then dir="$parent"; else dir="$branch"; fi
    (cd "$dir" && timeout -k 10 240 python bench.py --gpus 1 --steps 20 --warmup 5 2> "$out/${arm}_$r.err" | tail -1 > "$out/${arm}_$r.json")
    rc=$?
    if [ $rc -ne 0 ]; then echo "$arm round $r failed rc=$rc"; tail -5 "$out/${arm}_$r.err"; exit $rc; fi
    python -c "
import json
d = json.load(open('$out/${arm}_$r.json'))
print(f\"round $r $arm ms_per_step {d['ms_per_step']:.3f} images/s {d['value']:.2f} self_check {d['self_check']}\")" | tee -a "$out/rounds.txt"
  done
done
python -c "
import re, statistics
v = {'parent': [], 'branch': []}
for line in open('$out/rounds.txt'):
    m = re.match(r'round \d+ (\w+) ms_per_step ([\d.]+)', line)
    if m: v[m.group(1)].append(float(m.group(2)))
p, b = v['parent'], v['branch']
print(f'parent median {statistics.median(p):.3f} ms (spread {max(p) - min(p):.3f}), branch median {statistics.median(b):.3f} ms (spread {max(b) - min(b):.3f}), '
      f'drop {statistics.median(p) - statistics.median(b):.3f} ms = {100 * (1 - statistics.median(b) / statistics.median(p)):.2f} %')" | tee -a "$out/rounds.txt"
