#!/usr/bin/env python3
"""The times of the runs beside this file, side by side, with the rule of profiles/image_core/README.md applied: both new
runs no slower than the slower parent run plus the distance between the parent's two.  usage: bench_lines.py > bench_lines.md"""
import glob
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
SKIP = ("device", "rays", "rows", "generations", "window_ms", "repeats", "steps", "ms_min", "ms_max")
DERIVED = ("terms", "retraces_ms", "with_sensitivity_ms")  # (tolerance_bench: sums and multiples of figures that have their own line)


def figures(path):
    """{(label of the line, key): milliseconds} of one run: every key that ends in ms."""
    out = {}
    for line in open(path):
        rec = json.loads(line)
        label = " ".join(f"{k}={v}" for k, v in rec.items() if k not in SKIP and isinstance(v, (str, int)))
        for key, value in rec.items():
            if key.endswith("ms") and key not in SKIP + DERIVED and isinstance(value, float):
                out[(label, key)] = value
    return out


inside = total = 0
print("| bench | figure | new 1 | parent 1 | new 2 | parent 2 | limit | |\n|---|---|---|---|---|---|---|---|")
for first in sorted(glob.glob(os.path.join(HERE, "*_bench.new1.jsonl"))):
    bench = os.path.basename(first)[:-len(".new1.jsonl")]
    runs = {run: figures(os.path.join(HERE, f"{bench}.{run}.jsonl")) for run in ("new1", "parent1", "new2", "parent2")}
    for key in runs["new1"]:
        n1, p1, n2, p2 = (runs[run][key] for run in ("new1", "parent1", "new2", "parent2"))
        limit = max(p1, p2) + abs(p1 - p2)
        ok = max(n1, n2) <= limit
        inside, total = inside + ok, total + 1
        print(f"| {bench} | {key[0]} {key[1]} | {n1:.4f} | {p1:.4f} | {n2:.4f} | {p2:.4f} | {limit:.4f} | "
              f"{'inside' if ok else f'OUTSIDE {100 * (max(n1, n2) / limit - 1):+.1f} %'} |")
print(f"\n{inside} of {total} figures inside.")
