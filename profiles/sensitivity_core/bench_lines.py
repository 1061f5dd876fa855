"""The four runs of each bench side by side with the rule applied: both new runs no slower than the slower parent run plus
the distance between the parent's two.  python profiles/sensitivity_core/bench_lines.py DIR > bench_lines.md"""
import json
import os
import sys

d = sys.argv[1]
print("| bench | figure | new 1 | parent 1 | new 2 | parent 2 | allowed | |")
print("|---|---|---|---|---|---|---|---|")
inside = total = 0
for bench in ("sensitivity_bench", "design_sensitivity_bench", "opd_sensitivity_bench", "launch_sensitivity_bench"):
    runs = {}
    for run in ("new1", "parent1", "new2", "parent2"):
        for line in open(os.path.join(d, f"{bench}.{run}.jsonl")):
            rec = json.loads(line)
            if "ms" not in rec:
                continue
            key = rec["what"] + (f" K={rec['K']}" if "K" in rec else "")
            runs.setdefault(key, {})[run] = rec["ms"]
    for key, r in runs.items():
        if len(r) != 4:
            continue
        allowed = max(r["parent1"], r["parent2"]) + abs(r["parent1"] - r["parent2"])
        ok = r["new1"] <= allowed and r["new2"] <= allowed
        total += 1
        inside += ok
        print(f"| {bench} | {key} | {r['new1']:.4f} | {r['parent1']:.4f} | {r['new2']:.4f} | {r['parent2']:.4f} | {allowed:.4f} | "
              f"{'inside' if ok else 'OUTSIDE %+.1f %%' % (100 * (max(r['new1'], r['new2']) / allowed - 1))} |")
print(f"\n{inside} of {total} figures inside (ms).")
