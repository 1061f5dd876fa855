"""Median duration per (kernel, workgroup grid) of a rocprofv3 --kernel-trace run: python profiles/sensitivity_core/kernel_medians.py DIR"""
import collections
import csv
import glob
import json
import os
import statistics
import sys

files = glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True)
assert files, f"no kernel trace under {sys.argv[1]}"
took = collections.defaultdict(list)
for path in files:
    for r in csv.DictReader(open(path)):
        name = r["Kernel_Name"].split("(")[0]
        if "k_sens" not in name and "k_opl" not in name and "k_frame" not in name:
            continue
        grid = "x".join(str(int(r[f"Grid_Size_{a}"]) // max(int(r[f"Workgroup_Size_{a}"]), 1)) for a in "XYZ")
        took[(name, grid)].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for (name, grid), us in sorted(took.items()):
    print(json.dumps({"kernel": name, "grid": grid, "launches": len(us), "median_us": statistics.median(us)}))
