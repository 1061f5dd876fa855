#!/usr/bin/env python3
"""The through-focus diffraction PSF (DeviceFrame.psf(focus=), RayTracer.trace_psf(focus=)) on BASELINE config 2, timed
against what it replaces.  Every figure is the median of --steps timed calls after warm-up, a host clock around work
that ends in a device synchronise; one JSON line per figure.

  scan       tracer.trace_psf(detector, pixels=n, focus=F planes): one trace, one wavefront, one call
  retrace    what a user did before: for each of the F shifts a detector moved by it, a trace and trace_psf(detector).
             The F tracers are built before the clock starts.
  gap        (--gap) on the singlet of examples/diffraction_focus.py, the Strehl ratio of the scan beside that of a
             re-trace behind a moved detector on three planes: two approximations of one field, the scan's reference
             sphere stays centred on the first detector's point (information, not a test)
  --kernels  only runs psf() and psf(focus=) --steps times per shape: the run to put under
             rocprofv3 --kernel-trace --output-format csv
  --summarise TRACE.csv  per (kernel, grid): launches, median / min / max microseconds of a kernel trace, JSON lines

usage: tools/psf_focus_bench.py [--rays N] [--steps K] [--pixels 64 128] [--planes 11 41] [--gap] [--kernels]"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summarise(path):
    """Per (kernel, grid in workgroups) of a rocprofv3 kernel trace: launches and microseconds."""
    rows = {}
    with open(path, newline="") as handle:
        for row in csv.DictReader(handle):
            name = row["Kernel_Name"].split("(")[0]
            grid = tuple(int(row[f"Grid_Size_{a}"]) // max(1, int(row[f"Workgroup_Size_{a}"])) for a in "XYZ")
            rows.setdefault((name, grid), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for (name, grid), us in sorted(rows.items()):
        if "psf" in name:
            print(json.dumps({"kernel": name, "grid_workgroups": list(grid), "launches": len(us),
                              "us_median": round(statistics.median(us), 1), "us_min": round(min(us), 1),
                              "us_max": round(max(us), 1), "us_total": round(sum(us), 1)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--pixels", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--planes", type=int, nargs="+", default=[11, 41])
    ap.add_argument("--gap", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--summarise")
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise)

    import numpy as np
    import torch

    import scenes
    import pyrayt_amd as pyrayt

    def tracer_at(det_x):
        pyrayt.g3d.objects.CountedObject.reset_ids()
        lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
        src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
        det = pyrayt.components.baffle((1, 1)).move_x(det_x)
        return pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays), det

    def median_ms(fn, warmup=1):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t) * 1e3)
        return statistics.median(times), min(times), max(times)

    tracer, det = tracer_at(1.0)
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "steps": args.steps}
    if args.kernels:
        frame = tracer.trace_device()
        for n in args.pixels:
            for _ in range(args.steps):
                frame.psf(det, world_unit_um=1000.0, pixels=n)
            for planes in args.planes:
                focus = np.linspace(-0.02, 0.02, planes)
                for _ in range(args.steps):
                    frame.psf(det, world_unit_um=1000.0, pixels=n, focus=focus)
        torch.cuda.synchronize()
        return
    for n in args.pixels:
        for planes in args.planes:
            focus = np.linspace(-0.02, 0.02, planes)
            moved = [tracer_at(1.0 + delta) for delta in focus]
            scan = median_ms(lambda: tracer.trace_psf(det, world_unit_um=1000.0, pixels=n, focus=focus))
            retrace = median_ms(lambda: [t.trace_psf(d, world_unit_um=1000.0, pixels=n) for t, d in moved])
            print(json.dumps({**common, "what": "scan_vs_retrace", "pixels": n, "planes": planes,
                              "scan_ms": scan[0], "scan_ms_min_max": scan[1:], "retrace_ms": retrace[0],
                              "retrace_ms_min_max": retrace[1:], "retrace_over_scan": retrace[0] / scan[0]}), flush=True)
    if args.gap:  # (on the example's singlet: config 2's cone of rays is one ring, whose Strehl ratio is 1 on every plane)
        sys.path.insert(0, os.path.join(ROOT, "examples"))
        import diffraction_focus as example

        rays, diameter = 32_000, 0.7
        found = example.main(rays, diameter, verbose=False)
        focus = np.array([0.0, 0.5 * found["diffraction"], found["diffraction"]])
        first, det0 = example.build(rays, diameter)
        scan = first.trace_psf(det0, world_unit_um=1000.0, pixels=8, focus=focus)
        fresh = []
        for delta in focus:
            moved, det1 = example.build(rays, diameter, 2.0 + delta)
            fresh.append(float(moved.trace_psf(det1, world_unit_um=1000.0, pixels=8).strehl[0]))
        print(json.dumps({"what": "gap", "rays": rays, "focus": focus.tolist(), "strehl_scan": scan.strehl[0].tolist(),
                          "strehl_retrace": fresh}), flush=True)


if __name__ == "__main__":
    main()
