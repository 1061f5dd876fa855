#!/usr/bin/env python3
"""Ghost rays of the frame on the device (DeviceFrame.ghosts, RayTracer.trace_ghosts), timed with device events after
warm-up, on BASELINE config 2 inside a housing at --rays rays (3 generations, two refractions a ray):

  fresnel        the yardstick, in the same session: DeviceFrame.fresnel() on the same frame
  ghosts         DeviceFrame.ghosts() end to end: prt_frame_ghosts_count (marking, the sort's count and scans, the
                 read-back), the allocation of the ray set, prt_frame_ghosts_emit; `ratio` = ghosts / fresnel
  trace          the signal trace alone (RayTracer.trace_device)
  trace_ghosts   RayTracer.trace_ghosts(order=2): the signal trace, three Fresnel passes, two spawns, two traces of
                 the children; `ratio` = trace_ghosts / trace

Prints one JSON line per figure and, with --out, appends them to that file.
usage: tools/ghost_bench.py [--rays N] [--steps K] [--out profiles/ghosts/ghost_bench.jsonl]
(run under rocprofv3 --kernel-trace --stats for per-kernel times: k_ghost_mark against k_fresnel_step)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from mtf_bench import device_ms  # noqa: E402
from pyrayt_amd import ghosts  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det, ghosts.housing(30.0)], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation)}
    lines = []

    def report(**line):
        lines.append({**common, **line})
        print(json.dumps(lines[-1]), flush=True)

    fresnel = frame.fresnel()
    glass = ghosts.refracting_surfaces(tracer)
    spawn = dict(rays_per_source=args.rays, n_groups=1)
    children = frame.ghosts(fresnel, glass, **spawn)
    fresnel_ms = device_ms(lambda: frame.fresnel(), args.steps)
    report(what="fresnel", ms=fresnel_ms)
    ghosts_ms = device_ms(lambda: frame.ghosts(fresnel, glass, **spawn), args.steps)
    report(what="ghosts", ms=ghosts_ms, ratio=ghosts_ms / fresnel_ms, children=len(children), groups=children.n_groups,
           n_open=children.n_open)
    trace_ms = device_ms(lambda: tracer.trace_device(), args.steps)
    report(what="trace", ms=trace_ms)
    analysis = tracer.trace_ghosts(det, order=2)
    table = analysis.table()
    all_ms = device_ms(lambda: tracer.trace_ghosts(det, order=2), max(2, args.steps // 2))
    report(what="trace_ghosts", ms=all_ms, ratio=all_ms / trace_ms, order=2, paths=len(table),
           worst_share=float(table["share"].iloc[0]) if len(table) else None)
    if args.out:
        with open(args.out, "a") as out:
            for line in lines:
                out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
