#!/usr/bin/env python3
"""Scattered rays of the frame on the device (DeviceFrame.scatter, RayTracer.trace_scatter), timed with device events
after warm-up, on BASELINE config 2 inside a housing at --rays rays (3 generations; both lens faces listed, a Harvey
table on them):

  ghosts, fresnel  the yardsticks, in the same session: DeviceFrame.ghosts() and DeviceFrame.fresnel() on the same frame
  scatter          DeviceFrame.scatter() end to end for N = 1, 4, 16 children a hit in both modes (hemisphere, disk):
                   prt_frame_scatter_count (the uploads, the marking, the sort's count and scans, the read-back), the
                   allocation of the ray set, prt_frame_scatter_emit; `ratio` = scatter / ghosts
  trace            the signal trace alone (RayTracer.trace_device)
  trace_scatter    RayTracer.trace_scatter(N = 1, hemisphere): the signal trace, the spawn, the trace of the
                   children; `ratio` = trace_scatter / trace

Prints one JSON line per figure and, with --out, appends them to that file.
usage: tools/scatter_bench.py [--rays N] [--steps K] [--out profiles/scatter/scatter_bench.jsonl]
(run under rocprofv3 --kernel-trace --stats for per-kernel times: k_scatter_mark and k_scatter_emit against k_ghost_mark
and k_ghost_emit)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from mtf_bench import device_ms  # noqa: E402
from pyrayt_amd import ghosts  # noqa: E402
from pyrayt_amd.scatter import Scatter, Target  # noqa: E402


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
    met = [s for s in glass if bool((frame["surface"] == s).any())]  # (both lens faces; the edge is not met)
    spawn = dict(rays_per_source=args.rays, n_groups=1)
    fresnel_ms = device_ms(lambda: frame.fresnel(), args.steps)
    report(what="fresnel", ms=fresnel_ms)
    children = frame.ghosts(fresnel, glass, **spawn)
    ghosts_ms = device_ms(lambda: frame.ghosts(fresnel, glass, **spawn), args.steps)
    report(what="ghosts", ms=ghosts_ms, children=len(children))
    polish = {tuple(met): Scatter.harvey(0.8, 0.02, -1.8)}
    modes = (("hemisphere", None), ("disk", Target.disk((-1.5, 0.0, 0.0), (1.0, 0.0, 0.0), 0.75)))  # (on the side the light comes from: the scatter is reflective)
    for mode, toward in modes:
        for n in (1, 4, 16):
            call = dict(toward=toward, rays_per_hit=n, seed=1, **spawn)
            rays = frame.scatter(polish, tracer, **call)
            steps = max(2, args.steps // (1 if n < 16 else 2))
            ms = device_ms(lambda: frame.scatter(polish, tracer, **call), steps)
            report(what="scatter", mode=mode, rays_per_hit=n, ms=ms, ratio=ms / ghosts_ms, items=2 * args.rays * n,
                   children=len(rays), rejected=rays.n_rejected, below=rays.n_below)
            del rays
    trace_ms = device_ms(lambda: tracer.trace_device(), args.steps)
    report(what="trace", ms=trace_ms)
    run = dict(toward=None, rays_per_hit=1, seed=1)
    analysis = tracer.trace_scatter(det, polish, **run)
    all_ms = device_ms(lambda: tracer.trace_scatter(det, polish, **run), max(2, args.steps // 2))
    report(what="trace_scatter", ms=all_ms, ratio=all_ms / trace_ms, mode="hemisphere", rays_per_hit=1,
           children=len(analysis.rays), total_share=analysis.total_share())
    if args.out:
        with open(args.out, "a") as out:
            for line in lines:
                out.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
