#!/usr/bin/env python3
"""Ray-aberration curves of the frame on the device (DeviceFrame.launch_index / ray_aberrations,
RayTracer.trace_ray_aberrations), timed with device events after warm-up, on BASELINE config 2 (3 generations; the
detector holds one row per ray; a point source, so the pupil coordinate is the launch direction).

  join          DeviceFrame.launch_index(): the per-id table and the gather over every row
  aberrations   DeviceFrame.ray_aberrations(detector, pupil="direction"): the join, the pass (21 terms, 64 zones) and the
                host-side solve
  loop          trace_ray_aberrations(detector) in a loop that moves the detector before every trace (wall time per
                iteration), against trace_device() alone in the same loop
  pandas        the same trace followed by to_pandas() and the notebook's join (cell 12: isin on the ids, the axis
                intercept and the launch heights) on the host (one core): one iteration, wall time

Prints one JSON line per figure.  usage: tools/ray_aberration_bench.py [--rays N] [--steps K] [--no-pandas]
(run under rocprofv3 --kernel-trace --stats for per-kernel times)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402


def device_ms(fn, steps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps


def wall_ms(fn, steps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / steps


def notebook_join(results):
    """examples/lens_design.ipynb cell 12, as written there."""
    imager_rays = results.loc[results["generation"] == np.max(results["generation"])]
    intercept = -imager_rays["x_tilt"] * imager_rays["y0"] / imager_rays["y_tilt"] + imager_rays["x0"]
    radii = results.loc[np.logical_and(results["generation"] == 0, results["id"].isin(imager_rays["id"]))]["y0"]
    return radii, intercept


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-pandas", action="store_true")
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame)}
    ms = device_ms(frame.launch_index, args.steps)
    print(json.dumps({**common, "what": "join", "ms": ms}), flush=True)
    got = frame.ray_aberrations(det, pupil="direction")
    ms = device_ms(lambda: frame.ray_aberrations(det, pupil="direction"), args.steps)
    print(json.dumps({**common, "what": "aberrations", "terms": 21, "zones": 64, "rays_used": int(got.n_rays.sum()),
                      "ms": ms}), flush=True)
    step = [1e-3]

    def move():  # (the detector steps back and forth by 1 um)
        det.move_x(step[0])
        step[0] = -step[0]

    trace_only = wall_ms(lambda: (move(), tracer.trace_device()), args.steps)
    loop = wall_ms(lambda: (move(), tracer.trace_ray_aberrations(det, pupil="direction")), args.steps)
    print(json.dumps({**common, "what": "loop", "trace_device_ms": trace_only, "trace_ray_aberrations_ms": loop}),
          flush=True)
    if not args.no_pandas:
        t = time.perf_counter()
        results = tracer.trace()
        traced = time.perf_counter()
        notebook_join(results)
        done = time.perf_counter()
        print(json.dumps({**common, "what": "pandas", "trace_to_pandas_ms": (traced - t) * 1e3,
                          "notebook_join_ms": (done - traced) * 1e3}), flush=True)


if __name__ == "__main__":
    main()
