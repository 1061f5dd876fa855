#!/usr/bin/env python3
"""Optical path and wavefront of the frame on the device (DeviceFrame.optical_path / wavefront,
RayTracer.trace_wavefront), timed with device events after warm-up, on BASELINE config 2 at 1M rays (3 generations,
about 3M rows).

  optical_path   prt_frame_optical_path: one launch per generation (and one status word read back)
  wavefront      DeviceFrame.wavefront(detector, zernike=15): the optical path, the wavefront passes, the per-group
                 records brought back and solved on the host
  loop           trace_wavefront(detector) end to end, against trace() -> pandas groupby('id') cumulative OPL (the host
                 path: the frame across PCIe, then pandas)

Prints one JSON line per figure.  usage: tools/wavefront_bench.py [--rays N] [--steps K] [--host-steps K]
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
import pandas as pd  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402


def device_ms(fn, steps, warmup=3):
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


def host_opl(tracer):
    frame = tracer.trace()
    d = [frame[b].to_numpy() - frame[a].to_numpy() for a, b in (("x0", "x1"), ("y0", "y1"), ("z0", "z1"))]
    segment = pd.Series(frame["index"].to_numpy() * np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    return segment.groupby(frame["id"].to_numpy()).cumsum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--host-steps", type=int, default=3)
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation)}
    print(json.dumps({**common, "what": "optical_path", "ms": device_ms(frame.optical_path, args.steps)}), flush=True)
    for terms in (15, 36):
        ms = device_ms(lambda: frame.wavefront(det, zernike=terms), args.steps)
        print(json.dumps({**common, "what": f"wavefront_J{terms}", "ms": ms}), flush=True)
    trace_only = wall_ms(tracer.trace_device, args.steps)
    loop = wall_ms(lambda: tracer.trace_wavefront(det), args.steps)
    host = wall_ms(lambda: host_opl(tracer), args.host_steps)
    print(json.dumps({**common, "what": "loop", "trace_device_ms": trace_only, "trace_wavefront_ms": loop,
                      "trace_to_pandas_groupby_ms": host}), flush=True)


if __name__ == "__main__":
    main()
