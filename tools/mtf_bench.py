#!/usr/bin/env python3
"""Geometric MTF of the frame on the device (DeviceFrame.mtf, RayTracer.trace_mtf), timed with device events after
warm-up, on BASELINE config 2 (3 generations; the detector holds one row per ray).

  a             DeviceFrame.mtf(detector): 1 plane x 2 azimuths x 128 frequencies
  b             DeviceFrame.mtf(detector): 41 planes x 2 azimuths x 64 frequencies (a through-focus scan)
                each with its rate in ray-output terms per second (rays summed x outputs / time) of the whole call
  loop          case a by trace_mtf(detector) in a loop that moves the detector before every trace (wall time per
                iteration), against trace_device() alone in the same loop
  numpy         trace() to a DataFrame plus the definition restated in numpy on the host (one core) for case a: one
                iteration, wall time

Prints one JSON line per figure.  usage: tools/mtf_bench.py [--rays N] [--steps K] [--no-numpy]
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


def numpy_mtf(rows, nu, azimuths, chunk=65536):
    """The definition on the host: default axes, centroid reference, intensity weights, one plane at delta = 0."""
    q, u, w = rows[["x1", "y1", "z1"]].to_numpy(), rows[["x_tilt", "y_tilt", "z_tilt"]].to_numpy(), rows["intensity"].to_numpy()
    c = np.average(q, axis=0, weights=w)
    s = u[:, 1:] / u[:, :1]
    p = (q[:, 1:] - c[1:]) - s * (q[:, :1] - c[0])
    theta = np.radians(azimuths)
    k = np.stack([np.cos(theta)[:, None] * nu, np.sin(theta)[:, None] * nu], -1).reshape(-1, 2)
    total = np.zeros(len(k), dtype=complex)
    for at in range(0, len(p), chunk):
        total += (w[at:at + chunk] * np.exp(-2j * np.pi * (p[at:at + chunk] @ k.T).T)).sum(-1)
    return total / w.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame)}
    cases = {"a": (np.linspace(0.0, 127.0, 128), (0.0,)), "b": (np.linspace(0.0, 63.0, 64), np.linspace(-0.2, 0.2, 41))}
    for name, (nu, focus) in cases.items():
        got = frame.mtf(det, nu, focus=focus)
        ms = device_ms(lambda: frame.mtf(det, nu, focus=focus), args.steps)
        terms = float(got.n_rays.sum()) * got.otf[0].size
        print(json.dumps({**common, "what": name, "planes": len(focus), "azimuths": 2, "frequencies": len(nu),
                          "ms": ms, "terms": terms, "terms_per_s_whole_call": terms / (ms * 1e-3)}), flush=True)
    nu = cases["a"][0]
    step = [1e-3]

    def move():  # (the detector steps back and forth by 1 um)
        det.move_x(step[0])
        step[0] = -step[0]

    trace_only = wall_ms(lambda: (move(), tracer.trace_device()), args.steps)
    loop = wall_ms(lambda: (move(), tracer.trace_mtf(det, nu)), args.steps)
    print(json.dumps({**common, "what": "loop", "trace_device_ms": trace_only, "trace_mtf_ms": loop}), flush=True)
    if not args.no_numpy:
        t = time.perf_counter()
        rows = tracer.trace()
        rows = rows.loc[rows["surface"] == det.get_id()]
        numpy_mtf(rows, nu, np.array([0.0, 90.0]))
        print(json.dumps({**common, "what": "numpy", "trace_and_numpy_ms": (time.perf_counter() - t) * 1e3}),
              flush=True)


if __name__ == "__main__":
    main()
