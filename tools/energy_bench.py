#!/usr/bin/env python3
"""Geometric enclosed energy of the frame on the device (DeviceFrame.enclosed_energy,
RayTracer.trace_enclosed_energy), timed with device events after warm-up, on BASELINE config 2 (3 generations; the
detector holds one row per ray).

  a             DeviceFrame.enclosed_energy(detector): 1 plane x 3 fractions x 64 radii
  b             DeviceFrame.enclosed_energy(detector): 41 planes x 3 fractions x 64 radii (a through-focus scan)
  mtf           the yardstick: DeviceFrame.mtf(detector), 41 planes x 2 azimuths x 64 frequencies
  loop          case a by trace_enclosed_energy(detector) in a loop that moves the detector before every trace (wall
                time per iteration), against trace_device() alone in the same loop
  numpy         the host path for cases a and b: copy the detector's columns, then per plane a sort of the distances
                and a cumulative sum of the weights (wall time, one core; the trace is not in it)

Prints one JSON line per figure.  usage: tools/energy_bench.py [--rays N] [--steps K] [--no-numpy]
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
from mtf_bench import device_ms, wall_ms  # noqa: E402


def numpy_energy(frame, surface, radii, fractions, focus):
    """The host path: the detector's columns brought over, then per plane a sort and a cumulative sum (default axes,
    centroid reference, intensity weights, distances about each plane's centroid)."""
    cut = frame.where(surface=surface)
    q = np.stack([cut[name].cpu().numpy() for name in ("x1", "y1", "z1")], 1)
    u = np.stack([cut[name].cpu().numpy() for name in ("x_tilt", "y_tilt", "z_tilt")], 1)
    w = cut["intensity"].cpu().numpy()
    c = np.average(q, axis=0, weights=w)
    s = u[:, 1:] / u[:, :1]
    p = (q[:, 1:] - c[1:]) - s * (q[:, :1] - c[0])
    pbar, sbar = np.average(p, axis=0, weights=w), np.average(s, axis=0, weights=w)
    out = []
    for delta in focus:
        x = p + delta * s - (pbar + delta * sbar)
        d = np.hypot(x[:, 0], x[:, 1])
        order = np.argsort(d, kind="stable")
        d, run = d[order], np.cumsum(w[order])
        inside = np.searchsorted(d, radii, side="right")
        out.append((np.concatenate([[0.0], run])[inside] / run[-1], d[np.searchsorted(run, fractions * run[-1])]))
    return out


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
    fractions = np.array([0.5, 0.8, 0.9])
    first = frame.enclosed_energy(det, None, fractions=(1.0,))
    radii = np.linspace(0.0, float(first.radius.max()), 65)[1:]
    cases = {"a": (0.0,), "b": np.linspace(-0.2, 0.2, 41)}
    for name, focus in cases.items():
        got = frame.enclosed_energy(det, radii, fractions=fractions, focus=focus)
        ms = device_ms(lambda: frame.enclosed_energy(det, radii, fractions=fractions, focus=focus), args.steps)
        curve = device_ms(lambda: frame.enclosed_energy(det, radii, fractions=None, focus=focus), args.steps)
        select = device_ms(lambda: frame.enclosed_energy(det, None, fractions=fractions, focus=focus), args.steps)
        print(json.dumps({**common, "what": name, "planes": len(focus), "fractions": 3, "radii": len(radii), "ms": ms,
                          "radii_only_ms": curve, "fractions_only_ms": select, "rays_used": int(got.n_rays.sum()),
                          "radius_at_first_plane": got.radius[0, 0].tolist()}), flush=True)
    nu = np.linspace(0.0, 63.0, 64)
    ms = device_ms(lambda: frame.mtf(det, nu, focus=cases["b"]), args.steps)
    print(json.dumps({**common, "what": "mtf", "planes": 41, "azimuths": 2, "frequencies": 64, "ms": ms}), flush=True)
    step = [1e-3]

    def move():  # (the detector steps back and forth by 1 um)
        det.move_x(step[0])
        step[0] = -step[0]

    trace_only = wall_ms(lambda: (move(), tracer.trace_device()), args.steps)
    loop = wall_ms(lambda: (move(), tracer.trace_enclosed_energy(det, radii, fractions=fractions)), args.steps)
    print(json.dumps({**common, "what": "loop", "trace_device_ms": trace_only, "trace_enclosed_energy_ms": loop}),
          flush=True)
    if not args.no_numpy:
        frame = tracer.trace_device()
        for name, focus in cases.items():
            t = time.perf_counter()
            numpy_energy(frame, det.get_id(), radii, fractions, focus)
            print(json.dumps({**common, "what": "numpy_" + name, "planes": len(focus),
                              "copy_sort_cumsum_ms": (time.perf_counter() - t) * 1e3}), flush=True)


if __name__ == "__main__":
    main()
