#!/usr/bin/env python3
"""Sensitivities of the frame on the device (DeviceFrame.sensitivity), timed after warm-up on BASELINE config 2 at --rays
rays (3 generations, two refractions a ray), for K = 1, 6 and 16 parameters (--K to choose):

  sensitivity   DeviceFrame.sensitivity() end to end: the selection (torch), the launches, the sums, the read-back of the
                status word and the counters
  trace         the yardstick: one RayTracer.trace_device() of the same system (prt_trace).  Central differences cost
                2 K of them for K parameters, and this pass does not touch the trace
  optical_path  the other per-generation pass over a dense per-id state, for scale

One clock for all three: the host's, around calls that end in a synchronise (the trace runs on the scene's own streams,
where events on the current stream see nothing).  A window is as many calls as fill --window-ms (default 300 ms); each
figure is the median of --repeats windows, with the smallest and largest beside it.  Prints one JSON line per figure.
For the kernels' own times run it under `rocprofv3 --kernel-trace --stats --output-format csv`, in a run of its own, with
--K 1 --repeats 1 --window-ms 20: the kernel trace then holds one parameter count.
usage: tools/sensitivity_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 1 6 16]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from mtf_bench import wall_ms  # noqa: E402


def windows(fn, repeats, window_ms):
    fn()
    once = wall_ms(fn, 3, warmup=1)
    steps = max(3, int(np.ceil(window_ms / max(once, 1e-3))))
    times = sorted(wall_ms(fn, steps, warmup=1) for _ in range(repeats))
    return {"ms": times[len(times) // 2], "ms_min": times[0], "ms_max": times[-1], "steps": steps}


def motions_of(lens, det, K):
    e = np.eye(3)
    every = [pyrayt.Motion(lens, translate=tuple(e[k])) for k in range(3)]
    every += [pyrayt.Motion(lens, rotate=tuple(e[k])) for k in range(3)]
    every += [pyrayt.Motion(det, translate=tuple(e[k])) for k in range(3)]
    every += [pyrayt.Motion(det, rotate=tuple(e[k])) for k in range(3)]
    every += [pyrayt.Motion(lens, translate=tuple(e[k]), rotate=tuple(e[(k + 1) % 3])) for k in range(3)]
    every += [pyrayt.Motion(lens.surface_ids[0][0], translate=(0, 1, 0))]
    return every[:K] if K > 1 else every[4:5]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 6, 16])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-scenes.lensmakers_equation(2, -2, 1.5, 0.25))
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation), "window_ms": args.window_ms, "repeats": args.repeats}
    trace = windows(lambda: tracer.trace_device(), args.repeats, args.window_ms)
    print(json.dumps({**common, "what": "trace", **trace}), flush=True)
    print(json.dumps({**common, "what": "optical_path", **windows(lambda: frame.optical_path(), args.repeats, args.window_ms)}),
          flush=True)
    for K in args.K:
        motions = motions_of(lens, det, K)
        got = frame.sensitivity(det, motions, [lens, det])
        took = windows(lambda: frame.sensitivity(det, motions, [lens, det]), args.repeats, args.window_ms)
        print(json.dumps({**common, "what": "sensitivity", "K": K, **took, "central_differences_ms": 2 * K * trace["ms"],
                          "ratio": 2 * K * trace["ms"] / took["ms"], "n_unknown": got.n_unknown,
                          "n_invalid": got.n_invalid, "n_unfit": got.n_unfit,
                          "rms_radius_gradient": got.rms_radius_gradient[0].tolist()[:3]}), flush=True)


if __name__ == "__main__":
    main()
