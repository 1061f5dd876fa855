#!/usr/bin/env python3
"""Shape and index sensitivities of the frame on the device (DeviceFrame.sensitivity with Deformation / IndexChange, the
entry point prt_frame_design_sensitivity), timed after warm-up on BASELINE config 2 at --rays rays (3 generations, two
refractions a ray), for K = 1, 6 and 16 parameters (--K to choose), in the manner of tools/sensitivity_bench.py:

  design        DeviceFrame.sensitivity() end to end with a mix of radii, thickness, stretches, index and motions
  motion        the same call with K Motions: the rigid pass (prt_frame_sensitivity), on the same box and frame
  differences   what central differences cost for the same gradient: 2 K times (apply the parameter, trace -- which takes
                the scene update --, apply it back); measured on the first shape parameter, not multiplied out from a
                plain trace
  trace         one RayTracer.trace_device() of the unchanged system, for scale

One clock for all: the host's, around calls that end in a synchronise.  A window is as many calls as fill --window-ms
(default 300 ms); each figure is the median of --repeats windows, with the smallest and largest beside it.  Prints one
JSON line per figure.
usage: tools/design_sensitivity_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 1 6 16]"""
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
from sensitivity_bench import motions_of, windows  # noqa: E402


def design_of(lens, det, K):
    front, back, stock = (surface for _, surface in lens.surface_ids)
    D, shear = pyrayt.Deformation, [[0.1, 0.4, 0.0], [-0.3, 0.2, 0.5], [0.0, 0.1, -0.2]]
    every = [D.radius(front, keep=(-0.125, 0, 0)), D.radius(back, keep=(0.125, 0, 0)), D(back, translate=(1, 0, 0)),
             pyrayt.IndexChange(lens), pyrayt.Motion(lens, translate=(0, 1, 0)), pyrayt.Motion(det, translate=(1, 0, 0)),
             D.radius(front), D.radius(back), D.stretch(lens, (1, 0, 0)), D.stretch(lens, (0, 1, 0)), D(lens, linear=shear),
             pyrayt.IndexChange(lens, rate=0.5), pyrayt.Motion(lens, rotate=(0, 0, 1)), D.stretch(det, (0, 1, 0)),
             D(det, rotate=(0, 0.5, 0), linear=shear), pyrayt.Motion(lens, translate=(1, 0, 0))]
    return every[:K]


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
    radius = design_of(lens, det, 1)[0]
    h = 2.0 ** -12

    def two_traces():  # (one parameter's central difference: the scene changes, so each trace takes a scene update)
        radius.apply(h)
        tracer.trace_device()
        radius.apply(-2 * h * 2 / (2 + h))  # ((R + h) scaled back to R - h: the amount is in the own frame's units)
        tracer.trace_device()
        radius.apply(h * 2 / (2 - h))

    pair = windows(two_traces, args.repeats, args.window_ms)
    print(json.dumps({**common, "what": "differences", "K": 1, **pair}), flush=True)
    for K in args.K:
        design, motions = design_of(lens, det, K), motions_of(lens, det, K)
        got = frame.sensitivity(det, design, [lens, det])
        took = windows(lambda: frame.sensitivity(det, design, [lens, det]), args.repeats, args.window_ms)
        rigid = windows(lambda: frame.sensitivity(det, motions, [lens, det]), args.repeats, args.window_ms)
        print(json.dumps({**common, "what": "motion", "K": K, **rigid}), flush=True)
        print(json.dumps({**common, "what": "design", "K": K, **took, "motion_ms": rigid["ms"],
                          "design_over_motion": took["ms"] / rigid["ms"], "differences_ms": K * pair["ms"],
                          "differences_over_design": K * pair["ms"] / took["ms"], "n_unknown": got.n_unknown,
                          "n_invalid": got.n_invalid, "n_unfit": got.n_unfit,
                          "rms_radius_gradient": got.rms_radius_gradient[0].tolist()[:4]}), flush=True)


if __name__ == "__main__":
    main()
