#!/usr/bin/env python3
"""Launch and wavelength sensitivities of the frame on the device (DeviceFrame.sensitivity with SourceMotion and
WavelengthChange, the entry point prt_frame_launch_sensitivity), timed after warm-up on config 2's lens in BK7 at --rays rays
(3 generations, two refractions a ray), for K = 1, 6 and 16 parameters (--K to choose), in the manner of
tools/opd_sensitivity_bench.py:

  launch        DeviceFrame.sensitivity with K launch parameters (translations and rotations of the launch, wavelength
                changes, one source's rays), end to end: the new call without the wavefront
  launch_opd    the same with wavefront=w, w a Wavefront computed before (J = 15)
  design        K rigid Deformations (S = 0: the design form's code path, prt_frame_design_sensitivity) on the same frame
  opd           the same with wavefront=w: prt_frame_opd_sensitivity
  differences   what central differences cost for the same derivatives: 2 K re-traces of the frame (a moved source or a
                shifted wavelength changes no scene, so a re-trace is a plain trace_device); measured once, times K

By bytes the new forms move the design / opd forms' state plus 24 K bytes per selected row of slopes, so they should cost
the same per parameter within that share; the figures say whether they do.  One clock for all: the host's, around calls
that end in a synchronise.  A window is as many calls as fill --window-ms (default 300 ms); each figure is the median of
--repeats windows, with the smallest and largest beside it.  Prints one JSON line per figure.
usage: tools/launch_sensitivity_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 1 6 16]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyrayt_amd as pyrayt  # noqa: E402
from sensitivity_bench import windows  # noqa: E402


def launch_of(K, rays):
    S, W, e = pyrayt.SourceMotion, pyrayt.WavelengthChange, np.eye(3)
    six = [S(None, translate=tuple(e[1])), S(None, translate=tuple(e[2])), S(None, rotate=tuple(e[2]), pivot=(-1.9, 0, 0)),
           S(None, rotate=tuple(-e[1]), pivot=(-1.9, 0, 0)), W(), S.of_source(0, rays, translate=tuple(e[0]))]
    every = six + [S((0, rays // 2), rotate=tuple(e[0])), W((rays // 2, rays - rays // 2), rate=-1.0),
                   S(None, translate=(0.3, -0.2, 0.5), rotate=(0.1, 0.2, 0.3), pivot=(1, 0, 0)), W((0, rays // 3))] + six
    return every[:K] if K > 1 else every[2:3]


def rigid_of(lens, det, K):
    e = np.eye(3)
    every = [pyrayt.Deformation(part, **{kind: tuple(e[k])}) for part in (lens, det) for kind in ("translate", "rotate")
             for k in range(3)]
    return (every + every)[:K]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 6, 16])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1, material=pyrayt.materials.glass["BK7"])
    src = pyrayt.components.ConeOfRays(cone_angle=6, wavelength=0.55).move_x(-1.9)
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation), "window_ms": args.window_ms, "repeats": args.repeats}
    wave = frame.wavefront(det, weights="intensity")
    pair = windows(lambda: (tracer.trace_device(), tracer.trace_device(), torch.cuda.synchronize()), args.repeats, args.window_ms)
    print(json.dumps({**common, "what": "differences", "K": 1, **pair}), flush=True)
    for K in args.K:
        launch, rigid = launch_of(K, args.rays), rigid_of(lens, det, K)
        for name, wavefront, old_name in (("launch", None, "design"), ("launch_opd", wave, "opd")):
            old = windows(lambda: frame.sensitivity(det, rigid, [lens, det], wavefront=wavefront), args.repeats, args.window_ms)
            print(json.dumps({**common, "what": old_name, "K": K, **old}), flush=True)
            got = frame.sensitivity(det, launch, [lens, det], wavefront=wavefront)
            new = windows(lambda: frame.sensitivity(det, launch, [lens, det], wavefront=wavefront), args.repeats, args.window_ms)
            print(json.dumps({**common, "what": name, "K": K, **new, f"{old_name}_ms": old["ms"],
                              f"{name}_over_{old_name}": new["ms"] / old["ms"], "differences_ms": K * pair["ms"],
                              f"differences_over_{name}": K * pair["ms"] / new["ms"], "n_unfit": got.n_unfit,
                              "n_invalid": got.n_invalid, "focus_gradient": got.focus_gradient()[0].tolist()[:4]}), flush=True)


if __name__ == "__main__":
    main()
