#!/usr/bin/env python3
"""MTF sensitivities of the frame on the device (Sensitivity.mtf_gradient, the entry point prt_frame_mtf_gradient), timed
after warm-up on config 2's lens at --rays rays (3 generations), for K = 1, 6 and 16 parameters (--K to choose), at 256
outputs (2 azimuths x 128 frequencies, one plane) and on a 41-plane scan (41 x 2 x 16 outputs), in the manner of
tools/launch_sensitivity_bench.py:

  sensitivity   DeviceFrame.sensitivity(..., slopes=True) with K design parameters: what mtf_gradient needs first
  mtf_gradient  Sensitivity.mtf_gradient on that result, end to end (the five passes and the read-back of otf and dotf)
  mtf           DeviceFrame.mtf at the same outputs: the evaluate-only pass whose sum kernel k_mtfg_sum extends
  retrace       one trace_device() of the same rays: what a central difference pays twice a parameter, beside 2 mtf()
  differences   2 K x (retrace + mtf), from the two figures above: the cost of the same derivatives by central
                differences (a system changed between traces also recompiles its scene, which is not counted)

One clock for all: the host's, around calls that end in a synchronise.  A window is as many calls as fill --window-ms
(default 300 ms); each figure is the median of --repeats windows, with the smallest and largest beside it.  Prints one
JSON line per figure.  --once runs every call once after a warm-up, for a kernel trace (rocprofv3 --kernel-trace --stats
-- python tools/mtf_gradient_bench.py --once) that sets k_mtfg_sum beside k_mtf_sum on the same rays.
usage: tools/mtf_gradient_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 1 6 16] [--once]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pyrayt_amd as pyrayt  # noqa: E402
from sensitivity_bench import windows  # noqa: E402

OUTPUTS = {"256 outputs": dict(frequencies=np.linspace(0.0, 100.0, 128), azimuths=(0.0, 90.0), focus=(0.0,)),
           "41 planes": dict(frequencies=np.linspace(0.0, 100.0, 16), azimuths=(0.0, 90.0), focus=np.linspace(-0.1, 0.1, 41))}


def parameters_of(lens, det, K):
    """K design parameters on the singlet: radii, the thickness, the index, motions of the lens and the detector."""
    D, M, e = pyrayt.Deformation, pyrayt.Motion, np.eye(3)
    front, back = lens.surface_ids[0][1], lens.surface_ids[1][1]
    six = [D.radius(front, keep=(-0.125, 0, 0)), D.radius(back, keep=(0.125, 0, 0)), D(back, translate=(1, 0, 0)),
           pyrayt.IndexChange(lens), M(lens, translate=(0, 1, 0)), M(lens, rotate=(0, 0, 1))]
    every = six + [M(lens, translate=tuple(e[k])) for k in (0, 2)] + [M(lens, rotate=tuple(e[k])) for k in (0, 1)]
    every += [M(det, translate=tuple(e[k])) for k in range(3)] + [M(det, rotate=tuple(e[k])) for k in range(3)]
    return every[:K]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--K", type=int, nargs="+", default=[1, 6, 16])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    pyrayt.g3d.objects.CountedObject.reset_ids()
    lens = pyrayt.components.biconvex_lens(2, 2, 0.25, aperture=1)
    src = pyrayt.components.ConeOfRays(cone_angle=6).move_x(-1.9)
    det = pyrayt.components.baffle((1, 1)).move_x(1)
    tracer = pyrayt.RayTracer(src, [lens, det], rays_per_source=args.rays)
    frame = tracer.trace_device()
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation), "window_ms": args.window_ms, "repeats": args.repeats}

    def timed(fn):
        if args.once:
            fn()
            fn()
            torch.cuda.synchronize()
            return {"ms": float("nan")}
        return windows(fn, args.repeats, args.window_ms)

    retrace = timed(lambda: (tracer.trace_device(), torch.cuda.synchronize()))
    print(json.dumps({**common, "what": "retrace", **retrace}), flush=True)
    plain = {}
    for name, options in OUTPUTS.items():
        plain[name] = timed(lambda: frame.mtf(det, **options))
        print(json.dumps({**common, "what": "mtf", "outputs": name, **plain[name]}), flush=True)
    for K in args.K:
        parameters = parameters_of(lens, det, K)
        first = timed(lambda: frame.sensitivity(det, parameters, [lens, det], slopes=True))
        print(json.dumps({**common, "what": "sensitivity", "K": K, **first}), flush=True)
        sens = frame.sensitivity(det, parameters, [lens, det], slopes=True)
        for name, options in OUTPUTS.items():
            got = sens.mtf_gradient(**options)
            new = timed(lambda: sens.mtf_gradient(**options))
            differences = 2 * K * (retrace["ms"] + plain[name]["ms"])
            print(json.dumps({**common, "what": "mtf_gradient", "K": K, "outputs": name, **new,
                              "with_sensitivity_ms": new["ms"] + first["ms"], "mtf_ms": plain[name]["ms"],
                              "mtf_gradient_over_mtf": new["ms"] / plain[name]["ms"], "differences_ms": differences,
                              "differences_over_one_pass": differences / (new["ms"] + first["ms"]),
                              "n_rays": int(got.n_rays[0]), "n_unfollowed": int(got.n_unfollowed[0]),
                              "dmtf_at_the_last_frequency": got.dmtf[0, :, 0, 0, -1].tolist()[:4]}), flush=True)


if __name__ == "__main__":
    main()
