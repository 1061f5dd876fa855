#!/usr/bin/env python3
"""Monte Carlo tolerancing of the enclosed energy on the device (Sensitivity.energy_tolerance, the entry point
prt_frame_energy_tolerance), timed after warm-up on config 2's lens at --rays rays (3 generations), for K = 6 parameters
(--K to choose), M = 33, 1 000 and 10 000 trials (--trials to choose) and two samplings (--samplings): "fractions", 3
fractions x 1 plane (the select alone), and "radii", 8 radii x 3 planes (the curve alone), in the manner of
tools/mtf_tolerance_bench.py:

  sensitivity       DeviceFrame.sensitivity(..., slopes=True) with K design parameters: what energy_tolerance needs first
  energy_tolerance  Sensitivity.energy_tolerance on that result with the "focus" compensator, end to end (the staging, the
                    integer weights, the moments, the focus, the curve or the select, the folds and the read-back)
  retrace           the lens moved by a Motion on the host, then one trace_device() of the same rays and one
                    enclosed_energy() of the same sampling: what the route without this pass pays per perturbed system
                    (existing code: the same at the parent commit)
  retraces          M x retrace, from the figure above
  mtf_tolerance     Sensitivity.mtf_tolerance with 8 outputs on the same trials: the yardstick of the kernel form

One clock for all: the host's, around calls that end in a synchronise.  A window is as many calls as fill --window-ms;
each figure is the median of --repeats windows.  Prints one JSON line per figure and appends it to --out (default
profiles/energy_tolerance/energy_tolerance_bench.jsonl).  --once runs every call once after a warm-up, for a kernel trace
in a run of its own (rocprofv3 --kernel-trace --stats -- python tools/energy_tolerance_bench.py --once).
usage: tools/energy_tolerance_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 6] [--trials 33 1000 10000]
                                       [--samplings fractions radii] [--out FILE] [--once]"""
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
from mtf_gradient_bench import parameters_of  # noqa: E402
from sensitivity_bench import windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--K", type=int, nargs="+", default=[6])
    ap.add_argument("--trials", type=int, nargs="+", default=[33, 1000, 10000])
    ap.add_argument("--samplings", nargs="+", default=["fractions", "radii"], choices=["fractions", "radii"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_tolerance", "energy_tolerance_bench.jsonl"))
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
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def emit(line):
        text = json.dumps({**common, **line})
        print(text, flush=True)
        if not args.once:
            with open(args.out, "a") as out:
                out.write(text + "\n")

    def timed(fn):
        if args.once:
            fn()
            fn()
            torch.cuda.synchronize()
            return {"ms": float("nan")}
        return windows(fn, args.repeats, args.window_ms)

    nominal = frame.enclosed_energy(det, fractions=(0.5, 0.8, 0.9))
    r80 = float(nominal.radius[0, 0, 1])
    samplings = {"fractions": dict(radii=None, fractions=(0.5, 0.8, 0.9), focus=(0.0,)),
                 "radii": dict(radii=np.linspace(0.25, 2.0, 8) * r80, fractions=None, focus=(-0.05, 0.0, 0.05))}
    sign = [1.0]

    def perturbed(options):  # (the lens moved and moved back in turn, so that the system stays where it is)
        lens.move_y(sign[0] * 1e-6)
        sign[0] = -sign[0]
        tracer.trace_device().enclosed_energy(det, options["radii"], fractions=options["fractions"], focus=options["focus"])
        torch.cuda.synchronize()

    retrace = {}
    for name in args.samplings:
        retrace[name] = timed(lambda: perturbed(samplings[name]))
        emit({"what": "retrace", "sampling": name, **retrace[name]})
    for K in args.K:
        parameters = parameters_of(lens, det, K)
        first = timed(lambda: frame.sensitivity(det, parameters, [lens, det], slopes=True))
        emit({"what": "sensitivity", "K": K, **first})
        sens = frame.sensitivity(det, parameters, [lens, det], slopes=True)
        widths = [1e-3] * K
        for M in args.trials:
            trials = pyrayt.Tolerances(widths, "normal", seed=M).sample(M)
            for name in args.samplings:
                options = samplings[name]
                run = lambda: sens.energy_tolerance(trials, options["radii"], fractions=options["fractions"],  # noqa: E731
                                                    focus=options["focus"], compensators=("focus",))
                got = run()
                new = timed(run)
                retraces = M * retrace[name]["ms"]
                emit({"what": "energy_tolerance", "K": K, "sampling": name, "trials": M, **new,
                      "with_sensitivity_ms": new["ms"] + first["ms"], "retraces_ms": retraces,
                      "retraces_over_one_pass": retraces / (new["ms"] + first["ms"]), "n_rays": int(got.n_rays.sum()),
                      "n_unfollowed": int(got.n_unfollowed.sum()), "nominal_r80": r80,
                      "p90_of_the_last_radius": float(got.percentiles(90)[0, 0]) if name == "fractions" else None,
                      "yield_0.8_inside_r80": float(got.yield_(0.8, radius=3)[0]) if name == "radii" else None})
            mtf = timed(lambda: sens.mtf_tolerance(trials, np.linspace(0.0, 3.0, 2), azimuths=(0.0, 90.0), focus=(0.0, 0.05),
                                                   compensators=("focus",)))
            emit({"what": "mtf_tolerance", "K": K, "outputs": 8, "trials": M, **mtf})


if __name__ == "__main__":
    main()
