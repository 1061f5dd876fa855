#!/usr/bin/env python3
"""Monte Carlo tolerancing of the frame on the device (Sensitivity.tolerance, the entry points prt_frame_tolerance and
prt_frame_tolerance_moments), timed after warm-up on config 2's lens at --rays rays (3 generations), for K = 6 and 16
parameters (--K to choose) and M = 33 (a sensitivity table of 16 parameters), 1 000 and 10 000 trials (--trials to
choose), in the manner of tools/psf_gradient_bench.py:

  sensitivity   DeviceFrame.sensitivity(..., wavefront=w) with K design parameters: what tolerance needs first
  tolerance     Sensitivity.tolerance on that result with the "tilt" and "focus" compensators, end to end (the columns,
                the moments, the host's compensator solve, the Strehl pass and the read-back of the outputs)
  wavefront     one trace_wavefront() of the same rays: what the route without this pass pays per perturbed system ...
  psf           ... beside one DeviceFrame.psf of one pixel (its Strehl ratio)
  retraces      M x (wavefront + psf), from the two figures above (a system changed between traces also recompiles its
                scene and moves its parts on the host, which is not counted)

One clock for all: the host's, around calls that end in a synchronise.  A window is as many calls as fill --window-ms
(default 300 ms); each figure is the median of --repeats windows, with the smallest and largest beside it.  Prints one
JSON line per figure; (ray, trial) pairs per second are rays kept x (M + 1) over the call's time (the nominal trial
rides along).  --once runs every call once after a warm-up, for a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/tolerance_bench.py --once) that gives k_tol_sum alone.
usage: tools/tolerance_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 6 16] [--trials 33 1000 10000] [--once]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import pyrayt_amd as pyrayt  # noqa: E402
from mtf_gradient_bench import parameters_of  # noqa: E402
from sensitivity_bench import windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=1_000_000)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--K", type=int, nargs="+", default=[6, 16])
    ap.add_argument("--trials", type=int, nargs="+", default=[33, 1000, 10000])
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

    retrace = timed(lambda: (tracer.trace_wavefront(det), torch.cuda.synchronize()))
    print(json.dumps({**common, "what": "wavefront", **retrace}), flush=True)
    strehl = timed(lambda: frame.psf(det, world_unit_um=1000.0, pixels=1))
    print(json.dumps({**common, "what": "psf", "pixels": 1, **strehl}), flush=True)
    wave = frame.wavefront(det, weights="intensity")
    for K in args.K:
        parameters = parameters_of(lens, det, K)
        first = timed(lambda: frame.sensitivity(det, parameters, [lens, det], wavefront=wave))
        print(json.dumps({**common, "what": "sensitivity", "K": K, **first}), flush=True)
        sens = frame.sensitivity(det, parameters, [lens, det], wavefront=wave)
        widths = [1e-4] * K
        for M in args.trials:
            trials = pyrayt.Tolerances(widths, "normal", seed=M).sample(M)
            run = lambda: sens.tolerance(trials, world_unit_um=1000.0, compensators=("tilt", "focus"))  # noqa: E731
            got = run()
            new = timed(run)
            retraces = M * (retrace["ms"] + strehl["ms"])
            pairs = int(got.n_rays.sum()) * (M + 1)
            print(json.dumps({**common, "what": "tolerance", "K": K, "columns": K + 3, "trials": M, **new,
                              "with_sensitivity_ms": new["ms"] + first["ms"], "retraces_ms": retraces,
                              "retraces_over_one_pass": retraces / (new["ms"] + first["ms"]),
                              "ray_trial_pairs_per_s": pairs / (new["ms"] * 1e-3), "n_rays": int(got.n_rays.sum()),
                              "n_unfollowed": int(got.n_unfollowed.sum()), "nominal_strehl": float(got.nominal.strehl[0]),
                              "yield_0.8": float(got.yield_(0.8)[0])}), flush=True)


if __name__ == "__main__":
    main()
