#!/usr/bin/env python3
"""Monte Carlo tolerancing of the geometric MTF on the device (Sensitivity.mtf_tolerance, the entry point
prt_frame_mtf_tolerance), timed after warm-up on config 2's lens at --rays rays (3 generations), for K = 6 and 16
parameters (--K to choose), M = 33 (a sensitivity table of 16 parameters), 1 000 and 10 000 trials (--trials to choose) and
8 and 256 outputs (--outputs: 2 planes x 2 azimuths x 2 or 64 frequencies), in the manner of tools/tolerance_bench.py:

  sensitivity    DeviceFrame.sensitivity(..., slopes=True) with K design parameters: what mtf_tolerance needs first
  mtf_tolerance  Sensitivity.mtf_tolerance on that result with the "focus" compensator, end to end (the staging, the
                 moments, the focus, the sum, the fold and the read-back of the outputs)
  retrace        the lens moved by a Motion on the host, then one trace_mtf() of the same rays and outputs: what the route
                 without this pass pays per perturbed system (existing code: the same at the parent commit)
  retraces       M x retrace, from the figure above

One clock for all: the host's, around calls that end in a synchronise.  A window is as many calls as fill --window-ms
(default 300 ms); each figure is the median of --repeats windows, with the smallest and largest beside it.  Prints one
JSON line per figure and appends it to --out (default profiles/mtf_tolerance/mtf_tolerance_bench.jsonl); (ray, trial,
output) triples per second are rays kept x (M + 1) x outputs over the call's time (the nominal trial rides along).
--once runs every call once after a warm-up, for a kernel trace in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/mtf_tolerance_bench.py --once) that gives k_mtft_sum and k_mtft_moments
alone.
usage: tools/mtf_tolerance_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 6 16] [--trials 33 1000 10000]
                                    [--outputs 8 256] [--out FILE] [--once]"""
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
    ap.add_argument("--K", type=int, nargs="+", default=[6, 16])
    ap.add_argument("--trials", type=int, nargs="+", default=[33, 1000, 10000])
    ap.add_argument("--outputs", type=int, nargs="+", default=[8, 256])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mtf_tolerance", "mtf_tolerance_bench.jsonl"))
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

    def sampling(outputs):
        assert outputs % 4 == 0, "outputs: 2 planes x 2 azimuths x frequencies"
        return dict(frequencies=np.linspace(0.0, 3.0, outputs // 4), azimuths=(0.0, 90.0), focus=(0.0, 0.05))

    sign = [1.0]

    def perturbed(options):  # (the lens moved and moved back in turn, so that the system stays where it is)
        lens.move_y(sign[0] * 1e-6)
        sign[0] = -sign[0]
        tracer.trace_mtf(det, **options)
        torch.cuda.synchronize()

    retrace = {}
    for outputs in args.outputs:
        options = sampling(outputs)
        retrace[outputs] = timed(lambda: perturbed(options))
        emit({"what": "retrace", "outputs": outputs, **retrace[outputs]})
    for K in args.K:
        parameters = parameters_of(lens, det, K)
        first = timed(lambda: frame.sensitivity(det, parameters, [lens, det], slopes=True))
        emit({"what": "sensitivity", "K": K, **first})
        sens = frame.sensitivity(det, parameters, [lens, det], slopes=True)
        widths = [1e-3] * K
        for outputs in args.outputs:
            options = sampling(outputs)
            for M in args.trials:
                trials = pyrayt.Tolerances(widths, "normal", seed=M).sample(M)
                run = lambda: sens.mtf_tolerance(trials, compensators=("focus",), **options)  # noqa: E731
                got = run()
                new = timed(run)
                retraces = M * retrace[outputs]["ms"]
                triples = int(got.n_rays.sum()) * (M + 1) * outputs
                emit({"what": "mtf_tolerance", "K": K, "outputs": outputs, "trials": M, **new,
                      "with_sensitivity_ms": new["ms"] + first["ms"], "retraces_ms": retraces,
                      "retraces_over_one_pass": retraces / (new["ms"] + first["ms"]),
                      "ray_trial_output_triples_per_s": triples / (new["ms"] * 1e-3), "n_rays": int(got.n_rays.sum()),
                      "n_unfollowed": int(got.n_unfollowed.sum()), "nominal_mtf_top": float(got.nominal.mtf[0, 0, 0, -1]),
                      "yield_0.3_top": float(got.yield_(0.3, frequency=-1)[0])})


if __name__ == "__main__":
    main()
