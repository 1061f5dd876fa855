#!/usr/bin/env python3
"""Wavefront sensitivities of the frame on the device (DeviceFrame.sensitivity(wavefront=), the entry point
prt_frame_opd_sensitivity), timed after warm-up on BASELINE config 2 at --rays rays (3 generations, two refractions a ray),
for K = 1, 6 and 16 parameters (--K to choose), in the manner of tools/design_sensitivity_bench.py:

  opd           DeviceFrame.sensitivity(wavefront=w) end to end, w a Wavefront computed before (J = 15): the new call
  opd_true      the same with wavefront=True: the wavefront pass inside the call
  design        the same parameters without wavefront=: prt_frame_design_sensitivity, on the same box and frame
  wavefront     one DeviceFrame.wavefront() of the frame, for scale
  differences   what central differences cost for the same derivatives: 2 K times (apply the parameter, trace_wavefront --
                which takes the scene update --, apply it back); measured on the first shape parameter

On a tree without the wavefront form (the parent commit) `opd` and `opd_true` are left out and the rest is measured as it
is there: the figures the new call is set beside.  One clock for all: the host's, around calls that end in a synchronise.
A window is as many calls as fill --window-ms (default 300 ms); each figure is the median of --repeats windows, with the
smallest and largest beside it.  Prints one JSON line per figure.
usage: tools/opd_sensitivity_bench.py [--rays N] [--repeats R] [--window-ms MS] [--K 1 6 16]"""
import argparse
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import scenes  # noqa: E402
import pyrayt_amd as pyrayt  # noqa: E402
from design_sensitivity_bench import design_of  # noqa: E402
from sensitivity_bench import windows  # noqa: E402


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
    has_form = "wavefront" in inspect.signature(frame.sensitivity).parameters
    common = {"device": torch.cuda.get_device_name(0), "rays": args.rays, "rows": len(frame),
              "generations": len(frame.rows_per_generation), "window_ms": args.window_ms, "repeats": args.repeats,
              "wavefront_form": has_form}
    wave = frame.wavefront(det, weights="intensity")
    one = windows(lambda: (frame.wavefront(det, weights="intensity"), torch.cuda.synchronize()), args.repeats, args.window_ms)
    print(json.dumps({**common, "what": "wavefront", **one, "rms": wave.rms.tolist()}), flush=True)
    radius = design_of(lens, det, 1)[0]
    h = 2.0 ** -12

    def two_traces():  # (one parameter's central difference: the scene changes, so each trace takes a scene update)
        radius.apply(h)
        tracer.trace_wavefront(det, weights="intensity")
        radius.apply(-2 * h * 2 / (2 + h))  # ((R + h) scaled back to R - h: the amount is in the own frame's units)
        tracer.trace_wavefront(det, weights="intensity")
        radius.apply(h * 2 / (2 - h))
        torch.cuda.synchronize()

    pair = windows(two_traces, args.repeats, args.window_ms)
    print(json.dumps({**common, "what": "differences", "K": 1, **pair}), flush=True)
    for K in args.K:
        design = design_of(lens, det, K)
        plain = windows(lambda: frame.sensitivity(det, design, [lens, det]), args.repeats, args.window_ms)
        print(json.dumps({**common, "what": "design", "K": K, **plain, "differences_ms": K * pair["ms"]}), flush=True)
        if not has_form:
            continue
        got = frame.sensitivity(det, design, [lens, det], wavefront=wave)
        took = windows(lambda: frame.sensitivity(det, design, [lens, det], wavefront=wave), args.repeats, args.window_ms)
        whole = windows(lambda: frame.sensitivity(det, design, [lens, det], wavefront=True), args.repeats, args.window_ms)
        print(json.dumps({**common, "what": "opd_true", "K": K, **whole}), flush=True)
        print(json.dumps({**common, "what": "opd", "K": K, **took, "design_ms": plain["ms"],
                          "opd_over_design": took["ms"] / plain["ms"], "differences_ms": K * pair["ms"],
                          "differences_over_opd": K * pair["ms"] / took["ms"], "n_unfit": got.n_unfit,
                          "n_missed": got.n_missed.tolist(), "rms_opd_gradient": got.rms_opd_gradient[0].tolist()[:4]}),
              flush=True)


if __name__ == "__main__":
    main()
